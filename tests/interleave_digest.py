"""sha256 over the interleave suite's schedules (tests/ref_interleave.py): per schedule the kinds of its moves in order, every batch's
bytes and every expected result record's bytes.  Run at two commits to show that a change left the existing schedules byte for byte
as they were:

  python -m tests.interleave_digest                   the five schedules of round 26
  python -m tests.interleave_digest   n3-all-safe ... the named cases' schedules
  python -m tests.interleave_digest   --report        the schedules with PreVote, transfer and ReadIndex on: moves per kind, how many
                                                    state-changing moves the batch behind them tells from their absence, and per
                                                    Step rule of the three switches the number of batches that change without it

CPU only; nothing here touches a device.  TEST INFRASTRUCTURE: nothing in the product imports it."""
import hashlib
import sys
import time

R26 = ("n3", "n9", "n5-masked", "n3-cq", "n5-masked-cq")


def digest(case):
    from tests import ref_interleave as I

    h = hashlib.sha256()
    sch = I.schedule(case)
    for mv in sch.moves:
        h.update(mv.kind.encode() + b"\0")
        for m, w in zip(mv.batches, mv.wants):
            h.update(m.tobytes())
            h.update(w.tobytes())
    return h.hexdigest(), len(sch.moves)


def report():
    from tests import ref_interleave as I

    for case in sorted(set(I.CASES[k]["schedule"] for k in I.EXTENDED)):
        sch = I.schedule(case)
        kinds = I.counts(sch)
        held = [mv for mv in sch.moves if mv.kind not in I.no_change(case)]
        seen = sum(len(I.discriminates(mv)) >= 1 for mv in held)
        n_batches = sum(len(mv.batches) for mv in sch.moves)
        print(f"{case}: {len(sch.moves)} moves, {n_batches} batches, {sum(len(m) for mv in sch.moves for m in mv.batches)} Step records, "
              f"reference {sch.ref_seconds:.2f} s; seen {seen} of {len(held)}")
        print("  kinds: " + ", ".join(f"{k} {v}" for k, v in sorted(kinds.items())))
        t0 = time.perf_counter()
        rules = [f"{which} {rule}: {I.batches_changed_without(sch, which, rule)}" for which, rule in I.case_rules(case)]
        print(f"  batches of {n_batches} that change without the rule -- " + ", ".join(rules) + f" ({time.perf_counter() - t0:.1f} s)")


def main(argv):
    from oracle import pyoracle

    pyoracle.build()
    pyoracle.lib()
    if argv == ["--report"]:
        return report()
    whole = hashlib.sha256()
    for case in argv or R26:
        d, n = digest(case)
        whole.update(d.encode())
        print(f"{case:16s} {n:3d} moves  {d}")
    print(f"{'all':16s}            {whole.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1:])
