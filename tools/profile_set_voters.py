#!/usr/bin/env python3
"""Sweep sets whose members hold voter masks (raftq_set_create_voters, sweep_set_voters_kernel) at the headline shape: 36 handles of
1M groups x 5 peers, commit + votes, streamed, nothing adopted.  One process, three settings:
  (a) set_voters_random    36 handles with random masks, ONE dispatch through a set from raftq_set_create_voters
  (b) many_random          the same 36 handles, each on its own stream, through raftq_sweep_many_async: 36 launches of
                           sweep_voters_kernel -- the only way to sweep them before the set took masks, and the yardstick
  (c) set_voters_full      36 handles with every mask full through the new dispatch, beside
      set_plain            36 handles with no masks through a set from raftq_set_create (sweep_set_kernel: the headline)
Before anything is timed the outputs are compared: (a) and (b) leave the same commit buffers and outcomes on every handle, full
masks leave what no masks leave.  Then five turns, the order of the settings rotated from turn to turn; a turn is one untimed
pass and ten timed ones back to back between two waits; per setting the median and the range of the five per-pass wall times.
usage: tools/profile_set_voters.py [out.json]      (run on the GPU box)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import synth  # noqa: E402
from raftsql_amd._lib import SWEEP_COMMIT, SWEEP_NO_ADOPT, SWEEP_STREAM, SWEEP_VOTES  # noqa: E402
from raftsql_amd.engine import QuorumEngine, SweepSet, sweep_many_async  # noqa: E402

N, G, K, PASSES, TURNS = 5, 1 << 20, 36, 10, 5
FLAGS = SWEEP_COMMIT | SWEEP_VOTES | SWEEP_NO_ADOPT | SWEEP_STREAM
SETTINGS = ("set_voters_random", "many_random", "set_voters_full", "set_plain")


def handles(base, masks):
    es = []
    for k in range(K):
        e = QuorumEngine(G, N)
        e.clone_state_from(base)
        if masks is not None:
            e.load_voters(masks(k))
        es.append(e)
    return es


def main():
    rng = np.random.default_rng(1600)
    st = synth.make_groups(G, N, seed=synth.SEED_BASE + 3)
    base = QuorumEngine(G, N)
    base.load_state(st)
    full = np.full(G, (1 << N) - 1, np.uint16)
    rand = handles(base, lambda k: rng.integers(1, 1 << N, G).astype(np.uint16))
    fulls = handles(base, lambda k: full)
    plain = handles(base, None)

    def many(es):
        sweep_many_async(es, FLAGS)
        for e in es:
            e.wait()

    # outputs first
    many(rand)
    single = [(e.read_committed(), e.read_outcome()) for e in rand[:4]]
    with SweepSet(rand, voters=True) as s:
        s.sweep(FLAGS)
        same_ab = all(np.array_equal(e.read_committed(), c) and np.array_equal(e.read_outcome(), o) for e, (c, o) in zip(rand, single))
    with SweepSet(fulls, voters=True) as sf, SweepSet(plain) as sp:
        _, tf = sf.sweep(FLAGS)
        _, tp = sp.sweep(FLAGS)
        same_c = tf == tp and np.array_equal(fulls[0].read_committed(), plain[0].read_committed()) and \
            np.array_equal(fulls[K - 1].read_outcome(), plain[K - 1].read_outcome())
    differs = not np.array_equal(single[0][0], plain[0].read_committed())
    assert same_ab, "the set dispatch must leave what one launch per handle leaves"
    assert same_c, "full masks must leave what no masks leave"
    assert differs, "random masks were meant to change some commit index"

    def timed(run, wait):
        run()
        wait()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            run()
        wait()
        return (time.perf_counter() - t0) * 1e6 / PASSES

    def measure(name):
        if name == "many_random":  # every handle on its own stream: no set is open
            return timed(lambda: sweep_many_async(rand, FLAGS), lambda: [e.wait() for e in rand])
        es, voters = {"set_voters_random": (rand, True), "set_voters_full": (fulls, True), "set_plain": (plain, False)}[name]
        with SweepSet(es, voters=voters) as s:
            return timed(lambda: s.sweep_async(FLAGS), s.wait)

    per = {v: [] for v in SETTINGS}
    for turn in range(TURNS):
        for v in SETTINGS[turn % 4:] + SETTINGS[:turn % 4]:
            per[v].append(measure(v))
    rec = {"what": "wall us per pass over %d handles of %d x %d, commit + votes, streamed, not adopted; %d turns with the settings' order rotated, "
                   "a turn = one untimed pass and %d timed ones between two waits" % (K, G, N, TURNS, PASSES),
           "set_equals_one_launch_per_handle": bool(same_ab), "full_masks_equal_no_masks": bool(same_c), "settings": {}}
    for v in SETTINGS:
        a = np.array(per[v])
        rec["settings"][v] = {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1), "max_us": round(float(a.max()), 1),
                              "us_per_member": round(float(np.median(a)) / K, 2), "turns_us": [round(float(x), 1) for x in a]}
    r = rec["settings"]
    rec["a_over_b"] = round(r["set_voters_random"]["median_us"] / r["many_random"]["median_us"], 4)
    rec["a_and_b_ranges_disjoint"] = bool(r["set_voters_random"]["max_us"] < r["many_random"]["min_us"] or r["many_random"]["max_us"] < r["set_voters_random"]["min_us"])
    rec["full_over_plain"] = round(r["set_voters_full"]["median_us"] / r["set_plain"]["median_us"], 4)
    rec["random_over_plain"] = round(r["set_voters_random"]["median_us"] / r["set_plain"]["median_us"], 4)
    for e in rand + fulls + plain + [base]:
        e.close()
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
