#!/usr/bin/env python3
"""A node's Tick under raftq_set_check_quorum + raftq_set_pre_vote, the fused calls raftq_tick_set_checks opens against the sequence
they replace -- one process, three handles in the same state, alternated call by call:

  fused     the switches on, raftq_tick_set_checks on: (a) raftq_tick_collect_lists, (b) raftq_tick_frames, (c) raftq_tick_elect_frames
  sequence  the switches on, the fused calls closed (the parent's only route): raftq_tick with counts, raftq_collect_hups / _beats /
            _checks; for (b) also raftq_wire_encode of the heartbeat records; for (c) also raftq_step_batch of the MsgHup records and
            raftq_wire_encode of the heartbeat and MsgPreVote records.  The records are built on the host OUTSIDE the clock (once, from
            the same state), as in the README's other legs.
  plain     both switches off: the same fused call (the parent gives this figure for that handle; its election round campaigns).

Shapes: 1M groups x 3 and x 5 peers; one group in eight led and beating on every tick (heartbeat_tick 1), every leader's check due on the
timed tick, one in a hundred failing; every 20th group a follower whose election timer fires.  A call moves the state, so before every
timed call the roles, the timers and the activity words are put back and one untimed no-op Step batch re-reads the records' copies
of the dense arrays.  Per leg: median, min, max, p10 / p90 of CALLS timed calls after WARM untimed ones, host clock around calls
that end in the device wait.  Counts are compared on every call; byte parity is tests/test_tick_checks_gpu.py's business.

usage: tools/profile_tick_checks.py [out.json]      (default profiles/r28/tick_checks.json; CALLS, WARM from the environment)
Needs the GPU: no CPU path exists, and without a device the handle cannot be created."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = int(os.environ.get("CALLS", "30"))
WARM = int(os.environ.get("WARM", "4"))
ET = 10
MSG_HUP, MSG_BEAT, MSG_HEARTBEAT, MSG_PRE_VOTE = 0, 1, 8, 17


def stats(ns):
    a = np.sort(np.asarray(ns, np.float64)) / 1e3
    return {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a[0]), 1), "max_us": round(float(a[-1]), 1),
            "p10_us": round(float(a[len(a) // 10]), 1), "p90_us": round(float(a[(len(a) * 9) // 10]), 1), "calls": len(a)}


def shape(G, N, device=0):
    from raftsql_amd import step as S
    from raftsql_amd.engine import pinned_empty
    from raftsql_amd.wire import WIRE_MSG_DT, WireEngine

    me = 0
    rng = np.random.default_rng(28 + N)
    idx = np.arange(G)
    lead, fire = idx % 8 == 1, idx % 20 == 0
    lead &= ~fire
    role = np.where(lead, 2, 0).astype(np.uint8)
    elapsed = np.where(fire, 2 * ET - 1, 0).astype(np.uint32)  # one tick short of a timeout no draw exceeds
    full = (1 << N) - 1
    active = np.full(G, full, np.uint16)
    active[lead & (rng.random(G) < 0.01)] = 0
    le = np.where(lead, ET - 1, 0).astype(np.uint32)
    term = rng.integers(1, 1 << 20, G).astype(np.uint64)
    last = rng.integers(1, 1 << 30, G).astype(np.uint64)
    match = np.zeros((N, G), np.uint64)
    match[:, lead] = last[lead] // 2
    match[me] = last
    committed = np.where(lead, last // 2, 0).astype(np.uint64)
    fails = lead & (active == 0)
    n_fire, n_beat, n_chk = int(fire.sum()), int((lead & ~fails).sum()), int(fails.sum())
    slices = N - 1
    quiet = np.array([2], np.uint64)  # a follower whose timer does not fire: a MsgBeat to it does nothing

    def engine(cq, checks):
        e = WireEngine(G, N, me, device=device)
        e.set_timers(ET, 1, 7)
        if cq:
            e.set_check_quorum(True)
            e.set_pre_vote(True)
        e.load_match(match, committed)
        e.load_terms(np.where(lead, term, 0), lead.astype(np.uint64))
        e.load_roles(role, elapsed)
        e.load_node(term, np.where(lead, me + 1, 0).astype(np.uint32), np.where(lead, me + 1, 0).astype(np.uint32), last, term)
        if checks:
            e.set_tick_checks(G)
        return e

    fus, seq, pl = engine(True, True), engine(True, False), engine(False, False)
    noop = S.pack_msgs(quiet, MSG_BEAT)

    def reset(e, cq=True):
        e.load_roles(role, elapsed)
        if cq:
            e.load_activity(active, le)
        e.step_batch(noop)

    try:
        cap = fus.respond_cap(n_beat + n_fire)
        n_frames = (n_beat + n_fire) * slices
        out = pinned_empty(cap, np.uint8)
        off = pinned_empty(n_frames + 1, np.uint64)
        po = pinned_empty(2 * (N + 1), np.uint64)
        camp = pinned_empty(n_fire, S.OUT_S_DT)
        # the sequence's host-built records, made once outside the clock: the heartbeats of the beating leaders, the MsgHups, the MsgPreVotes
        beats, hups = np.flatnonzero(lead & ~fails), np.flatnonzero(fire)
        recs = pinned_empty(n_frames, WIRE_MSG_DT)
        recs[:] = np.zeros(1, WIRE_MSG_DT)[0]
        at = 0
        for p in range(1, N):
            r = recs[at:at + n_beat]
            r["group"], r["term"], r["type"], r["to"], r["from"], r["commit"] = beats, term[beats], MSG_HEARTBEAT, p, me, committed[beats]
            at += n_beat
        for p in range(1, N):
            r = recs[at:at + n_fire]
            r["group"], r["term"], r["type"], r["to"], r["from"] = hups, term[hups] + 1, MSG_PRE_VOTE, p, me
            r["index"], r["log_term"] = last[hups], term[hups]
            at += n_fire
        hup_msgs = S.pack_msgs(hups.astype(np.uint64), MSG_HUP)

        def sequence(leg):
            t0 = time.perf_counter_ns()
            nh, nb = seq.tick()
            seq.collect_hups()
            seq.collect_beats()
            _, nc = seq.collect_checks()
            if leg == "c":
                seq.step_batch(hup_msgs)
            if leg != "a":
                n = n_beat * slices if leg == "b" else n_frames
                seq.wire_encode(recs[:n], out=out, off=off[: n + 1])
            dt = time.perf_counter_ns() - t0
            assert (nh, nb, nc) == (n_fire, n_beat, n_chk), (nh, nb, nc)
            return dt

        def fused(e, leg, cq):
            t0 = time.perf_counter_ns()
            if leg == "a":
                _, nh, _, nb = e.tick_collect_lists(G, 0, beat_bitmap=True)
                frames = 0
            elif leg == "b":
                r = e.tick_frames(out, off[: n_beat * slices + 1], po, n_beat, beat_bitmap=True, cap=cap)
                nh, nb, frames = r[5], r[7], int(r[3].n_msgs)
            else:
                r = e.tick_elect_frames(camp, out, off, po, n_fire, n_beat, beat_bitmap=True, cap=cap)
                nh, nb, frames = r[6], r[8], int(r[3].n_msgs)
            nc = e.last_tick_checks()[1] if cq else 0
            dt = time.perf_counter_ns() - t0
            want_beat = n_beat if cq else n_beat + n_chk  # (without the switch nobody's check fails: every leader beats)
            want_frames = {"a": 0, "b": want_beat * slices, "c": (want_beat + n_fire) * slices}[leg]
            assert (nh, nb, nc, frames) == (n_fire, want_beat, n_chk if cq else 0, want_frames), (leg, cq, nh, nb, nc, frames)
            return dt

        legs = {}
        for leg in "abc":
            t = {"fused": [], "sequence": [], "plain": []}
            for i in range(WARM + CALLS):
                reset(fus)
                a = fused(fus, leg, True)
                reset(seq)
                b = sequence(leg)
                reset(pl, cq=False)
                c = fused_plain(pl, leg, fused, n_beat + n_chk, n_fire, slices, G, camp, po) if leg != "a" else fused(pl, leg, False)
                if i >= WARM:
                    t["fused"].append(a)
                    t["sequence"].append(b)
                    t["plain"].append(c)
            f, s, p = (stats(t[k]) for k in ("fused", "sequence", "plain"))
            legs[leg] = {"fused": f, "sequence": s, "plain_handle_same_call": p, "sequence_over_fused": round(s["median_us"] / f["median_us"], 2),
                         "fused_over_plain": round(f["median_us"] / p["median_us"], 2)}
        return {"groups": G, "peers": N, "hups_per_tick": n_fire, "beats_per_tick": n_beat, "failed_checks_per_tick": n_chk,
                "frames_b": n_beat * slices, "frames_c": n_frames,
                "legs": {"a_tick_collect_lists": legs["a"], "b_tick_frames": legs["b"], "c_tick_elect_frames": legs["c"]}}
    finally:
        for e in (fus, seq, pl):
            e.close()


_PLAIN = {}


def fused_plain(e, leg, fused, n_beat_all, n_fire, slices, G, camp, po):
    """the plain handle's call: every leader beats (nobody's check fails without the switch), so its buffers are a little larger"""
    from raftsql_amd.engine import pinned_empty

    key = (id(e), leg)
    if key not in _PLAIN:
        n = (n_beat_all + (n_fire if leg == "c" else 0)) * slices
        _PLAIN[key] = (pinned_empty(e.respond_cap(n_beat_all + n_fire), np.uint8), pinned_empty(n + 1, np.uint64))
    out, off = _PLAIN[key]
    t0 = time.perf_counter_ns()
    if leg == "b":
        r = e.tick_frames(out, off, po, n_beat_all, beat_bitmap=True, cap=len(out))
        nh, nb, frames = r[5], r[7], int(r[3].n_msgs)
        want = n_beat_all * slices
    else:
        r = e.tick_elect_frames(camp, out, off, po, n_fire, n_beat_all, beat_bitmap=True, cap=len(out))
        nh, nb, frames = r[6], r[8], int(r[3].n_msgs)
        want = (n_beat_all + n_fire) * slices
    dt = time.perf_counter_ns() - t0
    assert (nh, nb, frames) == (n_fire, n_beat_all, want), (leg, nh, nb, frames)
    return dt


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r28", "tick_checks.json")
    import torch

    assert torch.cuda.is_available(), "tools/profile_tick_checks.py measures on the GPU; there is none here"
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    rec = {"what": "the fused Tick calls under raftq_set_check_quorum + raftq_set_pre_vote (raftq_tick_set_checks) against raftq_tick + "
                   "raftq_collect_hups / _beats / _checks (+ raftq_step_batch of the MsgHups, + raftq_wire_encode of host-built records), and "
                   "against the same call on a handle with both switches off; alternated",
           "device": torch.cuda.get_device_name(0), "tree": head, "calls": CALLS, "warm": WARM, "clock": "time.perf_counter_ns around calls that wait",
           "shapes": [shape(1 << 20, 3), shape(1 << 20, 5)]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
