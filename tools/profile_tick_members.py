#!/usr/bin/env python3
"""raftq_tick_frames and raftq_tick_elect_frames over each group's own members (raftq_tick_set_voters: tick_voters_kernel,
beat_build_voters_kernel, elect_build_voters_kernel) against the same calls on a handle without masks -- the parent's path.
Two handles of one shape in the same state, in one process:
  unmasked   no masks loaded
  masked     random masks (ref: uniform in [1, 2^N)), the switch on
Shapes 32,768 x 3 and 1M x 5; an eighth of the groups is led by this node (HeartbeatTick 1: every leader beats on every tick),
the other timers are spread over two election timeouts, so some fire on every tick.  beat_cap = the leaders, hup_cap = 16,384.
The two settings are ALTERNATED five times, 20 calls a turn after a warm-up turn; per setting and call the median and the range of
the five turns' medians, wall time of the whole call (one submission, one wait).
What is expected, by bytes: the masked Tick moves 12 B per group where the plain one moves 10; the build kernels read two more
bytes per built group and write the same number of records; the encoder writes fewer bytes (a non-member's slot takes none); the
masked call adds an 8-byte memset and a one-thread kernel.
usage: tools/profile_tick_members.py [out.json]      (run on the GPU box)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd.engine import pinned_empty  # noqa: E402
from raftsql_amd.step import OUT_S_DT  # noqa: E402
from raftsql_amd.wire import WireEngine  # noqa: E402

SHAPES = ((32768, 3), (1 << 20, 5))
ET, HB, SEED, HUP_CAP, CALLS, TURNS = 10, 1, 0x7157, 16384, 20, 5
SETTINGS = ("unmasked", "masked")


def make(G, N, masked, rng):
    me = 0
    role = np.where(np.arange(G) % 8 == 0, 2, 0).astype(np.uint8)
    lead = role == 2
    term = rng.integers(1, 1000, G).astype(np.uint64)
    last = rng.integers(50, 100000, G).astype(np.uint64)
    match = (last[None, :] * rng.random((N, G))).astype(np.uint64)
    match[me] = last
    committed = (last * rng.random(G)).astype(np.uint64)
    elapsed = np.where(lead, 0, rng.integers(0, 2 * ET, G)).astype(np.uint32)
    e = WireEngine(G, N, me)
    e.set_timers(ET, HB, SEED)
    e.load_match(match, committed)
    e.load_terms(np.where(lead, term, 0), lead.astype(np.uint64))
    e.load_roles(role, elapsed)
    e.load_node(term, np.where(lead, me + 1, 0).astype(np.uint32), np.where(lead, me + 1, 0).astype(np.uint32), last, term)
    if masked:
        e.load_voters(rng.integers(1, 1 << N, G).astype(np.uint16))
        e.set_tick_voters(True)
    return e, int(lead.sum())


def main():
    rec = {"what": "wall us per call (one submission, one wait); two handles of one shape in one process, the settings alternated %d times, %d calls a "
                   "turn after a warm-up turn; median and range of the turns' medians" % (TURNS, CALLS),
           "expectation_by_bytes": "masked Tick 12 B per group against 10; the build kernels +2 B read per built group, the same records written; fewer "
                                   "bytes encoded; + one 8-byte memset and a one-thread kernel per call",
           "shapes": {}}
    for G, N in SHAPES:
        engines, bufs = {}, {}
        for s in SETTINGS:
            e, n_lead = make(G, N, s == "masked", np.random.default_rng(99))
            engines[s] = e
            n_max = (n_lead + HUP_CAP) * (N - 1)
            bufs[s] = dict(out=pinned_empty(e.respond_cap(n_lead + HUP_CAP), np.uint8), off=pinned_empty(n_max + 1, np.uint64),
                           po=pinned_empty(2 * (N + 1), np.uint64), camp=pinned_empty(HUP_CAP, OUT_S_DT), beat_cap=n_lead)
        shape = {}
        for call in ("raftq_tick_frames", "raftq_tick_elect_frames"):
            meds = {s: [] for s in SETTINGS}
            last = {}
            for turn in range(TURNS + 1):  # turn 0 warms both handles up and is dropped
                for s in SETTINGS if turn % 2 == 0 else SETTINGS[::-1]:
                    e, b = engines[s], bufs[s]
                    ts = []
                    for _ in range(CALLS):
                        t0 = time.perf_counter()
                        if call == "raftq_tick_frames":
                            r = e.tick_frames(b["out"], b["off"], b["po"], b["beat_cap"], hup_cap=HUP_CAP, beat_bitmap=True)
                            c, nh, nb = r[3], r[5], r[7]
                        else:
                            r = e.tick_elect_frames(b["camp"], b["out"], b["off"], b["po"], HUP_CAP, b["beat_cap"], beat_bitmap=True)
                            c, nh, nb = r[3], r[6], r[8]
                        ts.append((time.perf_counter() - t0) * 1e6)
                    last[s] = {"n_hup": int(nh), "n_beat": int(nb), "frames_with_bytes": int(c.n_msgs), "bytes": int(c.bytes)}
                    if turn:
                        meds[s].append(float(np.median(ts)))
            shape[call] = {s: {"median_us": round(float(np.median(meds[s])), 1), "min_us": round(min(meds[s]), 1), "max_us": round(max(meds[s]), 1),
                               "last_call": last[s]} for s in SETTINGS}
            shape[call]["masked_over_unmasked"] = round(shape[call]["masked"]["median_us"] / shape[call]["unmasked"]["median_us"], 3)
        rec["shapes"]["%dx%d" % (G, N)] = shape
        for e in engines.values():
            e.close()
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
