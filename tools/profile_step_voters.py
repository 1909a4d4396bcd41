#!/usr/bin/env python3
"""Step over each group's own voters (step_lists_voters_kernel) against the unmasked step_lists_kernel, one process, 1M x 5:
64K-message batches of the bench's Step mix (75 % acks / 20 % heartbeat responses / 5 % higher-term votes, every group led by
this node), pipelined three deep from the staging slots, 32-byte result records -- bench.py's step_measure (d') leg.  Three
handles in the same state, their batches alternated:
  unmasked        no masks loaded
  masked_full     opted in (raftq_step_set_voters), every mask full
  masked_random   opted in, random masks
Before anything is timed every handle steps the same batches synchronously and the result records are compared: masked_full
must give unmasked's bytes; masked_random's must differ (the masks decide something).  Then 100 timed batches per handle in
runs of 10, the handles' order rotated from run to run; per handle the median and min-max of the per-batch wall time.
usage: tools/profile_step_voters.py [out.json]      (run on the GPU box)"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import step as S  # noqa: E402

N, G, MSGS, RUN, RUNS = 5, 1 << 20, 65536, 10, 10
VARIANTS = ("unmasked", "masked_full", "masked_random")


def main():
    rng = np.random.default_rng(77)
    term = np.full(G, 3, np.uint64)
    last = rng.integers(50, 100, G).astype(np.uint64)
    match = (last[None, :] * rng.random((N, G))).astype(np.uint64)
    match[0] = last
    committed = np.sort(match, axis=0)[N - (N // 2 + 1)] // 2
    masks = {"unmasked": None, "masked_full": np.full(G, (1 << N) - 1, np.uint16), "masked_random": rng.integers(1, 1 << N, G).astype(np.uint16)}

    def batch():
        g = rng.integers(0, G, MSGS).astype(np.uint64)
        u = rng.random(MSGS)
        t = np.where(u < 0.75, S.MSG_APP_RESP, np.where(u < 0.95, S.MSG_HEARTBEAT_RESP, S.MSG_VOTE)).astype(np.uint8)
        mt = np.where(t == S.MSG_VOTE, 4, np.where(rng.random(MSGS) < 0.02, 2, 3)).astype(np.uint64)
        return S.pack_msgs(g, t, term=mt, frm=rng.integers(1, N, MSGS), index=(last[g] * rng.random(MSGS)).astype(np.uint64), log_term=3)

    bs = [batch() for _ in range(6)]
    engines = {}
    for v in VARIANTS:
        e = S.NodeEngine(G, N, self_peer=0)
        e.load_match(match, committed)
        e.load_terms(term, np.ones(G, np.uint64))
        e.load_roles(np.full(G, 2, np.uint8))
        e.load_node(term, np.ones(G, np.uint32), np.ones(G, np.uint32), last, term)
        if masks[v] is not None:
            e.load_voters(masks[v])
            e.set_step_voters(True)
        engines[v] = e
    # outputs first: three synchronous batches on every handle
    same_full, differ_random = True, 0
    for b in bs[:3]:
        outs = {v: engines[v].step_batch(b)[0] for v in VARIANTS}
        same_full &= outs["masked_full"].tobytes() == outs["unmasked"].tobytes()
        differ_random += int((outs["masked_random"].view(np.uint8).reshape(-1, 64) != outs["unmasked"].view(np.uint8).reshape(-1, 64)).any(axis=1).sum())
    assert same_full, "full masks must give the unmasked handle's records"
    assert differ_random > 0, "random masks were meant to change some result"
    for e in engines.values():
        e.set_compact(2)

    def prime(e):  # fill all three staging slots once, leave two batches in flight
        for b in bs[3:6]:
            st = e.step_stage(MSGS)
            ctypes.memmove(st.ctypes.data, b.ctypes.data, b.nbytes)
            e.step_submit(st)
        e.step_collect(copy=False)

    per_batch = {v: [] for v in VARIANTS}
    for v in VARIANTS:
        prime(engines[v])
    for r in range(RUNS + 1):  # run 0 warms every handle up and is dropped
        for v in VARIANTS[r % 3:] + VARIANTS[:r % 3]:
            e = engines[v]
            for _ in range(RUN):
                t0 = time.perf_counter()
                e.step_submit(e.step_stage(MSGS))
                e.step_collect(copy=False)
                if r:
                    per_batch[v].append((time.perf_counter() - t0) * 1e6)
    for e in engines.values():
        e.step_collect(copy=False)
        e.step_collect(copy=False)
    rec = {"what": "per 64K-message batch of the bench's Step mix on %d x %d, three batches in flight from the staging slots, 32-byte results; "
                   "three handles in one process, runs of %d batches alternated, %d timed batches each; wall us per batch" % (G, N, RUN, RUN * RUNS),
           "expectation_by_bytes": "masked_full ~ masked_random ~ unmasked x (1 + 32/256) at worst; less while the leg is link-out-bound",
           "masked_full_records_equal_unmasked": bool(same_full), "masked_random_records_that_differ_of_%d" % (3 * MSGS): differ_random, "variants": {}}
    for v in VARIANTS:
        a = np.array(per_batch[v])
        rec["variants"][v] = {"median_us": round(float(np.median(a)), 2), "min_us": round(float(a.min()), 2), "max_us": round(float(a.max()), 2),
                              "msgs_per_s": round(MSGS / (float(np.median(a)) * 1e-6))}
    base = rec["variants"]["unmasked"]["median_us"]
    for v in VARIANTS[1:]:
        rec["variants"][v]["ratio_to_unmasked"] = round(rec["variants"][v]["median_us"] / base, 4)
    for e in engines.values():
        e.close()
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
