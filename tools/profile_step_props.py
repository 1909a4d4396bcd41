#!/usr/bin/env python3
"""What raftq_step_set_props buys a node's inbound half-turn: 65,536 frames addressed to a leader of G = 16,384 groups of three
(four frames per group and call on average), MsgAppResp from both followers and, for 0 %, 25 % and 66 % of the frames, a
follower's forwarded MsgProp with one 16-byte entry.

  A  switch off: one raftq_step_frames call -- every MsgProp is RAFTQ_OUT_HELD, whatever follows it in its group
     RAFTQ_OUT_DEFERRED -- plus the second Step round for the deferred records: staged into raftq_step_stage's array and stepped
     with raftq_step_batch.  Picking the deferred records out of the results and the host's handling of the held proposals
     (its own appendEntry and the tail report) are NOT charged.
  B  switch on: one raftq_step_frames call.

Two handles in the same state, A and B alternated, 5 warm-up and 25 timed repetitions per setting; wall time of the calls (each
ends in its own wait), median and min-max in microseconds.  Before anything is timed B's results are checked: no HELD, no
DEFERRED, one RAFTQ_OUT_PROPOSED per MsgProp frame.
usage: tools/profile_step_props.py [out.json]      (run on the GPU box)"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import step as S  # noqa: E402
from raftsql_amd.engine import pinned_copy, pinned_empty  # noqa: E402
from raftsql_amd.wire import WIRE_ENT_DT, WIRE_MSG_DT, WireEngine  # noqa: E402

N, G, FRAMES, WARM, REPS = 3, 16384, 65536, 5, 25
SHARES = (0.0, 0.25, 0.66)


def engine(props, last):
    e = WireEngine(G, N, 0)
    term = np.full(G, 3, np.uint64)
    match = np.stack([last, last // 2, last // 3]).astype(np.uint64)
    e.load_match(match, (last // 3).astype(np.uint64))
    e.load_terms(term, np.ones(G, np.uint64))
    e.load_roles(np.full(G, 2, np.uint8))
    e.load_node(term, np.ones(G, np.uint32), np.ones(G, np.uint32), last, term)
    e.set_step_props(props)
    return e


def frames(rng, e, last, share):
    w = np.zeros(FRAMES, WIRE_MSG_DT)
    g = rng.integers(0, G, FRAMES)
    prop = rng.random(FRAMES) < share
    w["group"], w["from"], w["to"] = g, rng.integers(1, N, FRAMES), 0
    w["type"] = np.where(prop, S.MSG_PROP, S.MSG_APP_RESP)
    w["term"] = np.where(prop, 0, 3)
    w["index"] = np.where(prop, 0, (last[g] * rng.random(FRAMES)).astype(np.uint64))
    w["n_ents"] = prop
    w["ent_first"] = np.where(prop, np.cumsum(prop) - prop, 0)
    ents = np.zeros(int(prop.sum()), WIRE_ENT_DT)
    ents["data_len"], ents["data_off"] = 16, 16 * np.arange(len(ents))
    pool = rng.integers(0, 256, 16 * len(ents) + 1, dtype=np.uint8)
    stream, off = e.wire_encode(w, ents, pool)
    return pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64)), int(prop.sum())


def main():
    rng = np.random.default_rng(2121)
    last = rng.integers(50, 100, G).astype(np.uint64)
    a, b = engine(False, last), engine(True, last)
    msgs, ents = pinned_empty(FRAMES, WIRE_MSG_DT), pinned_empty(FRAMES, WIRE_ENT_DT)
    rec = {"what": "a leader's inbound half-turn, %d frames over %d groups x %d: MsgAppResp + the given share of forwarded MsgProp (one 16-byte "
                   "entry); A = switch off, raftq_step_frames + the second Step round for the deferred records, B = switch on, one call; "
                   "%d warm-up and %d timed repetitions, A and B alternated, wall us" % (FRAMES, G, N, WARM, REPS), "settings": {}}
    for share in SHARES:
        ps, po, n_props = frames(rng, a, last, share)
        # the records of A's second round, picked once: what is deferred depends on the frames' order alone
        gm, _, out_a, _ = a.step_frames(ps, po, msgs, ents)
        deferred = np.flatnonzero(out_a["type"] == S.OUT_DEFERRED)
        assert int((out_a["type"] == S.OUT_HELD).sum()) == n_props
        second = np.zeros(len(deferred), S.MSG_DT)
        for k in ("group", "term", "log_term", "index", "commit", "reject_hint", "from", "type", "reject"):
            second[k] = gm[k][deferred]
        _, _, out_b, _ = b.step_frames(ps, po, msgs, ents)
        t = out_b["type"]
        assert int((t == S.OUT_PROPOSED).sum()) == n_props and not np.isin(t, (S.OUT_HELD, S.OUT_DEFERRED)).any()
        if len(second):
            a.step_batch(second)
        times = {"A": [], "A_frames_call": [], "B": []}
        for r in range(WARM + REPS):
            for which in (("A", "B") if r % 2 == 0 else ("B", "A")):
                t0 = time.perf_counter()
                if which == "A":
                    a.step_frames(ps, po, msgs, ents, copy=False)
                    t1 = time.perf_counter()
                    if len(second):
                        st = a.step_stage(len(second))
                        ctypes.memmove(st.ctypes.data, second.ctypes.data, second.nbytes)
                        a.step_inplace(st)
                else:
                    b.step_frames(ps, po, msgs, ents, copy=False)
                    t1 = t0
                t2 = time.perf_counter()
                if r >= WARM:
                    times[which].append((t2 - t0) * 1e6)
                    if which == "A":
                        times["A_frames_call"].append((t1 - t0) * 1e6)
        row = {"msgprop_frames": n_props, "deferred_records_in_A": int(len(deferred))}
        for k, v in times.items():
            v = np.array(v)
            row[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(v.min()), 1), "max_us": round(float(v.max()), 1)}
        row["B_over_A"] = round(row["B"]["median_us"] / row["A"]["median_us"], 3)
        row["ranges_overlap"] = bool(row["B"]["min_us"] <= row["A"]["max_us"] and row["A"]["min_us"] <= row["B"]["max_us"])
        rec["settings"]["%d%%" % round(100 * share)] = row
    a.close()
    b.close()
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
