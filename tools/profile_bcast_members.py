#!/usr/bin/env python3
"""raftq_propose_frames and raftq_step_frames_respond over each group's own members (raftq_bcast_set_voters:
propose_check_voters_kernel, propose_build_voters_kernel, resp_count_voters_kernel, resp_scatter_voters_kernel) against the same
calls on a handle without masks -- the parent's path.  Three handles of one shape in the same state, in one process:
  none     no masks loaded (the unmasked instantiations)
  full     every slot votes, the switch on (the masked instantiations, the same frames)
  random   masks uniform in [1, 2^N) -- for the proposals with self and one other slot made voters, or the call would refuse the
           record -- the switch on (the masked instantiations, fewer frames)
Two calls:
  raftq_propose_frames       32,768 x 3, one statement per group behind 65,536 queued messages (the one-node leg's turn)
  raftq_step_frames_respond  1M x 5, 65,536 frames: two acks for each of 32,768 led groups whose tail was moved one entry on by an
                             (untimed) tail report, every at-tail bit set -- without masks the second ack commits and broadcasts
The settings are ALTERNATED five times, 10 calls a turn after a warm-up turn; per setting the median and the range of the five
turns' medians, wall time of the whole call (one submission, one wait).  What to hold the masked forms against is the `none` setting of
the same run.
What is expected, by construction: full masks move the same frames and add a 2-byte read per proposal or broadcast, for the
proposals an 8-byte memset and a one-thread kernel: a few us.  Random masks send fewer bytes over the link and should be faster.
usage: tools/profile_bcast_members.py [out.json]      (run on the GPU box)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import step as S  # noqa: E402
from raftsql_amd.engine import pinned_copy, pinned_empty  # noqa: E402
from raftsql_amd.wire import PROP_DT, PROP_ENT_DT, WIRE_ENT_DT, WIRE_MSG_DT, WireEngine  # noqa: E402

CALLS, TURNS = 10, 5
SETTINGS = ("none", "full", "random")
ME = 0


def masks_of(setting, G, N, rng, proposals):
    if setting == "none":
        return None
    if setting == "full":
        return np.full(G, (1 << N) - 1, np.uint16)
    v = rng.integers(1, 1 << N, G).astype(np.uint16)
    if proposals:  # self votes and so does one other slot: the record is sound over members
        v |= np.uint16(1 << ME)
        lone = v == (1 << ME)
        v[lone] |= (1 << rng.integers(1, N, int(lone.sum()))).astype(np.uint16)
    return v


def led_engine(G, N, setting, proposals):
    """every group led by slot 0 at term 3; the followers' Match and the commit index one entry below the tail"""
    rng = np.random.default_rng(99)
    last = rng.integers(50, 100000, G).astype(np.uint64)
    term = np.full(G, 3, np.uint64)
    match = np.tile(last - 1, (N, 1))
    match[ME] = last
    e = WireEngine(G, N, ME)
    e.load_match(match, last - 1)
    e.load_terms(term, np.ones(G, np.uint64))
    e.load_roles(np.full(G, 2, np.uint8))
    e.load_node(term, np.full(G, ME + 1, np.uint32), np.full(G, ME + 1, np.uint32), last, term)
    v = masks_of(setting, G, N, np.random.default_rng(7), proposals)
    if v is not None:
        e.load_voters(v)
        e.set_bcast_voters(True)
        e.set_step_voters(True)  # (the untimed tail reports of the respond leg)
    return e, last


def summary(meds, last):
    out = {s: {"median_us": round(float(np.median(meds[s])), 1), "min_us": round(min(meds[s]), 1), "max_us": round(max(meds[s]), 1),
               "last_call": last[s]} for s in SETTINGS}
    for s in SETTINGS[1:]:
        out["%s_over_none" % s] = round(out[s]["median_us"] / out["none"]["median_us"], 3)
    return out


def propose_leg():
    G, N, n_host = 32768, 3, 65536
    rng = np.random.default_rng(5)
    props = np.zeros(G, PROP_DT)
    props["group"], props["n_ents"], props["ent_first"] = np.arange(G), 1, np.arange(G)
    pe = np.zeros(G, PROP_ENT_DT)
    pe["data_len"] = rng.integers(20, 120, G)
    pe["data_off"] = np.cumsum(pe["data_len"]) - pe["data_len"]
    pool = rng.integers(0, 256, int(pe["data_len"].sum()), dtype=np.uint8)
    hm = np.zeros(n_host, WIRE_MSG_DT)  # what a node queued itself this turn: payload-free responses
    hm["group"], hm["type"], hm["term"] = rng.integers(0, G, n_host), S.MSG_APP_RESP, 3
    hm["from"], hm["to"], hm["index"] = ME, rng.integers(1, N, n_host), rng.integers(1, 100000, n_host)
    he = np.zeros(0, WIRE_ENT_DT)
    args = [pinned_copy(props), pinned_copy(pe), pinned_copy(hm), he, pinned_copy(pool)]
    engines = {s: led_engine(G, N, s, True)[0] for s in SETTINGS}
    out, off = pinned_empty(len(pool) + 100 * (n_host + G * (N - 1)), np.uint8), pinned_empty(n_host + G * (N - 1) + 1, np.uint64)
    meds, last = {s: [] for s in SETTINGS}, {}
    for turn in range(TURNS + 1):  # turn 0 warms the handles up and is dropped
        for s in SETTINGS if turn % 2 == 0 else SETTINGS[::-1]:
            e, ts = engines[s], []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                _, _, c = e.propose_frames(*args, out, off)
                ts.append((time.perf_counter() - t0) * 1e6)
            last[s] = {"frames_with_bytes": int(c.n_msgs), "bytes": int(c.bytes)}
            if turn:
                meds[s].append(float(np.median(ts)))
    for e in engines.values():
        e.close()
    return summary(meds, last)


def respond_leg():
    G, N, n_groups = 1 << 20, 5, 32768
    rng = np.random.default_rng(6)
    groups = np.sort(rng.choice(G, n_groups, replace=False)).astype(np.uint64)
    n = 2 * n_groups
    engines, last0 = {}, None
    for s in SETTINGS:
        engines[s], last0 = led_engine(G, N, s, False)
    at_tail = pinned_copy(np.full((G + 63) // 64, ~np.uint64(0), np.uint64))
    order = rng.permutation(n)
    msgs, ents = pinned_empty(n, WIRE_MSG_DT), pinned_empty(16, WIRE_ENT_DT)
    out, roff, poff = pinned_empty(engines["none"].respond_cap(n), np.uint8), pinned_empty(n * (N - 1) + 1, np.uint64), pinned_empty(N + 1, np.uint64)
    meds, last = {s: [] for s in SETTINGS}, {}
    done = {s: 0 for s in SETTINGS}  # entries appended so far
    streams = {}

    def frames(k):
        """two acks (slots 1 and 2) of the tail after k + 1 appends, for every chosen group, shuffled"""
        if k not in streams:
            m = np.zeros(n, WIRE_MSG_DT)
            m["group"] = np.tile(groups, 2)
            m["from"] = np.repeat([1, 2], n_groups)
            m["type"], m["term"], m["to"] = S.MSG_APP_RESP, 3, ME
            m["index"] = np.tile(last0[groups.astype(np.int64)] + np.uint64(k + 1), 2)
            st, fo = engines["none"].wire_encode(m[order])
            streams[k] = (pinned_copy(np.ascontiguousarray(st)), pinned_copy(np.ascontiguousarray(fo, np.uint64)))
        return streams[k]

    for turn in range(TURNS + 1):
        for s in SETTINGS if turn % 2 == 0 else SETTINGS[::-1]:
            e, ts = engines[s], []
            for _ in range(CALLS):
                k = done[s]
                st, fo = frames(k)
                e.apply_log_deltas(groups, last0[groups.astype(np.int64)] + np.uint64(k + 1), 3)  # untimed: the leader appended
                t0 = time.perf_counter()
                r = e.step_frames_respond(st, fo, msgs, ents, at_tail, out, roff, poff, copy=False)
                ts.append((time.perf_counter() - t0) * 1e6)
                done[s] = k + 1
            last[s] = {"frames": int(r[7].n_msgs), "bytes": int(r[7].bytes), "answered": int(((r[2]["flags"] & 0x10) != 0).sum())}
            if turn:
                meds[s].append(float(np.median(ts)))
    for e in engines.values():
        e.close()
    return summary(meds, last)


def main():
    rec = {"what": "wall us per call (one submission, one wait); three handles of one shape in one process, the settings alternated %d times, %d "
                   "calls a turn after a warm-up turn; median and range of the turns' medians" % (TURNS, CALLS),
           "expectation": "full masks: the same frames, + a 2-byte read per proposal or broadcast (proposals: + an 8-byte memset and a one-thread "
                          "kernel), a few us; random masks: fewer bytes over the link, faster",
           "raftq_propose_frames 32768x3, 1 statement per group behind 65536 queued messages": propose_leg(),
           "raftq_step_frames_respond 1Mx5, 65536 frames (two acks for each of 32768 groups)": respond_leg()}
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
