#!/usr/bin/env python3
"""A follower's proposals as MsgProp frames on the device (raftq_propose_set_forward) against what they replace: 32,768 groups, one
64-byte statement proposed in each, at N = 3 and 5 -- every group followed (every record forwarded, the leaders spread over the other
slots), and one third led / two thirds followed (the reference's three-node share: two thirds of all writes start on a follower).

  A   the switch on: ONE raftq_propose_frames -- 16-byte records, 16-byte entry records and the payload in; the MsgProp / MsgApp
      records and the entry headers built in HBM, the marshal behind them; the outcomes in the same submission; one wait
  B   the same frames built as host records -- a MsgProp record per forwarded group, N - 1 MsgApp records per led one, an entry
      header per statement, in A's order without the zero-length slots -- and passed to raftq_wire_encode.  The build (numpy field
      stores into page-locked memory: slower than a C++ loop) is timed separately and NOT counted in B

The state is reloaded before every call (not timed), so every call does the same work.  The paths are ALTERNATED: TURNS turns of
CALLS calls each after a warm-up turn; per path the median and the range of the turns' medians, wall us.  On the first timed turn
A's stream is compared with B's, byte for byte.  link_bytes: what each path moves over the link, summed from the sizes of the arrays
it reads and writes there.
usage: tools/profile_propose_forward.py [out.json]      (run on the GPU box)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import wire as W  # noqa: E402
from raftsql_amd.engine import pinned_copy, pinned_empty  # noqa: E402
from raftsql_amd.wire import WireEngine  # noqa: E402

G = int(os.environ.get("G", "32768"))
CALLS, TURNS = int(os.environ.get("CALLS", "6")), int(os.environ.get("TURNS", "5"))
TERM, PAYLOAD = 7, 64


def load(e, N, me, last, role, lead):
    match = np.tile(last - np.uint64(1), (N, 1))
    match[me] = last
    e.load_match(match, last - np.uint64(1))
    e.load_terms(np.full(G, TERM, np.uint64), np.ones(G, np.uint64))
    e.load_roles(role)
    e.load_node(np.full(G, TERM, np.uint64), lead, lead, last, np.full(G, TERM - 2, np.uint64))


def summary(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def measure(N, led_share, seed):
    rng = np.random.default_rng(seed)
    me = 1
    others = np.array([p for p in range(N) if p != me])
    last = rng.integers(50, 100000, G).astype(np.uint64)
    led = rng.random(G) < led_share
    role = np.where(led, 2, 0).astype(np.uint8)
    lead = np.where(led, me + 1, others[rng.integers(0, N - 1, G)] + 1).astype(np.uint32)
    props = np.zeros(G, W.PROP_DT)
    props["group"], props["ent_first"], props["n_ents"] = rng.permutation(G), np.arange(G), 1
    pe = np.zeros(G, W.PROP_ENT_DT)
    pe["data_len"], pe["data_off"] = PAYLOAD, np.arange(G) * PAYLOAD
    pool = pinned_copy(rng.integers(0, 256, G * PAYLOAD, dtype=np.uint8))
    p_props, p_pe = pinned_copy(props), pinned_copy(pe)
    none_m, none_e = pinned_empty(0, W.WIRE_MSG_DT), pinned_empty(0, W.WIRE_ENT_DT)
    g = props["group"].astype(np.int64)
    n_slots = G * (N - 1)
    n_frames = int(led[g].sum()) * (N - 1) + int((~led[g]).sum())
    cap = n_slots * 128 + G * PAYLOAD * (N - 1)
    out_a, off_a = pinned_empty(cap, np.uint8), pinned_empty(n_slots + 1, np.uint64)
    out_b, off_b = pinned_empty(cap, np.uint8), pinned_empty(n_frames + 1, np.uint64)
    enc_m, enc_e = pinned_empty(n_frames, W.WIRE_MSG_DT), pinned_empty(G, W.WIRE_ENT_DT)
    t = {key: [] for key in ("A", "B", "B_build")}
    keep, shape, link = {}, {}, {}
    with WireEngine(G, N, me, device=0) as a, WireEngine(G, N, me, device=0) as b:
        a.set_propose_forward(True)

        def path_a():
            load(a, N, me, last, role, lead)
            t0 = time.perf_counter()
            s, off, c, what = a.propose_frames(p_props, p_pe, none_m, none_e, pool, out_a, off_a)
            dt = (time.perf_counter() - t0) * 1e6
            assert c.n_msgs == n_frames
            shape["A"] = {"frames": int(c.n_msgs), "bytes_out": int(c.bytes), "forwarded": int((what == W.PROP_FORWARDED).sum()), "appended": int((what == W.PROP_APPENDED).sum())}
            link["A"] = {"in": p_props.nbytes + p_pe.nbytes + pool.nbytes, "out": int(c.bytes) + off_a.nbytes + len(what)}
            keep.setdefault("A", bytes(s))
            return {"A": dt}

        def path_b():
            t0 = time.perf_counter()
            # the entry headers: appendEntry's stamps for a led group, the client's zeros for a followed one
            enc_e[:] = np.zeros(1, W.WIRE_ENT_DT)
            enc_e["data_len"], enc_e["data_off"] = PAYLOAD, pe["data_off"]
            enc_e["term"], enc_e["index"] = np.where(led[g], TERM, 0), np.where(led[g], last[g] + np.uint64(1), 0)
            at = 0
            for p in others:  # run by run, as the call lays them out; a followed group's record only in its leader's run
                here = np.flatnonzero(led[g] | (lead[g] == p + 1))
                r = enc_m[at:at + len(here)]
                r[:] = np.zeros(1, W.WIRE_MSG_DT)
                gl = led[g[here]]
                r["group"], r["from"], r["to"], r["ent_first"], r["n_ents"] = g[here], me, p, here, 1
                r["type"] = np.where(gl, 3, 2)
                r["term"], r["log_term"] = np.where(gl, TERM, 0), np.where(gl, TERM - 2, 0)
                r["index"], r["commit"] = np.where(gl, last[g[here]], 0), np.where(gl, last[g[here]] - np.uint64(1), 0)
                at += len(here)
            assert at == n_frames
            t1 = time.perf_counter()
            s, off = b.wire_encode(enc_m, enc_e, pool, out=out_b, off=off_b)
            t2 = time.perf_counter()
            shape["B"] = {"frames": n_frames, "bytes_out": len(s)}
            link["B"] = {"in": enc_m.nbytes + enc_e.nbytes + pool.nbytes, "out": len(s) + off_b.nbytes}
            keep.setdefault("B", bytes(s))
            return {"B": (t2 - t1) * 1e6, "B_build": (t1 - t0) * 1e6}

        paths = [path_a, path_b]
        for turn in range(TURNS + 1):  # turn 0 warms both handles up and is dropped
            for path in paths if turn % 2 == 0 else paths[::-1]:
                per = {}
                for _ in range(CALLS):
                    for key, v in path().items():
                        per.setdefault(key, []).append(v)
                if turn:
                    for key, v in per.items():
                        t[key].append(float(np.median(v)))
        same = keep["A"] == keep["B"]
        assert same, "the paths disagree on the frames"
    rec = {"N": N, "led_share": led_share, "groups": G, "same_bytes": same, "last_call": shape, "link_bytes": link, **{key: summary(v) for key, v in t.items()}}
    rec["A_over_B"] = round(rec["A"]["median_us"] / rec["B"]["median_us"], 3)
    return rec


def main():
    runs = [measure(N, share, 23 + N) for N in (3, 5) for share in (0.0, 1 / 3)]
    rec = {"what": "wall us; %d groups, one %d-byte statement proposed in each; led_share of the groups led, the others followed (leaders spread over the "
                   "other slots); A = one raftq_propose_frames with raftq_propose_set_forward on, B = raftq_wire_encode of the same frames built "
                   "as host records (B_build, numpy, not counted in B); alternated %d times, %d calls a turn after a warm-up turn; median and range "
                   "of the turns' medians" % (G, PAYLOAD, TURNS, CALLS), "runs": runs}
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
