#!/usr/bin/env python3
"""becomeLeader's broadcast on the device (raftq_respond_set_lead) against what it replaces, at a failover's shape: 65,536 groups
x 5 peers, every group a candidate that lacks one grant, 65,536 MsgVoteResp frames a call -> 65,536 wins -> 262,144 MsgApps that
carry the empty entry.

  A  the switch on: ONE raftq_step_frames_respond (decode + Step + the broadcasts laid out and marshalled on the device; one wait)
  B  the switch off: raftq_step_frames_respond (the wins stay the caller's: no frame), the MsgApp records and entry headers built on
     the host from the results (numpy field stores into page-locked memory -- slower than a C++ loop, so the build is reported on
     its own), raftq_wire_encode of them (page-locked: the streaming form)

Both read 32-byte results.  The state is reloaded before every call (not timed), so every call does the same work.  A and B are
ALTERNATED: TURNS turns of CALLS calls each after a warm-up turn; per path the median and the range of the turns' medians, wall us.
On the first timed turn the two paths' bytes are compared.
usage: tools/profile_respond_lead.py [out.json]      (run on the GPU box)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import step as S  # noqa: E402
from raftsql_amd import wire as W  # noqa: E402
from raftsql_amd.engine import pinned_copy, pinned_empty  # noqa: E402
from raftsql_amd.wire import WireEngine  # noqa: E402

G, N, ME = int(os.environ.get("G", "65536")), 5, 0
CALLS, TURNS = int(os.environ.get("CALLS", "6")), int(os.environ.get("TURNS", "5"))
TERM = 7


def make_state(rng):
    last = rng.integers(50, 100000, G).astype(np.uint64)
    last_term = rng.integers(1, TERM - 1, G).astype(np.uint64)
    return last, last_term


def load(e, last, last_term):
    """every group a candidate of TERM with its own vote and slot 1's: one grant short of the quorum of three"""
    match = np.zeros((N, G), np.uint64)
    match[ME] = last
    e.load_match(match, last - np.uint64(2))
    votes = np.zeros((N, G), np.uint8)
    votes[ME], votes[1] = 1, 1
    e.load_votes(votes)
    e.load_terms(np.zeros(G, np.uint64), np.zeros(G, np.uint64))
    e.load_roles(np.full(G, 1, np.uint8))
    e.load_node(np.full(G, TERM, np.uint64), np.full(G, ME + 1, np.uint32), np.zeros(G, np.uint32), last, last_term)


def grants(e, rng):
    m = np.zeros(G, W.WIRE_MSG_DT)
    m["group"] = rng.permutation(G)
    m["from"], m["type"], m["term"], m["to"] = 2, S.MSG_VOTE_RESP, TERM, ME
    s, off = e.wire_encode(m)
    return pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64)), m


def summary(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def main():
    rng = np.random.default_rng(17)
    last, last_term = make_state(rng)
    n, n_out = G, G * (N - 1)
    with WireEngine(G, N, ME, device=0) as a, WireEngine(G, N, ME, device=0) as b:
        a.set_respond_lead(True)
        ps, po, m = grants(a, rng)
        groups = m["group"].astype(np.int64)
        for e in (a, b):
            e.set_compact(2)
        msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(16, W.WIRE_ENT_DT)
        out = pinned_empty(a.respond_cap(n), np.uint8)
        ro, pof = pinned_empty(n_out + 1, np.uint64), pinned_empty(N + 1, np.uint64)
        enc_msgs, enc_ents = pinned_empty(n_out, W.WIRE_MSG_DT), pinned_empty(n, W.WIRE_ENT_DT)
        enc_out, enc_off = pinned_empty(a.respond_cap(n), np.uint8), pinned_empty(n_out + 1, np.uint64)
        t = {k: [] for k in ("A", "B", "B_call", "B_build", "B_encode")}
        shape = {}
        bytes_a = None

        def path_a():
            nonlocal bytes_a
            load(a, last, last_term)
            t0 = time.perf_counter()
            _, _, go, rs, _, _, _, rc = a.step_frames_respond(ps, po, msgs, ents, None, out, ro, pof, copy=False)
            dt = (time.perf_counter() - t0) * 1e6
            shape["A"] = {"frames_out": int(rc.n_msgs), "bytes_out": int(rc.bytes), "answered": int(((go["flags"] & W.OUTF_ANSWERED) != 0).sum())}
            if bytes_a is None:
                bytes_a = bytes(rs)
            return {"A": dt}

        def path_b():
            load(b, last, last_term)
            t0 = time.perf_counter()
            _, _, go, _, _, _, _, rc = b.step_frames_respond(ps, po, msgs, ents, None, out, ro, pof, copy=False)
            t1 = time.perf_counter()
            assert rc.n_msgs == 0
            # becomeLeader's bcastAppend as the caller builds it today: per peer, in result order (the old lastTerm is the caller's own log's)
            hit = np.nonzero(go["type"] == S.OUT_BECAME_LEADER)[0]
            k = len(hit)
            en = enc_ents[:k]
            en[:] = np.zeros(1, W.WIRE_ENT_DT)
            en["term"], en["index"] = go["term"][hit], go["index"][hit]
            g = groups[hit]
            for j, p in enumerate(p for p in range(N) if p != ME):
                r = enc_msgs[j * k:(j + 1) * k]
                r[:] = np.zeros(1, W.WIRE_MSG_DT)
                r["group"], r["term"], r["index"], r["log_term"] = g, go["term"][hit], go["index"][hit] - np.uint64(1), last_term[g]
                r["commit"], r["from"], r["type"], r["to"] = go["commit"][hit], ME, 3, p
                r["ent_first"], r["n_ents"] = np.arange(k), 1
            t2 = time.perf_counter()
            s, _ = b.wire_encode(enc_msgs[: k * (N - 1)], en, out=enc_out, off=enc_off[: k * (N - 1) + 1])
            t3 = time.perf_counter()
            shape["B"] = {"frames_out": k * (N - 1), "bytes_out": len(s), "host_record_bytes": k * (N - 1) * 64 + k * 32}
            if bytes_a is not None and "same_bytes" not in shape:
                shape["same_bytes"] = bytes(s) == bytes_a
                assert shape["same_bytes"], "the two paths disagree on what goes out"
            return {"B": (t3 - t0) * 1e6, "B_call": (t1 - t0) * 1e6, "B_build": (t2 - t1) * 1e6, "B_encode": (t3 - t2) * 1e6}

        for turn in range(TURNS + 1):  # turn 0 warms both handles up and is dropped
            for path in (path_a, path_b) if turn % 2 == 0 else (path_b, path_a):
                per = {}
                for _ in range(CALLS):
                    for k, v in path().items():
                        per.setdefault(k, []).append(v)
                if turn:
                    for k, v in per.items():
                        t[k].append(float(np.median(v)))
    rec = {"what": "wall us; 65,536 groups x 5 win an election in one batch (65,536 MsgVoteResp in, 262,144 MsgApps with the empty entry out); "
                   "A = one raftq_step_frames_respond with raftq_respond_set_lead on, B = the switch off + the MsgApps built on the host (numpy) + "
                   "raftq_wire_encode; alternated %d times, %d calls a turn after a warm-up turn; median and range of the turns' medians" % (TURNS, CALLS),
           "G": G, "N": N, "frames_in": n, "same_bytes": shape.pop("same_bytes"), "last_call": shape, **{k: summary(v) for k, v in t.items()}}
    rec["A_over_B"] = round(rec["A"]["median_us"] / rec["B"]["median_us"], 3)
    rec["A_over_B_without_the_numpy_build"] = round(rec["A"]["median_us"] / (rec["B_call"]["median_us"] + rec["B_encode"]["median_us"]), 3)
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
