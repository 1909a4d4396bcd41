#!/usr/bin/env python3
"""A forwarded proposal's MsgApps on the device (raftq_respond_set_props) against what it replaces, at a steady-state leader's shape:
65,536 led groups with every follower at the tail, 65,536 frames a call -- a share of them MsgProp with one 64-byte entry from a
follower, the rest acknowledgements that commit -- at N = 3 and 5, with 25 % and 66 % MsgProp.

  A      the switch on: ONE raftq_step_frames_respond (decode + Step + every broadcast laid out and marshalled on the device, the
         payloads gathered from the decoder's copy of the stream in HBM; one wait)
  A_feed the same with RAFTQ_RESPOND_PROPS_POOL=feed: the encoder's readers pull the stream from the caller's array a second time
  B      the parent's path: the switch off (the proposals stay the caller's, the acks are answered), the MsgApp records and entry
         headers built on the host from the results and the decoded headers (numpy field stores into page-locked memory: slower
         than a C++ loop, so the build is reported on its own), raftq_wire_encode of them with the inbound stream as the pool

All read 32-byte results.  The state is reloaded before every call (not timed), so every call does the same work.  The paths are
ALTERNATED: TURNS turns of CALLS calls each after a warm-up turn; per path the median and the range of the turns' medians, wall us.
On the first timed turn A's proposal frames are compared with B's, byte for byte, slice by slice.  link_bytes: what each path moves
over the link, summed from the sizes of the arrays it reads and writes there.
usage: tools/profile_respond_props.py [out.json]      (run on the GPU box)"""
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

G, ME = int(os.environ.get("G", "65536")), 0
CALLS, TURNS = int(os.environ.get("CALLS", "6")), int(os.environ.get("TURNS", "5"))
TERM, PAYLOAD = 7, 64
POOL_ENV = "RAFTQ_RESPOND_PROPS_POOL"


def load(e, N, last):
    """every group led by ME at TERM and committed up to the entry before the tail; slot N - 1, the sender of every ack, is one
    entry behind in Match (its ack of the tail commits it), every follower is at the tail in Next"""
    match = np.tile(last, (N, 1))
    match[N - 1] = last - np.uint64(1)
    e.load_match(match, last - np.uint64(1))
    e.load_votes(np.zeros((N, G), np.uint8))
    e.load_terms(np.full(G, TERM, np.uint64), np.ones(G, np.uint64))
    e.load_roles(np.full(G, 2, np.uint8))
    e.load_node(np.full(G, TERM, np.uint64), np.full(G, ME + 1, np.uint32), np.full(G, ME + 1, np.uint32), last, np.full(G, TERM - 2, np.uint64))


def traffic(e, rng, N, share, last):
    """one frame per group, in a random order: a MsgProp with one PAYLOAD-byte entry (share of them) or the ack of the tail"""
    m = np.zeros(G, W.WIRE_MSG_DT)
    m["group"] = rng.permutation(G)
    prop = rng.random(G) < share
    m["from"], m["to"] = N - 1, ME
    m["type"] = np.where(prop, S.MSG_PROP, S.MSG_APP_RESP)
    m["term"] = np.where(prop, 0, TERM)
    m["index"] = np.where(prop, 0, last[m["group"].astype(np.int64)])
    m["n_ents"] = prop
    m["ent_first"] = np.cumsum(prop) - prop
    k = int(prop.sum())
    en = np.zeros(k, W.WIRE_ENT_DT)
    en["data_len"], en["data_off"] = PAYLOAD, np.arange(k) * PAYLOAD
    pool = rng.integers(0, 256, k * PAYLOAD + 1, dtype=np.uint8)
    s, off = e.wire_encode(m, en, pool)
    return pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64)), m, k


def summary(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def measure(N, share, seed):
    rng = np.random.default_rng(seed)
    last = rng.integers(50, 100000, G).astype(np.uint64)
    n, n_out = G, G * (N - 1)
    with WireEngine(G, N, ME, device=0) as a, WireEngine(G, N, ME, device=0) as b:
        for e in (a, b):
            e.set_compact(2)
            e.set_step_props(True)
        a.set_respond_props(True)
        ps, po, m, k = traffic(a, rng, N, share, last)
        groups = m["group"].astype(np.int64)
        ents_cap = k + 1
        msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(ents_cap, W.WIRE_ENT_DT)
        at_tail = pinned_copy(np.full((G + 63) // 64, 2**64 - 1, np.uint64))
        cap = a.respond_cap(n, len(ps), ents_cap)
        out = pinned_empty(cap, np.uint8)
        ro, pof = pinned_empty(n_out + 1, np.uint64), pinned_empty(N + 1, np.uint64)
        enc_msgs, enc_ents = pinned_empty(n_out, W.WIRE_MSG_DT), pinned_empty(ents_cap, W.WIRE_ENT_DT)
        enc_out, enc_off = pinned_empty(cap, np.uint8), pinned_empty(n_out + 1, np.uint64)
        t = {key: [] for key in ("A", "A_feed", "B", "B_call", "B_build", "B_encode")}
        shape, link, keep = {}, {}, {}
        fixed_in = len(ps) + po.nbytes + at_tail.nbytes
        fixed_out = n * msgs.itemsize + n * 32 + ro.nbytes + (N + 1) * 8  # records, 32-byte results, offsets, slices

        def call_a(name, feed):
            if feed:
                os.environ[POOL_ENV] = "feed"
            load(a, N, last)
            t0 = time.perf_counter()
            _, ge, go, rs, roff, _, c, rc = a.step_frames_respond(ps, po, msgs, ents, at_tail, out, ro, pof, copy=False)
            dt = (time.perf_counter() - t0) * 1e6
            os.environ.pop(POOL_ENV, None)
            shape[name] = {"frames_out": int(rc.n_msgs), "bytes_out": int(rc.bytes), "answered": int(((go["flags"] & W.OUTF_ANSWERED) != 0).sum())}
            # in: the stream, the boundaries, the bitmap, the decoder's headers read back by the layout (+ the stream again when fed);
            # out: the records, headers, results, offsets and the frames
            link[name] = {"in": fixed_in + int(c.n_ents) * 32 + (len(ps) if feed else 0), "out": fixed_out + int(c.n_ents) * 32 + int(rc.bytes)}
            if name not in keep:
                hit = np.nonzero(go["type"] == S.OUT_PROPOSED)[0]
                raw, roff = np.asarray(rs), np.asarray(roff)
                assert rc.n_msgs == n_out  # every result a broadcast: frame i of slice j is result i's
                keep[name] = [b"".join(bytes(raw[int(roff[j * n + i]):int(roff[j * n + i + 1])]) for i in hit) for j in range(N - 1)]
            return {name: dt}

        def path_b():
            load(b, N, last)
            t0 = time.perf_counter()
            _, ge, go, _, _, _, c, rc = b.step_frames_respond(ps, po, msgs, ents, at_tail, out, ro, pof, copy=False)
            t1 = time.perf_counter()
            # stepLeader's bcastAppend as the caller builds it today: per peer, in result order; the headers are the decoder's, stamped
            hit = np.nonzero(go["type"] == S.OUT_PROPOSED)[0]
            kk = len(hit)
            en = enc_ents[:kk]
            en[:] = ge[msgs["ent_first"][hit]]
            en["term"], en["index"] = go["term"][hit], go["index"][hit]
            g = groups[hit]
            for j, p in enumerate(p for p in range(N) if p != ME):
                r = enc_msgs[j * kk:(j + 1) * kk]
                r[:] = np.zeros(1, W.WIRE_MSG_DT)
                r["group"], r["term"], r["index"], r["log_term"] = g, go["term"][hit], go["index"][hit] - np.uint64(1), TERM - 2
                r["commit"], r["from"], r["type"], r["to"] = go["commit"][hit], ME, 3, p
                r["ent_first"], r["n_ents"] = np.arange(kk), 1
            t2 = time.perf_counter()
            s, soff = b.wire_encode(enc_msgs[: kk * (N - 1)], en, ps, out=enc_out, off=enc_off[: kk * (N - 1) + 1])
            t3 = time.perf_counter()
            shape["B"] = {"frames_out": int(rc.n_msgs) + kk * (N - 1), "bytes_out": int(rc.bytes) + len(s), "answered": int(((go["flags"] & W.OUTF_ANSWERED) != 0).sum())}
            link["B"] = {"in": fixed_in + kk * (N - 1) * 64 + kk * 32 + len(ps), "out": fixed_out + int(c.n_ents) * 32 + int(rc.bytes) + len(s) + (kk * (N - 1) + 1) * 8}
            if "B" not in keep:
                raw, soff = np.asarray(s), np.asarray(soff)
                keep["B"] = [bytes(raw[int(soff[j * kk]):int(soff[(j + 1) * kk])]) for j in range(N - 1)]
            return {"B": (t3 - t0) * 1e6, "B_call": (t1 - t0) * 1e6, "B_build": (t2 - t1) * 1e6, "B_encode": (t3 - t2) * 1e6}

        paths = [lambda: call_a("A", False), path_b, lambda: call_a("A_feed", True)]
        for turn in range(TURNS + 1):  # turn 0 warms both handles up and is dropped
            for path in paths if turn % 2 == 0 else paths[::-1]:
                per = {}
                for _ in range(CALLS):
                    for key, v in path().items():
                        per.setdefault(key, []).append(v)
                if turn:
                    for key, v in per.items():
                        t[key].append(float(np.median(v)))
        same = keep["A"] == keep["B"] == keep["A_feed"]
        assert same, "the paths disagree on the proposals' frames"
    rec = {"N": N, "share_of_msgprop": share, "frames_in": n, "stream_bytes_in": len(ps), "proposals": k, "same_bytes": same, "last_call": shape,
           "link_bytes": link, **{key: summary(v) for key, v in t.items()}}
    rec["A_over_B"] = round(rec["A"]["median_us"] / rec["B"]["median_us"], 3)
    rec["A_over_B_without_the_numpy_build"] = round(rec["A"]["median_us"] / (rec["B_call"]["median_us"] + rec["B_encode"]["median_us"]), 3)
    rec["A_over_A_feed"] = round(rec["A"]["median_us"] / rec["A_feed"]["median_us"], 3)
    return rec


def main():
    runs = [measure(N, share, 22 + N) for N in (3, 5) for share in (0.25, 0.66)]
    rec = {"what": "wall us; %d led groups, %d frames a call: MsgProp with one %d-byte entry (the share) or a committing ack; A = one "
                   "raftq_step_frames_respond with raftq_respond_set_props on (pool = the decoder's copy of the stream), A_feed = the same with the "
                   "pool fed from the caller's stream, B = the switch off + the MsgApps built on the host (numpy) + raftq_wire_encode with the "
                   "stream as the pool; alternated %d times, %d calls a turn after a warm-up turn; median and range of the turns' medians"
                   % (G, G, PAYLOAD, TURNS, CALLS), "runs": runs}
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
