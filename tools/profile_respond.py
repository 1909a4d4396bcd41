#!/usr/bin/env python3
"""raftq_step_frames_respond against what it replaces, at the one-node leg's shape: 32,768 groups x 3 peers led here, every
follower at the tail, 65,536 MsgAppResp frames a call (two acks per group: the first commits -> one commit broadcast of two
MsgApps, the second does not) -> 65,536 device-built frames.

  respond   raftq_step_frames_respond (decode + Step + the responses laid out and marshalled on the device; one wait)
  host      raftq_step_frames, the MsgApp records built on the host from the results (numpy field stores into page-locked
            memory -- slower than the node's C++ apply loop, so the build is reported on its own), raftq_wire_encode of them
            (page-locked: the streaming form)

Both read 32-byte results (the node's form).  The state is reloaded before every call (not timed), so every call does the
same work.  Median / p10 / p90 of REPS calls after WARM warm-up calls, one JSON line per form to stdout and to OUT
(default profiles/r07/respond_ab.jsonl).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/profile_respond.py`
for the kernels' share."""
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

G, N, ME = int(os.environ.get("G", "32768")), 3, 0
REPS, WARM = int(os.environ.get("REPS", "30")), int(os.environ.get("WARM", "5"))
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07", "respond_ab.jsonl"))
LAST, TERM = 20, 3


def load(e):
    match = np.full((N, G), LAST - 1, np.uint64)
    match[ME] = LAST
    e.load_match(match, np.full(G, LAST - 1, np.uint64))
    e.load_terms(np.full(G, TERM, np.uint64), np.ones(G, np.uint64))
    e.load_roles(np.full(G, 2, np.uint8))
    e.load_node(np.full(G, TERM, np.uint64), np.full(G, ME + 1, np.uint32), np.full(G, ME + 1, np.uint32), np.full(G, LAST, np.uint64),
                np.full(G, TERM, np.uint64))


def frames(e, rng):
    fol = np.array([p for p in range(N) if p != ME])
    m = np.zeros(G * len(fol), W.WIRE_MSG_DT)
    m["group"] = np.repeat(np.arange(G), len(fol))
    m["from"] = np.tile(fol, G)
    m["type"], m["term"], m["index"], m["to"] = 4, TERM, LAST, ME
    m = m[rng.permutation(len(m))]
    s, off = e.wire_encode(m)
    return pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64)), m


def stats(ts):
    a = np.array(ts) * 1e6
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)), "n": len(a)}


def main():
    rng = np.random.default_rng(7)
    rows = []
    with WireEngine(G, N, ME, device=0) as e:
        ps, po, m = frames(e, rng)
        n = len(po) - 1
        e.set_compact(2)
        msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(16, W.WIRE_ENT_DT)
        out, ro, pof = pinned_empty(e.respond_cap(n), np.uint8), pinned_empty(n * (N - 1) + 1, np.uint64), pinned_empty(N + 1, np.uint64)
        at = pinned_copy(np.full((G + 63) // 64, ~np.uint64(0), np.uint64))
        enc_msgs = pinned_empty(n * (N - 1), W.WIRE_MSG_DT)
        enc_out, enc_off = pinned_empty(e.respond_cap(n), np.uint8), pinned_empty(n * (N - 1) + 1, np.uint64)
        t_resp, t_host, t_step, t_build, t_enc = [], [], [], [], []
        nbytes = {}
        for it in range(WARM + REPS):
            load(e)
            t0 = time.perf_counter()
            _, _, go, rs, _, _, _, rc = e.step_frames_respond(ps, po, msgs, ents, at, out, ro, pof, copy=False)
            t1 = time.perf_counter()
            if it >= WARM:
                t_resp.append(t1 - t0)
            nbytes["respond"] = (int(rc.n_msgs), int(rc.bytes), int(((go["flags"] & W.OUTF_ANSWERED) != 0).sum()))
            load(e)
            t0 = time.perf_counter()
            _, _, go, _ = e.step_frames(ps, po, msgs, ents, copy=False)
            t1 = time.perf_counter()
            # bcastAppend for every committing ack, as apply_result would queue it (per peer, in result order)
            hit = np.nonzero((go["type"] == S.OUT_PROGRESS) & ((go["flags"] & S.OUTF_COMMITTED) != 0))[0]
            k = len(hit)
            for j, p in enumerate(p for p in range(N) if p != ME):
                r = enc_msgs[j * k:(j + 1) * k]
                r[:] = np.zeros(1, W.WIRE_MSG_DT)
                r["group"], r["term"], r["index"], r["log_term"] = m["group"][hit], go["term"][hit], LAST, TERM
                r["commit"], r["from"], r["type"], r["to"] = go["commit"][hit], ME, 3, p
            t2 = time.perf_counter()
            s, _ = e.wire_encode(enc_msgs[: k * (N - 1)], out=enc_out, off=enc_off[: k * (N - 1) + 1])
            t3 = time.perf_counter()
            if it >= WARM:
                t_host.append(t3 - t0)
                t_step.append(t1 - t0)
                t_build.append(t2 - t1)
                t_enc.append(t3 - t2)
            nbytes["host"] = (k * (N - 1), len(s))
            if it == WARM:  # the two forms agree on what goes out (peer-major, result order)
                assert nbytes["respond"][:2] == nbytes["host"] and bytes(rs) == bytes(s), "the forms disagree"
    base = {"G": G, "N": N, "frames_in": n}
    rows.append(dict(base, form="respond", frames_out=nbytes["respond"][0], bytes_out=nbytes["respond"][1], answered=nbytes["respond"][2],
                     result_bytes_in=n * 32, **stats(t_resp)))
    rows.append(dict(base, form="host", frames_out=nbytes["host"][0], bytes_out=nbytes["host"][1], result_bytes_in=n * 32,
                     host_records_bytes=nbytes["host"][0] * 64, step_frames=stats(t_step), build=stats(t_build), encode=stats(t_enc),
                     **stats(t_host)))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
