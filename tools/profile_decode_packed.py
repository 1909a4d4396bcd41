#!/usr/bin/env python3
"""The streaming decoder's narrow output forms against the plain calls, 65,536 frames a call, in ONE process:

  decode   raftq_wire_decode            | raftq_wire_decode_packed, RAFTQ_WIRE_FORM_40 | ..., RAFTQ_WIRE_FORM_HEAD
  step     raftq_step_frames            | raftq_step_frames_packed, RAFTQ_WIRE_FORM_40 | ..., RAFTQ_WIRE_FORM_HEAD

on two mixes, every frame addressed to this node's slot:
  codec    the bench's codec mix: 15 % MsgApp with 1-3 entries, the rest acknowledgements, heartbeats, votes and their answers
  acks     MsgAppResp only, two per group: the one-node leg's inbound traffic

The three forms of a call ALTERNATE inside one loop (plain, 40, head, plain, ...), so they see the same box in the same state;
the plain call is untouched code and its figure from the same loop is the baseline.  Before anything is timed the outputs
are compared: the narrow records expanded (raftsql_amd.wire.expand_packed) are the plain call's records, the entry headers
and the Step results are the same bytes.  Step's state is reloaded before every call (not timed).  Median / p10 / p90 of
REPS calls after WARM warm-up calls; one JSON line per (mix, call, form) to stdout and appended to OUT (default
profiles/r07/decode_packed_ab.jsonl)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import wire as W  # noqa: E402
from raftsql_amd.engine import pinned_copy, pinned_empty  # noqa: E402
from raftsql_amd.wire import WireEngine  # noqa: E402

G, N, ME = int(os.environ.get("G", "32768")), 3, 0
FRAMES = int(os.environ.get("FRAMES", "65536"))
REPS, WARM = int(os.environ.get("REPS", "30")), int(os.environ.get("WARM", "5"))
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07", "decode_packed_ab.jsonl"))
LAST, TERM = 20, 3
RESPONSE_KINDS = (1 << 4) | (1 << 6) | (1 << 9)
FORMS = (("plain", 0), ("form40", W.FORM_40), ("head", W.FORM_HEAD))


def load(e):
    """every group led here, every follower one entry behind the tail: an acknowledgement of LAST commits"""
    match = np.full((N, G), LAST - 1, np.uint64)
    match[ME] = LAST
    e.load_match(match, np.full(G, LAST - 1, np.uint64))
    e.load_terms(np.full(G, TERM, np.uint64), np.ones(G, np.uint64))
    e.load_roles(np.full(G, 2, np.uint8))
    e.load_node(np.full(G, TERM, np.uint64), np.full(G, ME + 1, np.uint32), np.full(G, ME + 1, np.uint32), np.full(G, LAST, np.uint64),
                np.full(G, TERM, np.uint64))


def mix(e, rng, kind):
    """-> (stream, frame_off) page-locked, and the number of entry headers in it"""
    n = FRAMES
    m = np.zeros(n, W.WIRE_MSG_DT)
    m["group"] = np.arange(n) % G
    m["from"] = (ME + 1 + np.arange(n) // G % (N - 1)) % N
    m["to"], m["term"], m["index"] = ME, TERM, LAST
    if kind == "acks":
        m["type"] = 4
    else:
        m["type"] = rng.choice([3, 4, 9, 8, 6, 5], n, p=[0.15, 0.47, 0.13, 0.10, 0.08, 0.07])
        m["log_term"] = np.where(np.isin(m["type"], [3, 5]), TERM, 0)
        m["commit"] = np.where(np.isin(m["type"], [3, 8]), LAST - 1, 0)
    m = m[rng.permutation(n)]
    k = np.where(m["type"] == 3, rng.integers(1, 4, n), 0)
    m["n_ents"] = k
    m["ent_first"] = np.where(k > 0, np.concatenate([[0], np.cumsum(k)[:-1]]), 0)
    ne = int(k.sum())
    ents = np.zeros(ne, W.WIRE_ENT_DT)
    owner = np.repeat(np.arange(n), k)
    ents["term"] = TERM
    ents["index"] = LAST + 1 + (np.arange(ne) - m["ent_first"][owner])
    ents["data_len"] = rng.integers(16, 64, ne)
    ents["data_off"] = np.concatenate([[0], np.cumsum(ents["data_len"])[:-1]]) if ne else 0
    pool = rng.integers(0, 256, int(ents["data_len"].sum()) + 1, dtype=np.uint8)
    s, off = e.wire_encode(m, ents, pool)
    return pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64)), ne


def stats(ts):
    a = np.array(ts) * 1e6
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)), "n": len(a)}


def delivered(msgs, narrow, form):
    """what an exact expansion gives back: in the head form a narrow frame's five scalar fields are the caller's declared loss"""
    out = msgs.copy()
    if form == W.FORM_HEAD:
        lost = (narrow["flags"] & W.F_WIDE) == 0
        for f in ("term", "index", "log_term", "commit", "reject_hint"):
            out[f][lost] = 0
    return out


def main():
    rng = np.random.default_rng(11)
    rows = []
    with WireEngine(G, N, ME, device=0) as e:
        e.set_compact(2)  # 32-byte results: the node's form
        for kind in ("codec", "acks"):
            ps, po, ne = mix(e, rng, kind)
            n = len(po) - 1
            msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(ne + 16, W.WIRE_ENT_DT)
            narrow = {W.FORM_40: pinned_empty(n, W.WIRE_MSG40_DT), W.FORM_HEAD: pinned_empty(n, W.WIRE_HEAD_DT)}
            wide, ents_p = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(ne + 16, W.WIRE_ENT_DT)

            def decode(form):
                if form == 0:
                    return e.wire_decode(ps, po, msgs=msgs, ents=ents)
                return e.wire_decode_packed(ps, po, form, ME, narrow[form], wide, ents_p, head_types=RESPONSE_KINDS)

            def step(form):
                if form == 0:
                    return e.step_frames(ps, po, msgs, ents, copy=False)
                return e.step_frames_packed(ps, po, form, narrow[form], wide, ents_p, head_types=RESPONSE_KINDS, copy=False)

            # the forms agree before anything is timed
            n_wide = {"decode": {}, "step": {}}
            pm, pe, _ = decode(0)
            pm, pe = pm.copy(), pe.copy()
            for _, form in FORMS[1:]:
                nar, wd, ge, _, nw, _ = decode(form)
                n_wide["decode"][form] = nw
                assert ge.tobytes() == pe.tobytes(), "entry headers differ"
                assert W.expand_packed(nar, wd, ME, form).tobytes() == delivered(pm, nar, form).tobytes(), "the expansion is not the plain call's records"
            load(e)
            sm, se, so, _ = step(0)
            sm, se, so = sm.copy(), se.copy(), so.copy()
            for _, form in FORMS[1:]:
                load(e)
                nar, wd, ge, go, _, nw = step(form)
                n_wide["step"][form] = nw
                assert ge.tobytes() == se.tobytes() and go.tobytes() == so.tobytes(), "Step's results differ"
                assert W.expand_packed(nar, wd, ME, form).tobytes() == delivered(sm, nar, form).tobytes(), "the expansion is not the plain call's records"
            for call, fn, reload in (("decode", decode, False), ("step", step, True)):
                ts = {name: [] for name, _ in FORMS}
                for it in range(WARM + REPS):
                    for name, form in FORMS:
                        if reload:
                            load(e)
                        t0 = time.perf_counter()
                        fn(form)
                        t1 = time.perf_counter()
                        if it >= WARM:
                            ts[name].append(t1 - t0)
                for name, form in FORMS:
                    nw = n_wide[call].get(form, n)
                    rows.append(dict(mix=kind, call=call, form=name, frames=n, stream_bytes=int(len(ps)), entry_headers=ne, n_wide=int(nw),
                                     record_bytes_out=int(n * 64 if form == 0 else n * form + nw * 64), **stats(ts[name])))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
