#!/usr/bin/env python3
"""A node's election round, two forms in one process, alternated call by call on the same handle:

  host    today's form: raftq_tick_collect_lists, one 64-byte local MsgHup record per id built on the host, raftq_step_batch of
          them, the N - 1 64-byte raftq_wire_msg_t MsgVotes per result built on the host into page-locked memory (the way
          raftq_node's apply_result does; here with numpy, one vectorised pass per field), then raftq_wire_encode;
  device  raftq_tick_elect_frames: the Tick, its lists, the campaigns, the records and their marshal in one submission.

Shapes: 32,768 groups x 3 peers with a third of the groups' timers firing, and 1M groups x 5 with every 20th firing (52,429:
DESIGN.md 4.7's list shape).  Every group is a follower or a candidate; beat_cap is 0.  A campaign moves the state, so before
every timed call the timers are put back (raftq_load_roles: the firing groups one tick short of a certain timeout, the others at
0) and one untimed no-op Step batch re-reads the records' copies of the dense arrays -- both forms then start from the same
kind of state; the terms grow by one per call, in both forms alike.  Per form and shape: median, min, max, p10 / p90 of CALLS
timed calls after WARM untimed ones, host clock around calls that end in the device wait.  `host` is reported whole and split
(tick call | MsgHup build | step call | MsgVote build | encode call).  Frame counts are compared on every call; byte parity is
tests/test_tick_elect_gpu.py's business.

usage: tools/profile_tick_elect.py [out.json]      (default profiles/r11/tick_elect.json; CALLS, WARM from the environment)
Needs the GPU: no CPU path exists, and without a device the handle cannot be created."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = int(os.environ.get("CALLS", "100"))
WARM = int(os.environ.get("WARM", "10"))
ET = 10
MSG_HUP, MSG_BEAT, MSG_VOTE, OUT_CAMPAIGN = 0, 1, 5, 3


def stats(ns):
    a = np.sort(np.asarray(ns, np.float64)) / 1e3
    return {"median_us": float(np.median(a)), "min_us": float(a[0]), "max_us": float(a[-1]), "p10_us": float(a[len(a) // 10]),
            "p90_us": float(a[(len(a) * 9) // 10]), "calls": len(a)}


def shape(G, N, fire_every, device=0):
    from raftsql_amd import _lib
    from raftsql_amd import step as S
    from raftsql_amd.engine import pinned_empty
    from raftsql_amd.wire import WIRE_MSG_DT, WireEngine

    me = 0
    rng = np.random.default_rng(11 + N)
    fire = np.arange(0, G, fire_every)
    n_fire, slices = len(fire), N - 1
    n_frames = n_fire * slices
    role = np.zeros(G, np.uint8)
    elapsed = np.zeros(G, np.uint32)
    elapsed[fire] = 2 * ET - 1  # one tick short of a timeout no draw exceeds
    quiet = 1 if fire_every > 1 else None
    term = rng.integers(1, 1 << 20, G).astype(np.uint64)
    last = rng.integers(1, 1 << 30, G).astype(np.uint64)
    match = np.zeros((N, G), np.uint64)
    match[me] = last
    with WireEngine(G, N, me, device=device) as e:
        lib, h = e._lib, e._h
        e.set_timers(ET, 1, 7)
        e.load_match(match, np.zeros(G, np.uint64))
        e.load_roles(role, elapsed)
        e.load_node(term, np.zeros(G, np.uint32), np.zeros(G, np.uint32), last, term)
        cap = e.respond_cap(n_fire)
        out_h, out_d = pinned_empty(cap, np.uint8), pinned_empty(cap, np.uint8)
        off_h, off_d = pinned_empty(n_frames + 1, np.uint64), pinned_empty(n_frames + 1, np.uint64)
        po = pinned_empty(2 * (N + 1), np.uint64)
        camp = pinned_empty(n_fire, S.OUT_S_DT)
        recs = pinned_empty(n_frames, WIRE_MSG_DT)
        hup_msgs, outs = pinned_empty(n_fire, S.MSG_DT), pinned_empty(n_fire, S.OUT_DT)
        noop = S.pack_msgs(np.array([quiet if quiet is not None else 0], np.uint64), MSG_BEAT)  # MsgBeat to a non-leader: nothing happens
        nh, nb = C.c_uint64(0), C.c_uint64(0)
        ch, cd = _lib.WireCounts(), _lib.WireCounts()
        ph, lh = C.c_void_p(None), C.c_uint64(0)

        def reset():
            e.load_roles(role, elapsed)
            if quiet is not None:
                e.step_batch(noop)

        def host_form():
            t0 = time.perf_counter_ns()
            e._chk(lib.raftq_tick_collect_lists(h, _lib.TICK_BEAT_BITMAP, G, 0, C.byref(nh), C.byref(nb)))
            e._chk(lib.raftq_last_tick_lists(h, C.byref(ph), C.byref(lh), None, None, None, None))
            t1 = time.perf_counter_ns()
            k = int(lh.value)
            g = np.frombuffer((C.c_char * (k * 4)).from_address(ph.value), dtype=np.uint32)
            m = hup_msgs[:k]
            m[:] = np.zeros(1, S.MSG_DT)[0]
            m["group"], m["type"] = g, MSG_HUP
            t2 = time.perf_counter_ns()
            e._chk(lib.raftq_step_batch(h, m.ctypes.data, k, outs.ctypes.data, None))
            t3 = time.perf_counter_ns()
            o = outs[:k]
            recs[: k * slices] = np.zeros(1, WIRE_MSG_DT)[0]
            s = 0
            for p in range(N):
                if p == me:
                    continue
                r = recs[s * k:(s + 1) * k]
                r["group"], r["term"], r["type"], r["to"], r["from"] = g, o["term"], MSG_VOTE, p, me
                r["index"], r["log_term"] = o["index"], o["log_term"]
                s += 1
            t4 = time.perf_counter_ns()
            e._chk(lib.raftq_wire_encode(h, recs.ctypes.data, k * slices, None, 0, None, 0, out_h.ctypes.data, cap, off_h.ctypes.data, C.byref(ch)))
            t5 = time.perf_counter_ns()
            assert k == n_fire and int((o["type"] == OUT_CAMPAIGN).sum()) == k, (k, n_fire)
            return t5 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4

        def device_form():
            t0 = time.perf_counter_ns()
            e._chk(lib.raftq_tick_elect_frames(h, _lib.TICK_BEAT_BITMAP, n_fire, 0, C.byref(nh), C.byref(nb), camp.ctypes.data, out_d.ctypes.data, cap,
                                               off_d.ctypes.data, po.ctypes.data, C.byref(cd)))
            return time.perf_counter_ns() - t0

        th, td = [], []
        for i in range(WARM + CALLS):
            reset()
            a = host_form()
            reset()
            b = device_form()
            assert nh.value == n_fire and cd.n_msgs == n_frames == ch.n_msgs, (nh.value, n_fire, cd.n_msgs, ch.n_msgs)
            assert int((camp["type"] == OUT_CAMPAIGN).sum()) == n_fire
            if i >= WARM:
                th.append(a)
                td.append(b)
        th = np.asarray(th)
        return {"groups": G, "peers": N, "campaigns_per_tick": n_fire, "frames_per_tick": n_frames, "stream_bytes": int(cd.bytes),
                "host_records_bytes_over_the_link": n_fire * 64 + n_frames * 64, "frame_counts_identical": True,
                "host_form": {"whole": stats(th[:, 0]), "tick_collect_lists": stats(th[:, 1]), "msghup_build_numpy": stats(th[:, 2]),
                              "step_batch": stats(th[:, 3]), "msgvote_build_numpy": stats(th[:, 4]), "wire_encode": stats(th[:, 5])},
                "device_form": {"tick_elect_frames": stats(td)}}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11", "tick_elect.json")
    import torch

    assert torch.cuda.is_available(), "tools/profile_tick_elect.py measures on the GPU; there is none here"
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    rec = {"what": "election round: raftq_tick_collect_lists + raftq_step_batch of host-built MsgHups + host-built MsgVotes + raftq_wire_encode against "
                   "raftq_tick_elect_frames, alternated",
           "device": torch.cuda.get_device_name(0), "tree": head, "calls": CALLS, "warm": WARM, "clock": "time.perf_counter_ns around calls that wait",
           "shapes": [shape(32768, 3, 3), shape(1 << 20, 5, 20)]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
