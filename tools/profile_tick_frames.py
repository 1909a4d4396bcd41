#!/usr/bin/env python3
"""A node's heartbeat round, two forms in one process, alternated call by call on the same handle:

  host    today's form: raftq_tick_collect_lists with the MsgBeat bitmap, the 64-byte raftq_wire_msg_t records of bcastHeartbeat
          built on the host into page-locked memory (from the bitmap and the host's own copies of term / committed / match, the way
          raftq_node's bcast_heartbeat does; here with numpy, one vectorised pass per field), then raftq_wire_encode;
  device  raftq_tick_frames: the Tick, its lists, the records and their marshal in one submission.

Shapes: 32,768 groups x 3 peers, all led (the one-node leg's), and 1M groups x 5 with a quarter led.  HeartbeatTick 1: every led
group beats on every tick; ElectionTick is set out of reach so that the followers of the second shape never raise MsgHup and every
call does the same work.  Per form and shape: median, min, max, p10 / p90 of CALLS timed calls after WARM untimed ones, host clock
around calls that end in the device wait.  `host` is reported whole and split (tick call | record build | encode call).  The two
forms' bytes are compared on the first timed call.

usage: tools/profile_tick_frames.py [out.json]      (default profiles/r10/tick_frames.json; CALLS, WARM from the environment)
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
CALLS = int(os.environ.get("CALLS", "200"))
WARM = int(os.environ.get("WARM", "20"))
MSG_HEARTBEAT = 8


def stats(ns):
    a = np.sort(np.asarray(ns, np.float64)) / 1e3
    return {"median_us": float(np.median(a)), "min_us": float(a[0]), "max_us": float(a[-1]), "p10_us": float(a[len(a) // 10]),
            "p90_us": float(a[(len(a) * 9) // 10]), "calls": len(a)}


def shape(G, N, led_every, device=0):
    from raftsql_amd import _lib
    from raftsql_amd.engine import pinned_empty
    from raftsql_amd.wire import WIRE_MSG_DT, WireEngine

    me = 0
    rng = np.random.default_rng(10 + N)
    role = np.zeros(G, np.uint8)
    role[::led_every] = 2
    led = np.nonzero(role == 2)[0]
    term = rng.integers(1, 1 << 20, G).astype(np.uint64)
    committed = rng.integers(1, 1 << 30, G).astype(np.uint64)
    match = np.zeros((N, G), np.uint64)
    for p in range(N):  # followers a little behind or at the commit index, the leader's own row ahead
        match[p] = committed - rng.integers(0, 2, G).astype(np.uint64) if p != me else committed + np.uint64(1)
    last = committed + np.uint64(1)
    n_led, slices = len(led), N - 1
    n_frames = n_led * slices
    with WireEngine(G, N, me, device=device) as e:
        lib, h = e._lib, e._h
        e.set_timers(1 << 30, 1, 7)
        e.load_match(match, committed)
        e.load_roles(role, np.zeros(G, np.uint32))
        e.load_node(term, np.where(role == 2, me + 1, 0).astype(np.uint32), np.where(role == 2, me + 1, 0).astype(np.uint32), last, term)
        cap = e.respond_cap(n_led)
        out_h, out_d = pinned_empty(cap, np.uint8), pinned_empty(cap, np.uint8)
        off_h, off_d = pinned_empty(n_frames + 1, np.uint64), pinned_empty(n_frames + 1, np.uint64)
        po = pinned_empty(N + 1, np.uint64)
        recs = pinned_empty(n_frames, WIRE_MSG_DT)
        nh, nb = C.c_uint64(0), C.c_uint64(0)
        ch, cd = _lib.WireCounts(), _lib.WireCounts()
        pm, lm = C.c_void_p(None), C.c_uint64(0)

        def host_form():
            t0 = time.perf_counter_ns()
            e._chk(lib.raftq_tick_collect_lists(h, _lib.TICK_BEAT_BITMAP, G, 0, C.byref(nh), C.byref(nb)))
            e._chk(lib.raftq_last_tick_lists(h, None, None, None, None, C.byref(pm), C.byref(lm)))
            t1 = time.perf_counter_ns()
            words = np.frombuffer((C.c_char * (lm.value * 8)).from_address(pm.value), dtype=np.uint8)
            g = np.nonzero(np.unpackbits(words, bitorder="little")[:G])[0]
            k = len(g)
            recs[: k * slices] = np.zeros(1, WIRE_MSG_DT)[0]
            s = 0
            for p in range(N):
                if p == me:
                    continue
                r = recs[s * k:(s + 1) * k]
                r["group"], r["term"], r["type"], r["to"], r["from"] = g, term[g], MSG_HEARTBEAT, p, me
                r["commit"] = np.minimum(match[p][g], committed[g])
                s += 1
            t2 = time.perf_counter_ns()
            e._chk(lib.raftq_wire_encode(h, recs.ctypes.data, k * slices, None, 0, None, 0, out_h.ctypes.data, cap, off_h.ctypes.data, C.byref(ch)))
            t3 = time.perf_counter_ns()
            return t3 - t0, t1 - t0, t2 - t1, t3 - t2

        def device_form():
            t0 = time.perf_counter_ns()
            e._chk(lib.raftq_tick_frames(h, _lib.TICK_BEAT_BITMAP, G, n_led, C.byref(nh), C.byref(nb), out_d.ctypes.data, cap, off_d.ctypes.data,
                                         po.ctypes.data, C.byref(cd)))
            return time.perf_counter_ns() - t0

        for _ in range(WARM):
            host_form()
            device_form()
        assert nb.value == n_led and cd.n_msgs == n_frames == ch.n_msgs, (nb.value, n_led, cd.n_msgs, ch.n_msgs)
        same = ch.bytes == cd.bytes and bytes(out_h[: ch.bytes]) == bytes(out_d[: cd.bytes]) and np.array_equal(off_h, off_d)
        assert same, "the two forms' streams differ"
        th, td = [], []
        for _ in range(CALLS):
            th.append(host_form())
            td.append(device_form())
        th = np.asarray(th)
        return {"groups": G, "peers": N, "led_groups": n_led, "frames_per_tick": n_frames, "stream_bytes": int(cd.bytes),
                "host_records_bytes_over_the_link": n_frames * 64, "streams_identical": bool(same),
                "host_form": {"whole": stats(th[:, 0]), "tick_collect_lists": stats(th[:, 1]), "record_build_numpy": stats(th[:, 2]),
                              "wire_encode": stats(th[:, 3])},
                "device_form": {"tick_frames": stats(td)}}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10", "tick_frames.json")
    import torch

    assert torch.cuda.is_available(), "tools/profile_tick_frames.py measures on the GPU; there is none here"
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    rec = {"what": "heartbeat round: raftq_tick_collect_lists + host-built records + raftq_wire_encode against raftq_tick_frames, alternated",
           "device": torch.cuda.get_device_name(0), "tree": head, "calls": CALLS, "warm": WARM, "clock": "time.perf_counter_ns around calls that wait",
           "shapes": [shape(32768, 3, 1), shape(1 << 20, 5, 4)]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
