#!/usr/bin/env python3
"""raftq_propose_frames with every switch off: 32,768 led groups x 3 peers, one 64-byte statement each -> 65,536 MsgApps a call.
For parent / child comparisons: run it from the root of the tree to be measured (it imports that tree's package), in a process of
its own per run, the trees alternated; TREE in the environment names the tree in the record.  Prints one JSON line: the median and
range of TURNS medians of CALLS calls (the state reloaded before every call, not timed), wall us, and a digest of the stream.
usage: cd TREE_ROOT && TREE=name python PATH/tools/profile_propose_leg.py      (run on the GPU box)"""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from raftsql_amd import wire as W
from raftsql_amd.engine import pinned_copy, pinned_empty
from raftsql_amd.wire import WireEngine

G, N, ME, TERM, PAYLOAD, CALLS, TURNS = 32768, 3, 0, 7, 64, 8, 5
rng = np.random.default_rng(23)
last = rng.integers(50, 100000, G).astype(np.uint64)
props = np.zeros(G, W.PROP_DT)
props["group"], props["ent_first"], props["n_ents"] = rng.permutation(G), np.arange(G), 1
pe = np.zeros(G, W.PROP_ENT_DT)
pe["data_len"], pe["data_off"] = PAYLOAD, np.arange(G) * PAYLOAD
pool = pinned_copy(rng.integers(0, 256, G * PAYLOAD, dtype=np.uint8))
pp, ppe = pinned_copy(props), pinned_copy(pe)
nm, ne = pinned_empty(0, W.WIRE_MSG_DT), pinned_empty(0, W.WIRE_ENT_DT)
out, off = pinned_empty(G * (N - 1) * (128 + PAYLOAD), np.uint8), pinned_empty(G * (N - 1) + 1, np.uint64)
meds = []
with WireEngine(G, N, ME, device=0) as e:
    for turn in range(TURNS + 1):
        ts = []
        for _ in range(CALLS):
            match = np.tile(last - np.uint64(1), (N, 1))
            match[ME] = last
            e.load_match(match, last - np.uint64(1))
            e.load_terms(np.full(G, TERM, np.uint64), np.ones(G, np.uint64))
            e.load_roles(np.full(G, 2, np.uint8))
            e.load_node(np.full(G, TERM, np.uint64), np.full(G, ME + 1, np.uint32), np.full(G, ME + 1, np.uint32), last, np.full(G, TERM - 2, np.uint64))
            t0 = time.perf_counter()
            r = e.propose_frames(pp, ppe, nm, ne, pool, out, off)
            ts.append((time.perf_counter() - t0) * 1e6)
        if turn:
            meds.append(float(np.median(ts)))
    digest = hashlib.sha256(bytes(r[0])).hexdigest()[:16]
print(json.dumps({"tree": os.environ.get("TREE", "?"), "leg": "propose_frames, 65,536 MsgApps a call", "median_us": round(float(np.median(meds)), 1),
                  "min_us": round(min(meds), 1), "max_us": round(max(meds), 1), "frames": int(r[2].n_msgs), "bytes": int(r[2].bytes), "sha256_16": digest}))
