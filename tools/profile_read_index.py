#!/usr/bin/env python3
"""What raftq_set_read_index costs a handle that has CheckQuorum on: the bench's pipelined Step leg (bench.step_measure, the leg
tools/profile_check_quorum.py and profiles/r24 measure) over engines with raftq_set_check_quorum on and

  off    the read switch off: the *_cq_* walks as every such handle launches them.  This setting runs in ANY tree -- it names
         nothing the parent lacks -- so the same file measures the parent: run it with the parent's root as the working directory
  lease  RAFTQ_READ_LEASE on (no read traffic in the bench's mix: the run-time test alone)
  safe   RAFTQ_READ_SAFE on (likewise; the read records allocated and never touched)
  safe10 RAFTQ_READ_SAFE on and 10 % of every batch read traffic: one record in twenty a local MsgReadIndex, one in twenty a
         MsgHeartbeatResp that carries a context (1 or 2: within what the requests have handed out after the first batch).  The
         bench's batches are rewritten as they are packed; everything else about the leg is the bench's

One process per run, as profiles/r24's legs_ab.jsonl: the caller alternates trees and settings.  Prints one JSON line.
usage (from the root of the tree to measure): python PATH/tools/profile_read_index.py off|lease|safe|safe10 [label]     (on the GPU box)"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import bench  # noqa: E402
from raftsql_amd import step as S  # noqa: E402


def main():
    setting = sys.argv[1] if len(sys.argv) > 1 else "off"
    label = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(os.getcwd())
    plain = S.NodeEngine

    class Checked(plain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_check_quorum(True)
            if setting != "off":
                self.set_read_index({"safe": 1, "safe10": 1, "lease": 2}[setting])

    pack, rng, share = S.pack_msgs, np.random.default_rng(30), {"reads": 0, "acks": 0, "all": 0}

    def pack_with_reads(group, type, **kw):
        m = pack(group, type, **kw)
        u = rng.random(len(m))
        req, ack = u < 0.05, (u >= 0.05) & (u < 0.10)
        m["type"][req], m["term"][req], m["from"][req], m["index"][req] = S.MSG_READ_INDEX, 0, 0, 0
        m["type"][ack], m["term"][ack], m["reject"][ack] = S.MSG_HEARTBEAT_RESP, 3, 0
        m["index"][ack] = rng.integers(1, 3, int(ack.sum()))
        share["reads"] += int(req.sum())
        share["acks"] += int(ack.sum())
        share["all"] += len(m)
        return m

    S.NodeEngine = Checked
    if setting == "safe10":
        S.pack_msgs = pack_with_reads
    try:
        r = bench.step_measure(bench.CONFIGS[3], 0, with_cpu=False)
    finally:
        S.NodeEngine, S.pack_msgs = plain, pack
    p = r["pipelined"]
    print(json.dumps({"tree": label, "check_quorum": True, "read_index": setting, "unit": "1e9 msgs/s",
                      "pipelined_32B": round(p["short_results"]["msgs_per_s"] / 1e9, 4),
                      **({"read_requests": round(share["reads"] / share["all"], 4), "context_acks": round(share["acks"] / share["all"], 4)} if share["all"] else {}),
                      **({"pipelined_64B": round(p["msgs_per_s"] / 1e9, 4)} if "msgs_per_s" in p else {})}))


if __name__ == "__main__":
    main()
