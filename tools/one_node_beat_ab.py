#!/usr/bin/env python3
"""The one-node leg (bench.py one_node_measure: 32,768 groups x 3 led by ONE node, scripted peers, WAL on) with
RAFTQ_NODE_BEAT_DEVICE=0 and =1, alternated, RUNS runs each, one handle (shard_counts=(1,)), each run in a child process of its
own (the option is read when a node is created) with RAFTQ_PROFILE=1: the node's phase split goes to the child's stderr when
its handles are destroyed.  One JSON line per run to stdout and to OUT (default profiles/r10/beat_one_node.jsonl), the
phase lines kept beside the rates.  The leg ticks on the reference's 100 ms ticker (raft.go:217), so only the turns on which
it fires pay for a heartbeat round: the `tick` phase of the profile is where the two settings differ."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = int(os.environ.get("RUNS", "3"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r10", "beat_one_node.jsonl"))
CHILD = ("import json, bench; r = bench.one_node_measure(0, shard_counts=(1,)); "
         "print('RESULT ' + json.dumps({k: r[k] for k in ('proposals_committed_per_s', 'ms_per_turn', 'no_wal')}))")


def main():
    rows = []
    for run in range(RUNS):
        for knob in ("0", "1"):
            env = dict(os.environ, RAFTQ_NODE_BEAT_DEVICE=knob, RAFTQ_PROFILE="1")
            p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
                sys.exit(p.returncode or 1)
            res = [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
            phases = [l for l in (p.stdout + p.stderr).splitlines() if "phase" in l.lower() or "advance" in l.lower()][-12:]
            row = {"run": run, "RAFTQ_NODE_BEAT_DEVICE": int(knob), **res, "profile": phases}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
