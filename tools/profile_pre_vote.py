#!/usr/bin/env python3
"""The bench's pipelined Step leg under raftq_set_check_quorum with raftq_set_pre_vote off and on -- one box, one process.

bench.step_measure as it stands, over engines that turn the switches on when they are made:
  cq        raftq_set_check_quorum alone: the *_cq_* walks with NodeArrays::pv clear
  cq_pv     both switches: the same walks with the flag set
alternated in pairs, PAIRS times.  The leg's mix (acknowledgements, heartbeat responses, 5 % MsgVote of a higher term, stale
stragglers) holds no MsgHup and neither of the two new kinds, so the two settings apply the same state changes: what differs is the
flag's tests in the walk.  Reported: the pipelined rate with 32-byte results, 1e9 messages/s, every run.

In a tree that has no raftq_set_pre_vote (the parent commit's, to which this file is copied for the comparison) only `cq` is
measured: the parent's CheckQuorum-on figure, taken by the same code.
usage: tools/profile_pre_vote.py [out.json] [--pairs K]      (run on the GPU box)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def step_leg(pairs):
    import bench
    from raftsql_amd import step as S
    from raftsql_amd.engine import QuorumEngine

    plain = S.NodeEngine
    has_pv = hasattr(QuorumEngine, "set_pre_vote")

    class Checked(plain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_check_quorum(True)

    class PreVoting(Checked):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_pre_vote(True)

    settings = (("cq", Checked), ("cq_pv", PreVoting)) if has_pv else (("cq", Checked),)
    cfg = bench.CONFIGS[3]
    out = {key: [] for key, _ in settings}
    for _ in range(pairs):
        for key, cls in settings:
            S.NodeEngine = cls
            try:
                r = bench.step_measure(cfg, 0, with_cpu=False)
            finally:
                S.NodeEngine = plain
            out[key].append(round(r["pipelined"]["short_results"]["msgs_per_s"] / 1e9, 4))
    return {"what": "bench.step_measure, pipelined, 32-byte results, 1e9 messages/s; %d alternated runs of each setting, in run order" % pairs,
            "has_raftq_set_pre_vote": has_pv, **out}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pairs = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 3
    if "--pairs" in sys.argv:
        args = [a for a in args if a != sys.argv[sys.argv.index("--pairs") + 1]]
    text = json.dumps(step_leg(pairs))
    print(text)
    if args:
        with open(args[0], "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
