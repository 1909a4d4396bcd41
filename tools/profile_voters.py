#!/usr/bin/env python3
"""The masked sweep (sweep_voters_kernel) against the unmasked sweep_kernel at the README's n1 shape: ONE launch of 1M x 5,
commit + votes, streamed, over 33 resident handles per variant so that no launch is served from the Infinity Cache.  Four
variants in one process, their runs alternated: unmasked as loaded (the self row is skipped: 4 rows read), unmasked with the
self-max fact broken in one group (all 5 rows read: what the masked sweep's bytes compare with), masked with every mask
full, masked with random masks.  Per variant: median and min-max over the rounds of the per-round median launch time.
usage: tools/profile_voters.py [out.json]      (run on the GPU box)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import _lib, synth  # noqa: E402
from raftsql_amd.engine import QuorumEngine  # noqa: E402

N, G, K, ROUNDS = 5, 1 << 20, 33, 9
FLAGS = _lib.SWEEP_COMMIT | _lib.SWEEP_VOTES | _lib.SWEEP_NO_ADOPT | _lib.SWEEP_STREAM
VARIANTS = ("unmasked_self_row_skipped", "unmasked_all_rows", "masked_full", "masked_random")


def main():
    st = synth.make_groups(G, N, seed=synth.SEED_BASE + N, with_terms=True)
    rng = np.random.default_rng(9)
    random_masks = rng.integers(0, 1 << N, G).astype(np.uint16)
    sets = {}
    for v in VARIANTS:
        es = [QuorumEngine(G, N) for _ in range(K)]
        es[0].load_state(st)
        if v == "unmasked_all_rows":  # one follower one above its leader in one group: the sweep reads every row again
            es[0].apply_deltas(np.array([0], np.uint64), np.array([1], np.uint32), st.match[0, :1] + np.uint64(1))
            assert es[0].self_max() == -1
        if v == "masked_full":
            es[0].load_voters(np.full(G, (1 << N) - 1, np.uint16))
        if v == "masked_random":
            es[0].load_voters(random_masks)
        for e in es[1:]:
            e.clone_state_from(es[0])
        sets[v] = es
    assert sets["unmasked_self_row_skipped"][1].self_max() == 0 and sets["masked_random"][1].read_voters().tobytes() == random_masks.tobytes()
    per_round = {v: [] for v in VARIANTS}
    for r in range(ROUNDS + 1):  # round 0 warms every variant up and is dropped
        for v in VARIANTS[r % len(VARIANTS):] + VARIANTS[:r % len(VARIANTS)]:  # the order rotates from round to round
            t = []
            for e in sets[v]:  # every handle has its own stream: each launch is timed on its own
                e.timer_begin()
                e.step_async(FLAGS)
                t.append(e.timer_end() * 1e3)
            if r:
                per_round[v].append(float(np.median(t)))
    rec = {"what": "one launch of %d x %d, commit + votes, streamed, NO_ADOPT; %d resident handles per variant, launches timed one by one "
                   "with HIP events; %d rounds, the variants' order rotated; us per launch" % (G, N, K, ROUNDS),
           "algorithmic_bytes_per_decision": {"unmasked_all_rows": 58.25, "masked": 60.25, "ratio": round(60.25 / 58.25, 4)}, "variants": {}}
    for v in VARIANTS:
        a = np.array(per_round[v])
        rec["variants"][v] = {"median_us": round(float(np.median(a)), 3), "min_us": round(float(a.min()), 3), "max_us": round(float(a.max()), 3),
                              "per_round_median_us": [round(x, 3) for x in per_round[v]]}
    base = rec["variants"]["unmasked_all_rows"]
    for v in ("masked_full", "masked_random"):
        rec["variants"][v]["ratio_to_unmasked_all_rows"] = round(rec["variants"][v]["median_us"] / base["median_us"], 4)
    rec["unmasked_all_rows_spread"] = round((base["max_us"] - base["min_us"]) / base["median_us"], 4)
    # a full mask everywhere decides what the unmasked sweep decides
    a, b = sets["masked_full"][1], sets["unmasked_all_rows"][1]
    rec["masked_full_equals_unmasked"] = bool(np.array_equal(a.read_committed(), b.read_committed()) and np.array_equal(a.read_outcome(), b.read_outcome()))
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
