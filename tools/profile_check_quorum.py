#!/usr/bin/env python3
"""The Tick leg under raftq_set_check_quorum (tick_check_kernel) beside the plain Tick (tick_kernel), and the bench's pipelined
Step leg with the switch on beside the same leg with it off -- one box, one process.

Tick: two populations of 8 handles x 1M groups x 5 peers in the same state (roles as the bench's Tick leg: one group in three
led; election_tick 60,000 so that no follower's timer is past its base timeout: the bench's steady state), each in a sweep set so
that its 8 raftq_tick launches share one stream and HIP events time exactly them:
  plain          the switch off: 8 x tick_kernel, 10 B per group            (the set's ONE dispatch, raftq_set_tick, beside it)
  steady         the switch on, no check due: 8 x tick_check_kernel, 18 B per group
  all_due        ... every leader's check due on this tick, all passing (activity words full)
  one_pct_fail   ... every leader's check due on this tick, 1 % of them failing (action 3, third bitmap)
The settings are ALTERNATED in pairs (plain, then one switched-on state), TURNS times, REPS timed rounds a turn; the two states
with checks due reload the activity words before every round (outside the clock).  Reported: the median and range of the turns'
medians in us per round of 8 launches, bytes per group, and the fraction of 8 TB/s.
Expectation from the arrays: 18 B per group against 10; HBM-bound that is x1.8.
usage: tools/profile_check_quorum.py [out.json]      (run on the GPU box)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raftsql_amd import _lib  # noqa: E402
from raftsql_amd.engine import QuorumEngine, SweepSet  # noqa: E402

G, N, K = 1 << 20, 5, 8
ET, HB, SEED, TURNS, REPS = 60000, 1, 0x1000, 5, 20
HBM = 8e12
STATES = ("steady", "all_due", "one_pct_fail")


def population(on):
    role = (np.arange(G) % 3).astype(np.uint8)
    es = []
    for _ in range(K):
        e = QuorumEngine(G, N)
        e._chk(_lib.load().raftq_set_self(e._h, 0))
        e.set_timers(ET, HB, SEED)
        e.load_roles(role)
        if on:
            e.set_check_quorum(True)
        es.append(e)
    return es, role


def reload(es, role, state, rng):
    """the followers' clocks back to 0 (nobody draws), the activity words as the state wants them"""
    full = (1 << N) - 1
    active = np.full(G, full, np.uint16)
    if state == "one_pct_fail":
        active[rng.random(G) < 0.01] = 0
    le = np.full(G, 0 if state == "steady" else ET - 1, np.uint32)
    for e in es:
        e.load_roles(role)
        if state is not None:
            e.load_activity(active, le)


def rounds(s, es, reps, before=None):
    out = []
    for _ in range(reps):
        if before:
            before()
        s.timer_begin()
        for e in es:
            e.tick(want_counts=False)
        out.append(s.timer_end() * 1e3)
    return out


def summary(meds, bytes_per_group):
    m = float(np.median(meds))
    return {"median_us": round(m, 2), "min_us": round(min(meds), 2), "max_us": round(max(meds), 2), "bytes_per_group": bytes_per_group,
            "frac_of_8TBps": round(bytes_per_group * G * K / (m * 1e-6) / HBM, 3)}


def tick_leg():
    rng = np.random.default_rng(24)
    off, role = population(False)
    on, _ = population(True)
    rec = {}
    with SweepSet(off) as s_off, SweepSet(on) as s_on:
        for state in STATES:
            meds = {"plain": [], state: [], "plain_set_dispatch": []}
            for turn in range(TURNS + 1):  # turn 0 warms up and is dropped
                reload(off, role, None, rng)
                a = rounds(s_off, off, REPS)
                s_off.timer_begin()
                for _ in range(REPS):
                    s_off.tick()
                d = s_off.timer_end() * 1e3 / REPS
                if state == "steady":
                    reload(on, role, state, rng)
                    b = rounds(s_on, on, REPS)
                else:
                    b = rounds(s_on, on, max(REPS // 4, 3), before=lambda: reload(on, role, state, rng))
                if turn:
                    meds["plain"].append(float(np.median(a)))
                    meds[state].append(float(np.median(b)))
                    meds["plain_set_dispatch"].append(d)
            reload(on, role, state, rng)  # what the timed tick does, counted once on one handle
            n_hup, n_beat = on[0].tick()
            last = {"n_hup": n_hup, "n_beat": n_beat, "n_checks_failing": on[0].collect_checks(cap=0)[1], "leaders": int((role == 2).sum())}
            rec[state] = {"plain": summary(meds["plain"], 10), "switch_on": summary(meds[state], 18),
                          "plain_set_dispatch": summary(meds["plain_set_dispatch"], 10), "on_the_timed_tick": last,
                          "on_over_plain": round(float(np.median(meds[state])) / float(np.median(meds["plain"])), 3)}
    for e in off + on:
        e.close()
    return rec


def step_leg(pairs=3):
    """bench.step_measure as it stands (switch off) alternated with the same function over engines that turned the switch on"""
    import bench
    from raftsql_amd import step as S

    plain = S.NodeEngine

    class Checked(plain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_check_quorum(True)

    cfg = bench.CONFIGS[3]
    out = {"off": [], "on": []}
    for _ in range(pairs):
        for key, cls in (("off", plain), ("on", Checked)):
            S.NodeEngine = cls
            try:
                r = bench.step_measure(cfg, 0, with_cpu=False)
            finally:
                S.NodeEngine = plain
            out[key].append(r["pipelined"]["short_results"]["msgs_per_s"])
    return {"what": "bench.step_measure, pipelined, 32-byte results, messages/s; %d alternated pairs" % pairs,
            "switch_off": sorted(round(x / 1e9, 3) for x in out["off"]), "switch_on": sorted(round(x / 1e9, 3) for x in out["on"]), "unit": "1e9 msgs/s"}


def main():
    rec = {"what": "us per round of %d raftq_tick launches (%d handles x %d groups x %d peers on one stream, HIP events); %d alternated turns, "
                   "median and range of the turns' medians" % (K, K, G, N, TURNS),
           "expectation_by_bytes": "18 B per group against 10: x1.8 when HBM-bound", "tick": tick_leg()}
    if os.environ.get("CQ_STEP", "1") != "0":
        rec["step"] = step_leg()
    text = json.dumps(rec, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
