"""The reference of the fused Tick calls under CheckQuorum and PreVote (raftq_tick_set_checks, include/raftq.h "CheckQuorum";
include/raftq_wire.h raftq_tick_frames / raftq_tick_elect_frames): one Tick, its three lists, the heartbeat round and the election
round, COMPOSED of what the suite already trusts and of nothing else --

  the Tick        ref_check_quorum.tick_array (oracle.pyoracle.tick, ref_tick_members.tick_array over masks, the leader's check on top)
  the campaigns   ref_check_quorum.step_batch, or ref_pre_vote.step_batch under PreVote, on MSG_HUP records of the first hup_cap MsgHup
                  groups: the state they leave, and the result records camp[] packs
  the sections    test_tick_frames_gpu.want_frames / ref_tick_members.member_beats for the heartbeats, ref_tick_members' slot rule and
                  positional offsets for both
  the bytes       oracle.pywire.wire_encode

-- and the generators of the GPU tests' inputs (tests/test_tick_checks_ref.py shows that each of them discriminates).
TEST INFRASTRUCTURE: nothing in the product imports it."""
import functools

import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from tests import ref_check_quorum as Q
from tests import ref_pre_vote as PV
from tests import ref_step_voters as V
from tests import ref_tick_members as M

MSG_HUP, MSG_VOTE, MSG_PRE_VOTE = 0, 5, 17
OUT_CAMPAIGN, OUT_BECAME_LEADER, OUT_PRE_CAMPAIGN = 3, 4, 14
OUTF_HARDSTATE, OUTF_ANSWERED = 0x01, 0x10
ET, SEED = 10, 0x7157  # (test_tick_frames_gpu's)
TICKS = 3


def copy_case(st, active, lead_elapsed):
    return V.copy_state(st), active.copy(), lead_elapsed.copy()


def tick(st, active, lead_elapsed, voters, hb, tick_no, et=ET, seed=SEED):
    """ref_check_quorum.tick_array on the state (st.elapsed, active and lead_elapsed MOVE) -> action u8 [G].
    active is None: both switches off -- the Tick ref_check_quorum.tick_array puts the check on top of"""
    if active is None:
        if voters is None:
            el, act, _, _ = pyoracle.tick(st.role, st.elapsed, et, hb, seed, tick_no)
        else:
            el, act, _, _ = M.tick_array(pyoracle, st.role, st.elapsed, voters, st.self_peer, et, hb, seed, tick_no)
        st.elapsed[:] = el
        return act
    el, act, ac, le, _, _ = Q.tick_array(pyoracle, st.role, st.elapsed, active, lead_elapsed, voters, st.self_peer, st.N, et, hb, seed, tick_no)
    st.elapsed[:], active[:], lead_elapsed[:] = el, ac, le
    return act


def campaigns(st, active, lead_elapsed, voters, hups, hup_cap, pre_vote, et=ET, plain_hup=False, step=None):
    """Step(MsgHup) of the first hup_cap MsgHup groups with the switches on (the state MOVES) -> (every positional record of the vote
    section, keep [slots] bool, camp records, campaigned ids, the raw 64-byte results).
    plain_hup (tests only): PreVote's rule 1 left out -- the MsgHup is stepped as a plain campaign.
    step: msgs -> raftq_step_out_t[], for a caller whose handle has more switches on than the two (it moves the caller's state)."""
    from raftsql_amd import step as S

    N, me = st.N, st.self_peer
    built = np.asarray(hups[:hup_cap], np.int64)
    msgs = S.pack_msgs(built.astype(np.uint64), MSG_HUP)
    if len(built) == 0:
        outs = np.zeros(0, S.OUT_DT)
    elif step is not None:
        outs = step(msgs)
    elif active is None:  # both switches off: the statements the two references override
        outs = st.step_batch(msgs) if voters is None else V.step_batch(st, voters, msgs)
    elif pre_vote:
        outs = PV.step_batch(st, voters, active, lead_elapsed, msgs, et, leave_out={1} if plain_hup else frozenset())
    else:
        outs = Q.step_batch(st, voters, active, lead_elapsed, msgs, et)
    assert np.isin(outs["type"], (OUT_CAMPAIGN, OUT_BECAME_LEADER, OUT_PRE_CAMPAIGN)).all(), "Step(MsgHup) of a non-leader campaigns"
    pre, asks = outs["type"] == OUT_PRE_CAMPAIGN, outs["type"] != OUT_BECAME_LEADER
    camp = np.zeros(len(built), S.OUT_S_DT)
    for k in ("term", "index", "vote", "lead", "type", "reject", "role"):
        camp[k] = outs[k]
    camp["commit"] = np.where(asks, outs["log_term"], outs["commit"])  # the 32-byte record carries a (pre-)campaign's lastTerm there
    camp["flags"] = outs["flags"] | np.where(asks, OUTF_ANSWERED, 0).astype(np.uint8)
    recs = []
    for p in range(N):
        if p == me:
            continue
        w = np.zeros(len(built), W.WIRE_MSG_DT)
        w["group"], w["to"], w["from"] = built, p, me
        w["type"] = np.where(pre, MSG_PRE_VOTE, MSG_VOTE)
        w["term"] = outs["term"] + pre.astype(np.uint64)  # a pre-election asks at term + 1 and moves none
        w["index"], w["log_term"] = outs["index"], outs["log_term"]
        recs.append(w)
    w = np.concatenate(recs) if recs else np.zeros(0, W.WIRE_MSG_DT)
    if voters is None:
        keep = np.tile(asks, N - 1)
    else:
        keep = M._slots(voters, built, N, me, allowed=asks)
    return w, keep, camp, built, outs


def beats_round(st, voters, beats, beat_cap):
    """the heartbeat section -> (every positional record, keep [slots] bool, peer_off [N + 1])"""
    from tests import test_tick_frames_gpu as TF

    if voters is None:
        w, po = TF.want_frames(st, beats, beat_cap)
        return w, np.ones(len(w), bool), po
    return M.member_beats(st, voters, beats, beat_cap)


def round_(st, active, lead_elapsed, voters, hb, tick_no, hup_cap, beat_cap, pre_vote, et=ET, seed=SEED, plain_hup=False):
    """one fused call (the state MOVES) -> dict: act, hups / beats / checks (all of them, u32 ascending), camp, built, outs (the raw
    results), w / keep (both sections' positional records), po [2 (N + 1)], stream, off (positional, [n_max + 1]), n_max, frames"""
    N, me = st.N, st.self_peer
    act = tick(st, active, lead_elapsed, voters, hb, tick_no, et, seed)
    hups, beats, checks = (np.flatnonzero(act == a).astype(np.uint32) for a in (1, 2, 3))
    bw, bkeep, bpo = beats_round(st, voters, beats, beat_cap)  # (led groups and campaigning groups are disjoint)
    vw, vkeep, camp, built, outs = campaigns(st, active, lead_elapsed, voters, hups, hup_cap, pre_vote, et, plain_hup)
    w, keep = np.concatenate([bw, vw]), np.concatenate([bkeep, vkeep])
    po = np.zeros(2 * (N + 1), np.uint64)
    po[: N + 1] = bpo
    po[N + 1] = bpo[N]
    po[N + 2:] = bpo[N] + np.cumsum([0 if p == me else len(built) for p in range(N)]).astype(np.uint64)
    n_max = (beat_cap + hup_cap) * (N - 1)  # the slots frame_off has room for
    stream, off = M.encode_members(w, keep, n_max)
    return dict(act=act, hups=hups, beats=beats, checks=checks, camp=camp, built=built, outs=outs, w=w, keep=keep, po=po, stream=stream, off=off,
                n_max=n_max, frames=int(keep.sum()), n_beat_built=min(len(beats), beat_cap))


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------------------
MODES = ("cq", "cq_pv", "cq_masks", "cq_pv_masks")
GS = (1, 129, 3149)
NS = (2, 3, 5)


def _one(n, me, role, rng):
    """one group in a plausible state of the given role (0 follower, 1 candidate, 2 leader)"""
    s = pyoracle.NodeState(1, n, me)
    s.role[0] = role
    s.term[0], s.last_index[0], s.last_term[0], s.committed[0] = rng.integers(2, 300), rng.integers(20, 40000), 1, 12
    s.last_term[0] = s.term[0] - (0 if role == 2 else 1)
    for p in range(n):
        s.match[p, 0] = rng.integers(0, 20) if role == 2 else 0
    s.match[me, 0] = s.last_index[0]
    if role == 2:
        s.first_idx[0], s.lead[0], s.vote[0] = 1, me + 1, me + 1
    elif role == 1:
        s.vote[0], s.votes[me, 0] = me + 1, 1
    else:
        s.vote[0] = rng.integers(0, n + 1)
    return s


def _single_scenes(mode, n, me, rng):
    """G = 1: one planted group per thing a case must show, each its own scene"""
    pv, masks = "pv" in mode, "masks" in mode
    full = (1 << n) - 1
    rows = [  # role, elapsed, active, lead_elapsed, mask, hb
        (2, 0, full, ET - 1, full, 1),            # a check due at once: passes, the bits are cleared, the beat goes out
        (2, 0, 0, ET - 2, full, 1),               # due on the second tick: fails, action 3, no beat
        (2, 1, full, ET - 3, full, 3),            # heartbeat_tick 3: the beat and the check fall on different ticks
        (0, 2 * ET - 1, 0, 0, full, 1),           # the timer fires at once, and again behind the campaign's reset
        (1, 2 * ET - 2, 0, 0, full, 3),           # a candidate whose timer fires: campaigns again (PreVote: turns pre-candidate)
    ]
    if masks:
        rows += [(0, 2 * ET - 1, 0, 0, 1 << me, 1),                           # self is the only voter: wins at once
                 (2, 0, 0, ET - 1, 1 << me, 1),                               # a leader nobody else is a member of: no frame, the check passes
                 (0, 2 * ET - 1, 0, 0, full & ~(1 << ((me + 1) % n)), 1),     # a peer that is no member is not asked
                 (0, 2 * ET - 1, 0, 0, full & ~(1 << me), 1)]                 # self does not vote: never campaigns
    scenes = []
    for role, el, ac, le, mask, hb in rows:
        st = _one(n, me, role, rng)
        st.elapsed[0] = el
        scenes.append(dict(st=st, active=np.array([ac], np.uint16), lead_elapsed=np.array([le], np.uint32),
                           voters=np.array([mask], np.uint16) if masks else None, hb=hb, pre_vote=pv))
    return scenes


def _random_scene(mode, g, n, me, hb, rng, wide64=False):
    """wide64: test_tick_frames_gpu.make_state's terms and indices in [2^62, 2^64), group 0 a leader at term 2^64 - 1 (no scene
    campaigns from the top term)"""
    from tests import test_tick_elect_gpu as TE

    pv, masks = "pv" in mode, "masks" in mode
    full = (1 << n) - 1
    st = TE.make_state(rng, g, n, me, hb, wide64)
    assert not wide64 or (int(st.role[0]) == 2 and int(st.term[0]) == 2**64 - 1)
    if pv:  # some of the candidates are pre-candidates already
        cand = np.flatnonzero(st.role == 1)
        st.role[cand[::3]] = PV.PRE
    active = np.where(rng.random(g) < 0.3, 0, np.where(rng.random(g) < 0.3, full, rng.integers(0, full + 1, g))).astype(np.uint16)
    lead_elapsed = rng.integers(0, ET, g).astype(np.uint32)  # (three in ten fall due within the three ticks)
    voters = None
    if masks:
        voters = V.random_masks(rng, n, g)
        voters[rng.random(g) < 0.6] |= np.uint16(1 << me)
    lead = rng.permutation(np.flatnonzero(st.role == 2))
    free = rng.permutation(np.flatnonzero(st.role == 0))
    cand = rng.permutation(np.flatnonzero(st.role == 1))
    assert len(lead) >= 4 and len(free) >= 4 and len(cand) >= 1, (len(lead), len(free), len(cand))
    # planted: a passing and a failing check within the three ticks, a timer that fires, a candidate whose timer fires
    active[lead[0]], lead_elapsed[lead[0]] = full, ET - 1
    active[lead[1]], lead_elapsed[lead[1]] = 0, ET - 2
    st.elapsed[free[0]] = 2 * ET - 1
    st.elapsed[cand[0]] = 2 * ET - 1
    if masks:
        voters[lead[:2]] = full
        voters[free[0]] = full & ~(1 << ((me + 1) % n)) if n > 2 else full
        voters[cand[0]] = full
        voters[free[1]], st.elapsed[free[1]] = 1 << me, 2 * ET - 1         # the only voter: wins at once
        voters[lead[2]], lead_elapsed[lead[2]] = 1 << me, ET - 1           # a leader without members: fillers only, its check passes
        voters[lead[3]] = 0                                                 # an unused slot that leads by role: its check fails
        lead_elapsed[lead[3]] = ET - 1
        voters[free[2]], st.elapsed[free[2]] = full & ~(1 << me), 2 * ET - 1  # self does not vote: never campaigns
    return dict(st=st, active=active, lead_elapsed=lead_elapsed, voters=voters, hb=hb, pre_vote=pv)


def _self_of(mode, g, n):
    return (MODES.index(mode) + g + n) % n


@functools.lru_cache(maxsize=None)
def scenes(mode, g, n, wide64=False):
    """the scenes of one GPU case, never changed: each a start state (st, active, lead_elapsed, voters | None, hb, pre_vote) that the
    test runs TICKS fused calls on.  G = 1: one planted group per scene; else one random scene per heartbeat_tick.  wide64 (a
    case's fourth word, G > 1): 64-bit terms and indices"""
    me = _self_of(mode, g, n)
    rng = np.random.default_rng(28000 + 1000 * MODES.index(mode) + 16 * n + g + (500 if wide64 else 0))
    if g == 1:
        assert not wide64
        return tuple(_single_scenes(mode, n, me, rng))
    return tuple(_random_scene(mode, g, n, me, hb, rng, bool(wide64)) for hb in (1, 3))


def case_list():
    """(mode, G, N) of every case tests/test_tick_checks_gpu.py runs: the four switch settings over every shape, N = 9 once; then
    (mode, G, N, "wide64"): the device-built MsgPreVote and MsgVote rounds at term + 1 with every term and index above 2^62"""
    cases = [(mode, g, n) for mode in MODES for g in GS for n in NS]
    cases.append(("cq_pv_masks", 3149, 9))
    cases += [("cq_pv", 129, 3, "wide64"), ("cq_pv_masks", 129, 5, "wide64")]
    return cases


def play(scene, hup_cap=None, beat_cap=None, plain_hup=False, ticks=TICKS):
    """the reference alone on a copy of the scene -> [round_() dict per tick] with the state behind each call in 'after'"""
    st, active, lead_elapsed = copy_case(scene["st"], scene["active"], scene["lead_elapsed"])
    g = st.G
    out = []
    for t in range(ticks):
        before = copy_case(st, active, lead_elapsed)
        r = round_(st, active, lead_elapsed, scene["voters"], scene["hb"], t, g if hup_cap is None else hup_cap, g if beat_cap is None else beat_cap,
                   scene["pre_vote"], plain_hup=plain_hup)
        r["before"], r["after"] = before, copy_case(st, active, lead_elapsed)
        out.append(r)
    return out


def shows(case):
    """what a case's inputs show of the feature, read off the reference alone -> dict of counts over all its scenes and ticks"""
    mode, g, n = case[:3]
    c = dict(passed=0, failed=0, failed_beats=0, hups=0, beats=0, pre_kept_term=0, cand_to_pre=0, solo_wins=0, empty_slots=0, campaigns=0)
    for scene in scenes(*case):
        me = scene["st"].self_peer
        for r in play(scene):
            (s0, a0, le0), (s1, a1, le1) = r["before"], r["after"]
            lead = s0.role == 2
            due = lead & (le0 + 1 >= ET)
            failed = r["act"] == 3
            c["passed"] += int((due & ~failed & (a0 != 0) & (a1 == 0)).sum())
            c["failed"] += int((due & failed).sum())
            assert not (failed & ~due).any()
            # a failed check's group is in no heartbeat frame
            beat_groups = set(r["w"]["group"][: r["n_beat_built"] * (n - 1)].tolist())
            c["failed_beats"] += len(beat_groups & set(np.flatnonzero(failed).tolist()))
            c["hups"] += len(r["hups"])
            c["beats"] += len(r["beats"])
            b = r["built"]
            pre = r["outs"]["type"] == OUT_PRE_CAMPAIGN
            c["pre_kept_term"] += int((pre & (s1.term[b] == s0.term[b]) & (s1.role[b] == PV.PRE)).sum())
            c["cand_to_pre"] += int((pre & (s0.role[b] == 1)).sum())
            c["campaigns"] += int((r["outs"]["type"] == OUT_CAMPAIGN).sum())
            c["solo_wins"] += int((r["outs"]["type"] == OUT_BECAME_LEADER).sum())
            c["empty_slots"] += int((~r["keep"]).sum())
    return c
