"""CPU: the yardstick of Step with forwarded proposals (tests/ref_step_props.py) is itself checked against things this feature
did not write.

1. On traffic without MsgProp its driver IS the C oracle: result records and state, byte for byte (and, with masks, IS
   tests/ref_step_voters.py).
2. On a leader, stepping a MsgProp of n entries leaves exactly the state the C oracle's tail report {last_index + n, term, 0}
   leaves -- appendEntry's bookkeeping is the one raftq_apply_log_deltas has always done -- for N = 1..9, and with masks the
   state tests/ref_step_voters.apply_log_deltas leaves.
3. A hand table written from the upstream rules (include/raftq_step.h) gives the table's answers.
4. Every generated batch the GPU tests step can tell the feature from its absence (ref_step_props.FLOORS), asserted on the
   reference's own output."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _stepgen
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

CASES, FRAMES = P.case_list()


def _same_state(a, b):
    for k, _ in a.FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.match, b.match) and np.array_equal(a.votes, b.votes)


@pytest.mark.parametrize("hot", [False, True], ids=["spread", "hot"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9])
def test_without_msgprop_it_is_the_c_oracle(oracle, n, hot):
    rng = np.random.default_rng(9100 + 2 * n + hot)
    g = 200
    s = _stepgen.random_state(rng, g, n, n // 2)
    mine, masked = V.copy_state(s), V.copy_state(s)
    hot_groups = rng.permutation(g)[:6] if hot else None
    for rnd in range(3):
        m = _stepgen.random_batch(rng, s, 500, hot_groups)
        if rnd == 1:
            m = _stepgen.with_hold_skip(rng, m)  # (a held record of type 2 is not looked at: HOLD wins over the type)
        want = s.step_batch(m)
        assert P.step_batch(mine, None, m).tobytes() == want.tobytes()
        assert P.step_batch(masked, V.full_masks(n, g), m).tobytes() == want.tobytes()
        _same_state(mine, s)
        _same_state(masked, s)


@pytest.mark.parametrize("n", range(1, 10))
def test_a_leaders_msgprop_is_the_c_oracles_tail_report(oracle, n):
    rng = np.random.default_rng(9150 + n)
    g, me = 300, n // 2
    s = P.props_state(rng, n, me, g)
    led = np.flatnonzero(s.role == 2)
    assert len(led) > 50
    k = rng.integers(1, 5, len(led)).astype(np.uint64)
    m = np.zeros(len(led), pyoracle.STEP_MSG_DT)
    for i, grp in enumerate(led):
        P._prop(m, i, grp, int(k[i]), frm=int(rng.integers(0, n)))
    mine, masked, masked_ref = V.copy_state(s), V.copy_state(s), V.copy_state(s)
    before = s.last_index[led].copy()
    committed = s.apply_log_deltas(led.astype(np.uint64), before + k, s.term[led], np.zeros(len(led), np.uint64))
    out = P.step_batch(mine, None, m)
    _same_state(mine, s)
    assert (out["type"] == P.OutProposed).all() and np.array_equal(out["index"], before + 1) and np.array_equal(out["log_term"], s.term[led])
    assert np.array_equal(out["last_index"], before + k) and np.array_equal(out["commit"], committed)
    moved = (out["flags"] & R.FlagCommitted) != 0
    assert moved.sum() >= P.PLANT and (n > 1 or moved.all())  # (N = 1: the leader is its own quorum)
    assert np.array_equal((out["flags"] & R.FlagHardState) != 0, moved) and (out["to"] == m["from"]).all()
    # ... and over each group's own voters, the masked tail report
    voters = V.random_masks(rng, n, g)
    V.apply_log_deltas(masked_ref, voters, led.astype(np.uint64), before + k, s.term[led])
    P.step_batch(masked, voters, m)
    _same_state(masked, masked_ref)


def _table():
    """one group per row: N = 3 (row 4: N = 1 is its own test), self = slot 0, term 5, the log ends at (10, 4), commit 7, the
    followers' Match 8 and 6, first_idx 9.  (role, lead, [messages (type, term, from, index, n)], [want (type, to, index,
    log_term, commit, last_index, flags, role after, lead after)])"""
    P_, A = P.MsgProp, R.MsgAppResp
    H, C, U_ = R.FlagHardState, R.FlagCommitted, R.FlagUpdated
    return [
        ("leader", 2, 1, [(P_, 0, 1, 0, 3)], [(12, 1, 11, 5, 7, 13, 0, 2, 1)]),
        ("follower with a leader", 0, 3, [(P_, 0, 1, 0, 2)], [(13, 2, 0, 0, 7, 10, 0, 0, 3)]),
        ("follower without a leader", 0, 0, [(P_, 0, 1, 0, 2)], [(0, 1, 0, 0, 7, 10, 0, 0, 0)]),
        ("candidate", 1, 0, [(P_, 0, 1, 0, 2)], [(0, 1, 0, 0, 7, 10, 0, 1, 0)]),
        ("a higher term: follower of the sender, then forwarded to it", 2, 1, [(P_, 6, 2, 0, 1)], [(13, 2, 0, 0, 7, 10, H | 8, 0, 3)]),
        ("a stale term: ignored", 2, 1, [(P_, 4, 1, 0, 1)], [(0, 1, 0, 0, 7, 10, 0, 2, 1)]),
        # an ack for 12 behind a proposal of three: 12 lies between the old tail (10) and the new one (13) -- min(m.index,
        # lastIndex) keeps it, slot 1's Match is 12, the quorum holds 12: committed.  Without the append it would be clamped to 10.
        ("a proposal, then an ack inside the new entries", 2, 1, [(P_, 0, 1, 0, 3), (A, 5, 1, 12, 0)],
         [(12, 1, 11, 5, 7, 13, 0, 2, 1), (5, 1, 12, 0, 12, 13, H | C | U_, 2, 1)]),
        ("two proposals in one batch", 2, 1, [(P_, 0, 1, 0, 2), (P_, 0, 2, 0, 4)], [(12, 1, 11, 5, 7, 12, 0, 2, 1), (12, 2, 13, 5, 7, 16, 0, 2, 1)]),
    ]


def _table_state(rows, n=3):
    s = pyoracle.NodeState(len(rows), n, 0)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:] = 5, 10, 4, 7
    s.match[0] = 10
    for g, (_, role, lead, _, _) in enumerate(rows):
        s.role[g], s.lead[g] = role, lead
        if role == 2:
            s.first_idx[g], s.vote[g] = 9, 1
            if n > 1:
                s.match[1, g], s.match[2, g] = 8, 6
        if role == 1:
            s.vote[g], s.votes[0, g] = 1, 1
    return s


def table_batch():
    """-> (NodeState, msgs, want rows) of the hand table"""
    rows = _table()
    s = _table_state(rows)
    recs, want = [], []
    for g, (_, _, _, msgs, wants) in enumerate(rows):
        for (t, term, frm, index, k), w in zip(msgs, wants):
            recs.append((g, t, term, frm, index, k))
            want.append(w)
    m = np.zeros(len(recs), pyoracle.STEP_MSG_DT)
    for i, (g, t, term, frm, index, k) in enumerate(recs):
        m["group"][i], m["type"][i], m["term"][i], m["from"][i], m["index"][i] = g, t, term, frm, index
        if t == P.MsgProp:
            m["_pad"][i][1], m["_resv"][i] = V.MSGF_ENTRIES, k
    return s, m, want


def check_table(out, want):
    for i, w in enumerate(want):
        o = out[i]
        got = tuple(int(o[k]) for k in ("type", "to", "index", "log_term", "commit", "last_index", "flags", "role", "lead"))
        assert got == w, (i, got, w)


def test_hand_table():
    s, m, want = table_batch()
    check_table(P.step_batch(s, None, m), want)
    assert [int(x) for x in s.last_index] == [13, 10, 10, 10, 10, 10, 13, 16]
    assert int(s.last_term[0]) == 5 and int(s.match[0, 0]) == 13 and int(s.committed[6]) == 12 and int(s.match[1, 6]) == 12


def test_hand_table_n1_commits_on_its_own_proposal():
    s = pyoracle.NodeState(1, 1, 0)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:], s.role[:], s.lead[:], s.vote[:], s.first_idx[:] = 5, 10, 5, 10, 2, 1, 1, 3
    s.match[0] = 10
    m = np.zeros(1, pyoracle.STEP_MSG_DT)
    P._prop(m, 0, 0, 2)
    o = P.step_batch(s, None, m)[0]
    assert (int(o["type"]), int(o["index"]), int(o["commit"]), int(o["last_index"]), int(o["flags"])) == (12, 11, 12, 12, R.FlagHardState | R.FlagCommitted)


def test_malformed_records_fail_the_batch():
    s, m, _ = table_batch()
    for what, change in (("no flag", lambda r: r["_pad"].__setitem__(1, 0)), ("no entries", lambda r: r.__setitem__("_resv", 7 << 32)),
                         ("from", lambda r: r.__setitem__("from", 3))):
        bad = m.copy()
        change(bad[0])
        before = V.copy_state(s)
        with pytest.raises(ValueError):
            P.step_batch(s, None, bad)
        _same_state(s, before)


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_every_record_case_tells_the_feature_from_its_absence(oracle, kw):
    start, voters, m, want, _ = P.case(**kw)
    got = P.assert_discriminates(start, voters, m, want, kw)
    print(kw, got)
    counts = np.unique(m["group"], return_counts=True)[1]
    assert (counts.max() > 32) == bool(kw.get("hot")), counts.max()  # the stall and the replay run where they are meant to, only there
    assert not P.malformed(m, start.G, start.N).any()


@pytest.mark.parametrize("kw", FRAMES, ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_every_frames_case_tells_the_feature_from_its_absence(oracle, kw):
    s, stream, off, wm, we, by_switch = P.frames_case(**kw)
    want_m, rec, want_o, _ = by_switch[True]
    got = P.assert_discriminates(s, None, rec, want_o, kw)
    print(kw, got)
    empty = (wm["type"] == P.MsgProp) & (wm["n_ents"] == 0)
    assert empty.sum() >= 8 and (want_o["type"][empty] == V.OutSkipped).all()  # "some of them empty"
    # the switch-off form of the same frames: every MsgProp held, whatever it carries, and records wait behind it
    off_o = by_switch[False][2]
    assert (off_o["type"][wm["type"] == P.MsgProp] == V.OutHeld).all() and (off_o["type"] == R.OutDeferred).sum() >= 8
    assert not np.isin(off_o["type"], (P.OutProposed, P.OutForward)).any()
