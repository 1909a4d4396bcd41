"""CPU: the yardstick of the masked Tick and its rounds (tests/ref_tick_members.py) is itself checked.

The Tick is stated twice there -- array-shaped on oracle.pyoracle.tick, and as a per-group loop that restates upstream's
tickElection / tickHeartbeat with promotable() -- and the two must agree: N = 1 .. 9, G = 2,500, 20 consecutive ticks, masks from
ref_step_voters.random_masks with the empty mask, the full mask, {self} alone and self-absent added by hand.  Then the
properties the issue names, and the round builders on a small hand-made input."""
import numpy as np
import pytest

from oracle import pywire as W
from tests import ref_step_voters as V
from tests import ref_tick_members as M

G, ET, SEED, TICKS = 2500, 10, 0x7157, 20


def _input(n, hb, seed):
    rng = np.random.default_rng(seed)
    me = int(rng.integers(0, n))
    role = rng.choice([0, 1, 2], G).astype(np.uint8)
    elapsed = np.where(role == 2, rng.integers(0, hb, G), rng.integers(0, 2 * ET, G)).astype(np.uint32)
    voters = V.random_masks(rng, n, G)
    hand = M.hand_masks(n, me)
    for r in (0, 1, 2):  # every hand-made mask under every role
        at = np.flatnonzero(role == r)[: len(hand)]
        voters[at] = hand
    return me, role, elapsed, voters


@pytest.mark.parametrize("hb", [1, 3])
@pytest.mark.parametrize("n", range(1, 10))
def test_the_two_statements_agree(oracle, n, hb):
    me, role, elapsed, voters = _input(n, hb, 13100 + 10 * n + hb)
    mine = M.mine_of(voters, me)
    free = role != 2
    assert (free & ~mine).sum() > 100 and (free & mine).sum() > 100, "both kinds of non-leader groups are there"
    a_el, s_el, plain_el = elapsed.copy(), elapsed.copy(), elapsed.copy()
    hups = 0
    for t in range(TICKS):
        a = M.tick_array(oracle, role, a_el, voters, me, ET, hb, SEED, t)
        s = M.tick_scalar(oracle, role, s_el, voters, me, ET, hb, SEED, t)
        assert np.array_equal(a[0], s[0]) and np.array_equal(a[1], s[1]) and a[2:] == s[2:], (n, hb, t)
        a_el, s_el = a[0], s[0]
        # a non-promotable group never raises MsgHup, and its elapsed is 0
        idle = free & ~mine
        assert not (a[1][idle] != 0).any() and not a_el[idle].any()
        # leaders equal the unmasked result
        p_el, p_act, _, p_beat = oracle.tick(role, plain_el, ET, hb, SEED, t)
        assert np.array_equal(a[1][~free], p_act[~free]) and np.array_equal(a_el[~free], p_el[~free]) and a[3] == p_beat
        # ... and so does a promotable group, whose timer the masks never touched
        assert np.array_equal(a[1][free & mine], p_act[free & mine]) and np.array_equal(a_el[free & mine], p_el[free & mine])
        plain_el = p_el
        hups += a[2]
    assert hups > 100, "timers were meant to fire"


@pytest.mark.parametrize("n", range(1, 10))
def test_full_masks_are_the_oracle_bit_for_bit(oracle, n):
    me, role, elapsed, _ = _input(n, 1, 13300 + n)
    full = V.full_masks(n, G)
    el = elapsed.copy()
    for t in range(TICKS):
        want = oracle.tick(role, el, ET, 1, SEED, t)
        for got in (M.tick_array(oracle, role, el, full, me, ET, 1, SEED, t), M.tick_scalar(oracle, role, el, full, me, ET, 1, SEED, t)):
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:]
        el = want[0]


def test_encode_members_spreads_the_dense_offsets():
    """five slots, members at 0, 2 and 3: the positional offsets repeat where a slot has no bytes and end on the total"""
    w = np.zeros(5, W.WIRE_MSG_DT)
    w["group"], w["type"], w["to"], w["from"], w["term"] = np.arange(5), 8, 1, 0, [1, 2, 300, 4, 5]
    keep = np.array([True, False, True, True, False])
    stream, off = M.encode_members(w, keep, 7)
    want_s, dense = W.wire_encode(w[keep])
    assert bytes(stream) == bytes(want_s) and len(off) == 8
    assert list(off) == [dense[0], dense[1], dense[1], dense[2], dense[3], dense[3], dense[3], dense[3]]
    none_s, none_off = M.encode_members(w, np.zeros(5, bool), 5)
    assert len(none_s) == 0 and not none_off.any()


def test_member_campaigns_take_both_arms(oracle):
    """a group whose only voter is self becomes leader (no ANSWERED, every vote slot empty); any other promotable group campaigns
    and asks its members only"""
    from oracle import pyoracle

    n, me = 3, 1
    st = pyoracle.NodeState(4, n, me)
    st.term[:], st.last_index[:], st.last_term[:] = 4, 9, 3
    st.match[me] = 9
    voters = np.array([0b010, 0b111, 0b011, 0b110], np.uint16)
    w, keep, camp, built, outs = M.member_campaigns(st, voters, np.arange(4), 4)
    assert list(camp["type"]) == [M.OUT_BECAME_LEADER, M.OUT_CAMPAIGN, M.OUT_CAMPAIGN, M.OUT_CAMPAIGN]
    assert camp["flags"][0] & M.OUTF_HARDSTATE and not camp["flags"][0] & M.OUTF_ANSWERED
    assert (camp["flags"][1:] == (M.OUTF_HARDSTATE | M.OUTF_ANSWERED)).all()
    assert int(camp["index"][0]) == 10 and int(st.role[0]) == 2 and (st.role[1:] == 1).all() and (st.term == 5).all()
    assert (camp["commit"][1:] == 3).all()  # a campaign's lastTerm
    # slots, peer-major: peer 0 for groups 0..3, then peer 2
    assert list(keep) == [False, True, True, False, False, True, False, True]
    assert len(w) == 8 and (w["type"] == M.MSG_VOTE).all() and (w["term"] == 5).all()
