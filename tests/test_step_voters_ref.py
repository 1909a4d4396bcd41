"""CPU: the yardstick of the masked Step (tests/ref_step_voters.py) is itself checked, three ways.

1. With every mask full its driver IS the C oracle: result records and state, byte for byte, on random traffic.
2. On the directed commit input its commit indices are the array-shaped statement's (tests/ref_voters.commit_advance over the
   Match rows after the batch) -- in every group whose acknowledgement moved a Match.  Step, like upstream, runs maybeCommit only
   when Progress.maybeUpdate returned true; the sweep evaluates every group.  In a group whose ack moved nothing (the sender is
   self, or a non-voter already at the tail, or a voter that was there: 28-53 % of the groups) Step leaves the commit index
   alone, and that is asserted instead.
3. The directed inputs discriminate: the share of groups in which the masks change the outcome is above the floor set for it.
   For the commit input the share is read off the array-shaped statement (masks against full masks over the same rows after
   the batch), which is how the floors were derived; the share of groups in which STEP's own commit index differs is smaller,
   because of (2) -- measured with these generators at G = 3,149: 0.30-0.51 for N >= 3, 0.07 for N = 2 and 0 for N = 1 (slot
   0 is self and holds the tail: no ack moves its Match).  The one-voter cases of tests/test_step_voters_gpu.py cover N = 1."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _stepgen
from tests import ref_step_voters as V
from tests import ref_voters as RV

G0 = 3149
SHAPES = ((1, 0), (2, 1), (3, 0), (5, 4), (8, 2), (9, 8))


def _same_state(a, b):
    for k, _ in a.FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.match, b.match) and np.array_equal(a.votes, b.votes)


@pytest.mark.parametrize("hot", [False, True], ids=["spread", "hot"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9])
def test_full_masks_are_the_c_oracle(oracle, n, hot):
    rng = np.random.default_rng(8100 + 2 * n + hot)
    g = 200
    s = _stepgen.random_state(rng, g, n, n // 2)
    mine = V.copy_state(s)
    full = V.full_masks(n, g)
    hot_groups = rng.permutation(g)[:6] if hot else None
    for _ in range(3):
        m = _stepgen.random_batch(rng, s, 500, hot_groups)
        assert V.step_batch(mine, full, m).tobytes() == s.step_batch(m).tobytes()
        _same_state(mine, s)
        led = np.flatnonzero(s.role == 2)[:40]
        tail = s.last_index[led] + rng.integers(0, 3, len(led)).astype(np.uint64)
        fol = np.flatnonzero(s.role == 0)[:40]
        gr = np.concatenate([led, fol, led[:5]]).astype(np.uint64)  # (a group twice: records apply in order)
        li = np.concatenate([tail, s.last_index[fol] + 1, tail[:5] + 1])
        lt = np.concatenate([s.term[led], s.term[fol], s.term[led[:5]]])
        ct = np.concatenate([np.zeros(len(led), np.uint64), s.last_index[fol], np.zeros(len(led[:5]), np.uint64)])
        assert np.array_equal(V.apply_log_deltas(mine, full, gr, li, lt, ct), s.apply_log_deltas(gr, li, lt, ct))
        _same_state(mine, s)


@pytest.mark.parametrize("n,self_peer", SHAPES)
def test_commit_input_agrees_with_the_array_shaped_statement(n, self_peer):
    s, voters, m = V.commit_input(n, self_peer, G0, 8200 + n)
    a = V.copy_state(s)
    out = V.step_batch(a, voters, m)
    want, _ = RV.commit_advance(a.match, s.committed, voters, True, s.first_idx)
    moved = (out["flags"] & 4) != 0  # RAFTQ_OUTF_UPDATED: Progress.maybeUpdate returned true, so maybeCommit ran
    assert np.array_equal(a.committed[moved], want[moved])
    assert np.array_equal(a.committed[~moved], s.committed[~moved])
    assert n == 1 or moved.mean() > 0.4
    # non-voters' words are stored as always: the ack of a non-voter below the tail moved its Match
    bits = RV.member_bits(voters, n)
    frm = m["from"].astype(np.int64)
    outsider = ~bits[frm, np.arange(G0)] & moved
    assert n == 1 or outsider.any()
    assert np.array_equal(a.match[frm[outsider], np.flatnonzero(outsider)], m["index"][outsider])


def _array_shaped_share(n, self_peer, seed):
    s, voters, m = V.commit_input(n, self_peer, G0, seed)
    a = V.copy_state(s)
    V.step_batch(a, voters, m)
    masked, _ = RV.commit_advance(a.match, s.committed, voters, True, s.first_idx)
    full, _ = RV.commit_advance(a.match, s.committed, V.full_masks(n, G0), True, s.first_idx)
    return float((masked != full).mean())


@pytest.mark.parametrize("n,self_peer", SHAPES)
def test_the_directed_inputs_discriminate(n, self_peer):
    share = _array_shaped_share(n, self_peer, 8300 + n)
    print("commit input, N = %d: %.3f of the groups differ (array-shaped); %.3f in Step's own commit index" %
          (n, share, V.discrimination("commit", n, self_peer, G0, 8300 + n)))
    assert share >= V.floor_for("commit", n), (n, share)
    share = V.discrimination("election", n, self_peer, G0, 8400 + n)
    print("election input, N = %d: %.3f of the groups end in another role" % (n, share))
    assert share >= V.floor_for("election", n), (n, share)


def test_masked_rules_by_hand():
    """five slots, self = slot 0, one group per row: the rules of include/raftq_step.h, each on the smallest case that shows it"""
    def one(role, mask, votes=(0,) * 5, match=(0,) * 5, msg=None, **kw):
        s = pyoracle.NodeState(1, 5, 0)
        s.role[0], s.term[0], s.last_index[0], s.last_term[0] = role, 3, 5, 2
        s.vote[0] = 1 if role else 0
        s.votes[:, 0], s.match[:, 0] = votes, match
        for k, v in kw.items():
            getattr(s, k)[0] = v
        m = np.zeros(1, dtype=pyoracle.STEP_MSG_DT)
        m["type"], m["term"], m["from"], m["index"], m["reject"] = msg
        out = V.step_batch(s, np.array([mask], np.uint16), m)
        return s, out[0]

    # MsgHup where self does not vote: the own grant is recorded, not counted -> a campaign, never a win
    s, o = one(0, 0b00110, msg=(0, 0, 0, 0, 0))
    assert o["type"] == 3 and s.role[0] == 1 and s.votes[0, 0] == 1 and s.term[0] == 4
    # ... and with the mask {self}: q_g = 1, the own grant wins; the empty entry commits on its own
    s, o = one(0, 0b00001, msg=(0, 0, 0, 0, 0))
    assert o["type"] == 4 and s.role[0] == 2 and s.committed[0] == 6 and s.last_index[0] == 6
    # an empty mask: q_g = 1 and nothing counts
    s, o = one(0, 0, msg=(0, 0, 0, 0, 0))
    assert o["type"] == 3 and s.role[0] == 1
    # a non-voter's grant does not win (three voters, one grant so far) but is recorded ...
    s, o = one(1, 0b00111, votes=(1, 0, 0, 0, 0), msg=(6, 3, 4, 0, 0))
    assert s.role[0] == 1 and s.votes[4, 0] == 1
    # ... a voter's does: granted == q_g = 2
    s, o = one(1, 0b00111, votes=(1, 0, 0, 1, 1), msg=(6, 3, 1, 0, 0))
    assert o["type"] == 4 and s.role[0] == 2
    # rejections count over the voters too: two of three voters reject -> follower; the non-voters' rejections did not
    s, o = one(1, 0b00111, votes=(1, 2, 0, 2, 2), msg=(6, 3, 2, 0, 1))
    assert s.role[0] == 0 and (o["flags"] & 8)
    s, o = one(1, 0b00111, votes=(1, 0, 0, 2, 2), msg=(6, 3, 2, 0, 1))
    assert s.role[0] == 1
    # an ack from a non-voter moves its Match, sets RAFTQ_OUTF_UPDATED and commits nothing
    s, o = one(2, 0b00111, match=(5, 0, 0, 0, 0), msg=(4, 3, 4, 5, 0), first_idx=1, lead=1)
    assert s.match[4, 0] == 5 and (o["flags"] & 4) and s.committed[0] == 0
    # ... a voter's reaches q_g = 2 of {0, 1, 2}
    s, o = one(2, 0b00111, match=(5, 0, 0, 5, 5), msg=(4, 3, 1, 4, 0), first_idx=1, lead=1)
    assert s.committed[0] == 4 and (o["flags"] & 2)
