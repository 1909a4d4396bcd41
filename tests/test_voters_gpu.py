"""GPU: per-group voter sets (include/raftq.h "per-group voter sets") against tests/ref_voters.py, whole arrays, bit for
bit.  Shapes are the smallest that reach every index path of sweep_voters_kernel: 3149 groups = several 1,024-group tiles
and a ragged last one (the handle pads to 4096), 129 = across one 128-group round of a wave, 1 = a single group."""
import numpy as np
import pytest

from raftsql_amd._lib import (CYCLE_SEGMENTED, RAFTQ_EINVAL, RAFTQ_ESTATE, SWEEP_CACHED, SWEEP_CHANGED, SWEEP_COMMIT, SWEEP_GATED,
                              SWEEP_LDS, SWEEP_NO_ADOPT, SWEEP_STREAM, SWEEP_VOTES)
from raftsql_amd.engine import RaftqError, SweepSet
from tests import ref_voters as R

pytestmark = pytest.mark.gpu

SHAPES = (3149, 129, 1)
G0 = SHAPES[0]


class State:
    """inputs of one handle: match / votes [N, G], committed / cur_term / first_idx / voters [G]"""

    def __init__(self, n, g, seed, leak=True):
        rng = np.random.default_rng(seed)
        self.n, self.g = n, g
        self.voters = rng.integers(0, 1 << n, g).astype(np.uint16)
        edge = np.array([0, (1 << n) - 1, 1, 1 << (n - 1), 0, (1 << n) - 1], np.uint16)  # empty, full, single-voter masks
        at = rng.permutation(g)[:min(g, edge.size)]
        self.voters[at] = edge[:at.size]
        bits = R.member_bits(self.voters, n)
        self.match = rng.integers(0, 8, (n, g)).astype(np.uint64)  # a small range: ties
        top = rng.random((n, g)) < 0.03
        self.match[top] = R.U64_MAX - rng.integers(0, 3, int(top.sum())).astype(np.uint64)
        self.votes = rng.integers(0, 3, (n, g)).astype(np.uint8)
        if leak:  # whatever a non-voter holds must not count: its Match is the largest value there is,
            self.match[~bits] = R.U64_MAX  # and it grants in one half of the groups and rejects in the other
            self.votes[~bits] = np.broadcast_to(np.where(np.arange(g) % 2 == 0, 1, 2).astype(np.uint8), (n, g))[~bits]
        self.committed = rng.integers(0, 5, g).astype(np.uint64)
        self.cur_term = rng.integers(0, 3, g).astype(np.uint64)
        self.first_idx = rng.integers(0, 7, g).astype(np.uint64)

    @property
    def gate(self):  # what the device holds: a group that never saw an election has no current-term entry
        return np.where(self.cur_term == 0, np.uint64(0), self.first_idx)

    def load(self, e, voters=True):
        e.load_match(self.match, self.committed)
        e.load_votes(self.votes)
        e.load_terms(self.cur_term, self.first_idx)
        if voters:
            e.load_voters(self.voters)
        return e


def _advances(old, new):
    g = np.flatnonzero(old != new)
    return g.astype(np.uint64), old[g], new[g]


def _same_list(adv, old, new):
    g, o, n = _advances(old, new)
    return np.array_equal(adv["group"], g) and np.array_equal(adv["old_commit"], o) and np.array_equal(adv["new_commit"], n)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("n", range(1, 10))
def test_commit_over_the_voters(gpu_engine_cls, n, gated):
    for k, g in enumerate(SHAPES):
        st = State(n, g, 7000 + 10 * n + k)
        want, n_changed = R.commit_advance(st.match, st.committed, st.voters, gated, st.gate)
        assert g < 100 or 0 < n_changed < g
        with st.load(gpu_engine_cls(g, n)) as e:
            policy = (0, SWEEP_STREAM, SWEEP_CACHED)[(n + k) % 3]
            c = e.sweep(SWEEP_COMMIT | (SWEEP_GATED if gated else 0) | SWEEP_CHANGED | SWEEP_NO_ADOPT | policy)
            assert np.array_equal(e.read_committed(), want) and c.n_changed == n_changed, (n, g)
            adv, total = e.collect_changed()
            assert total == n_changed and _same_list(adv, st.committed, want)
            got, changed = e.commit_advance(gated)  # raftq_commit_advance: the same sweep, adopted
            assert np.array_equal(got, want) and changed == n_changed
            assert np.array_equal(e.read_match(), st.match)  # non-voters' words are stored and read back as always
            # adopted: nothing is left to advance, and the commit index did not decrease
            again, changed = e.commit_advance(gated)
            assert np.array_equal(again, want) and changed == 0 and (want >= st.committed).all()


@pytest.mark.parametrize("n", range(1, 10))
def test_tally_over_the_voters(gpu_engine_cls, n):
    for k, g in enumerate(SHAPES):
        st = State(n, g, 7200 + 10 * n + k)
        want, won, lost = R.vote_tally(st.votes, st.voters)
        with st.load(gpu_engine_cls(g, n)) as e:
            out, c = e.vote_tally()
            assert np.array_equal(out, want) and (c.n_won, c.n_lost) == (won, lost), (n, g)
            assert np.array_equal(e.read_votes(), st.votes)
            # together with the commit part: one launch, both decisions
            cw, n_changed = R.commit_advance(st.match, st.committed, st.voters)
            c = e.sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_STREAM)
            assert (c.n_changed, c.n_won, c.n_lost) == (n_changed, won, lost)
            assert np.array_equal(e.read_committed(), cw) and np.array_equal(e.read_outcome(), want)


@pytest.mark.parametrize("n", range(1, 10))
def test_full_mask_everywhere_is_the_unmasked_path(gpu_engine_cls, oracle, n):
    st = State(n, G0, 7400 + n, leak=False)
    st.voters[:] = (1 << n) - 1
    with st.load(gpu_engine_cls(G0, n)) as a, st.load(gpu_engine_cls(G0, n), voters=False) as b:
        assert np.array_equal(a.read_voters(), st.voters) and np.array_equal(b.read_voters(), st.voters)
        for flags in (SWEEP_COMMIT | SWEEP_GATED | SWEEP_VOTES | SWEEP_CHANGED | SWEEP_NO_ADOPT, SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED):
            ca, cb = a.sweep(flags), b.sweep(flags)
            assert ca == cb
            assert np.array_equal(a.read_committed(), b.read_committed()) and np.array_equal(a.read_outcome(), b.read_outcome())
            la, lb = a.collect_changed(), b.collect_changed()
            assert la[1] == lb[1] and la[0].tobytes() == lb[0].tobytes()
        want, n_changed = oracle.commit_advance(st.match, st.committed)
        assert np.array_equal(a.read_committed(), want) and ca.n_changed == n_changed
        assert np.array_equal(a.read_outcome(), oracle.vote_tally(st.votes)[0])


@pytest.mark.parametrize("n", range(2, 10))
def test_self_row_that_is_no_voter(gpu_engine_cls, n):
    """Row 0 is every group's maximum, so the device knows it (raftq_self_max) and an unmasked sweep would leave the row
    out as "the largest of the N"; no mask names slot 0, and the result is the voters' alone."""
    st = State(n, G0, 7500 + n, leak=False)
    st.match[0] = st.match.max(axis=0)
    st.voters &= np.uint16(~1 & 0xffff)
    for gated in (False, True):
        want, n_changed = R.commit_advance(st.match, st.committed, st.voters, gated, st.gate)
        with st.load(gpu_engine_cls(G0, n)) as e:
            assert e.self_max() == 0
            got, changed = e.commit_advance(gated)
            assert np.array_equal(got, want) and changed == n_changed
            assert e.self_max() == 0


@pytest.mark.parametrize("n", [5, 9], ids=["16-bit-vote-words", "32-bit-vote-words"])
def test_voter_deltas(gpu_engine_cls, oracle, n):
    full = np.uint16((1 << n) - 1)
    st = State(n, G0, 7600 + n, leak=False)
    st.match[0] = st.match.max(axis=0)  # the self row is every group's largest: the device knows (raftq_self_max)
    rng = np.random.default_rng(7600 + n)
    with st.load(gpu_engine_cls(G0, n), voters=False) as e:
        assert (e.read_voters() == full).all() and e.self_max() == 0
        match, votes, voters, committed = st.match, st.votes, np.full(G0, full, np.uint16), st.committed

        def sweep_and_compare():
            nonlocal committed
            want, n_changed = R.commit_advance(match, committed, voters)
            got, changed = e.commit_advance(False)
            assert np.array_equal(got, want) and changed == n_changed and (want >= committed).all()
            out, c = e.vote_tally()
            assert np.array_equal(out, R.vote_tally(votes, voters)[0])
            committed = want

        def apply_and_compare(group, new_voters, reset):
            nonlocal match, votes, voters
            e.apply_voter_deltas(e.pack_voter_deltas(group, new_voters, reset))
            match, votes, voters = R.apply_voter_deltas(match, votes, voters, group, new_voters, reset)
            assert np.array_equal(e.read_match(), match) and np.array_equal(e.read_votes(), votes)
            assert np.array_equal(e.read_voters(), voters)

        # the first records arrive on a handle with no masks: they change "every slot votes".  No row is touched yet
        apply_and_compare(np.array([11, 2048], np.uint64), np.array([1, full - 1], np.uint16), np.zeros(2, np.uint16))
        assert e.self_max() == 0
        group = rng.integers(0, G0, 900).astype(np.uint64)  # 900 draws of 3149: groups repeat, the last record wins
        assert np.unique(group).size < group.size
        apply_and_compare(group, rng.integers(0, 1 << n, 900).astype(np.uint16), rng.integers(0, 1 << n, 900).astype(np.uint16))
        assert (voters[np.setdiff1d(np.arange(G0), np.append(group, [11, 2048]))] == full).all()
        assert e.self_max() == -1  # a zeroed entry of the self row may have ended the fact: the word is cleared
        sweep_and_compare()
        # a replica is removed in some groups; in others a slot is reused: added as a voter with its Match and vote reset
        gone = rng.permutation(G0)[:400].astype(np.uint64)
        slot = rng.integers(0, n, 400)
        apply_and_compare(gone, voters[gone] & ~(1 << slot).astype(np.uint16), np.zeros(400, np.uint16))
        back = rng.permutation(G0)[:400].astype(np.uint64)
        slot = rng.integers(0, n, 400)
        apply_and_compare(back, voters[back] | (1 << slot).astype(np.uint16), (1 << slot).astype(np.uint16))
        assert (match[slot, back] == 0).all() and (votes[slot, back] == 0).all()
        sweep_and_compare()
        # acks move on (only upwards) and the new replicas answer: the commit index follows, never backwards
        dg, dp = rng.integers(0, G0, 2000).astype(np.uint64), rng.integers(0, n, 2000).astype(np.uint32)
        dv = rng.integers(0, 12, 2000).astype(np.uint64)
        e.apply_deltas(dg, dp, dv)
        match = oracle.apply_deltas(match, dg, dp, dv)
        sweep_and_compare()
        # all-or-nothing: one bad record and nothing is applied
        good = np.array([5, 6], np.uint64)
        for bad_group, bad_voters, bad_reset in ((G0, 1, 0), (7, 1 << n, 0), (7, 1, 1 << n), (7, 0x8000, 0)):
            with pytest.raises(RaftqError) as ei:
                e.apply_voter_deltas(e.pack_voter_deltas(np.append(good, np.uint64(bad_group)), [1, 1, bad_voters], [full, full, bad_reset]))
            assert ei.value.code == RAFTQ_EINVAL
        with pytest.raises(RaftqError) as ei:
            e.load_voters(np.where(np.arange(G0) == G0 - 1, 1 << n, 1).astype(np.uint16))
        assert ei.value.code == RAFTQ_EINVAL
        assert np.array_equal(e.read_match(), match) and np.array_equal(e.read_votes(), votes) and np.array_equal(e.read_voters(), voters)


@pytest.mark.parametrize("n", [3, 7])
def test_batching_turn(gpu_engine_cls, oracle, stage_mode, n):
    st = State(n, G0, 7700 + n)
    rng = np.random.default_rng(7700 + n)
    bits = R.member_bits(st.voters, n)
    with st.load(gpu_engine_cls(G0, n)) as e, st.load(gpu_engine_cls(G0, n)) as p:
        match, votes, committed = st.match, st.votes, st.committed
        for turn, gated in enumerate((False, True, False)):
            dg, dp = rng.integers(0, G0, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
            dv = rng.integers(0, 14, 1500).astype(np.uint64)
            vg, vp = rng.integers(0, G0, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
            vv = rng.integers(1, 3, 1500).astype(np.uint8)
            match = oracle.apply_deltas(match, dg, dp, dv)
            votes = oracle.apply_vote_deltas(votes, vg, vp, vv)
            assert (match[~bits] == R.U64_MAX).all()
            want, n_changed = R.commit_advance(match, committed, st.voters, gated, st.gate)
            outcome, won, lost = R.vote_tally(votes, st.voters)
            flags = SWEEP_COMMIT | (SWEEP_GATED if gated else 0) | SWEEP_VOTES | SWEEP_CHANGED
            adv, total, c = e.cycle(flags, e.pack_deltas(dg, dp, dv), e.pack_vote_deltas(vg, vp, vv))
            assert total == n_changed and (c.n_changed, c.n_won, c.n_lost) == (n_changed, won, lost), (turn, n_changed, total)
            assert _same_list(adv, committed, want)
            assert np.array_equal(e.read_committed(), want) and np.array_equal(e.read_outcome(), outcome)
            adv16, total, c = p.cycle_packed(flags, p.pack_deltas16(dg, dp, dv), p.pack_vote_deltas(vg, vp, vv))
            assert total == n_changed and (c.n_changed, c.n_won, c.n_lost) == (n_changed, won, lost)
            gr, old, new = _advances(committed, want)
            assert np.array_equal(adv16["group"], gr) and np.array_equal(adv16["new_commit"], new)
            assert np.array_equal(adv16["advanced_by"], np.minimum(new - old, np.uint64(0xffffffff)).astype(np.uint32))
            assert np.array_equal(p.read_committed(), want) and np.array_equal(p.read_outcome(), outcome)
            committed = want
        # RAFTQ_CYCLE_SEGMENTED: a masked turn produces the contiguous list, presented as ONE segment with the same records;
        # NO_ADOPT: the live commit index stays where it was
        dg, dp = rng.integers(0, G0, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
        dv = rng.integers(10, 30, 1500).astype(np.uint64)
        match = oracle.apply_deltas(match, dg, dp, dv)
        want, n_changed = R.commit_advance(match, committed, st.voters)
        assert n_changed > 0
        d, _ = p.stage_packed(1500, 0)
        d[:] = p.pack_deltas16(dg, dp, dv)
        _, total, _ = p.cycle_packed(SWEEP_COMMIT | SWEEP_NO_ADOPT | CYCLE_SEGMENTED, d, None, cap=G0, inplace=True, want_counts=False)
        recs, counts, stride = p.last_advance_segments()
        gr, old, new = _advances(committed, want)
        assert total == n_changed and counts.tolist() == [n_changed]
        assert np.array_equal(recs["group"], gr) and np.array_equal(recs["new_commit"], new)
        assert np.array_equal(p.read_committed(), want)  # the evaluated (shadow) values
        p.sweep(SWEEP_VOTES)
        assert np.array_equal(p.read_committed(), committed)  # ... which were not adopted


def test_refusals_and_the_way_back(gpu_engine_cls, oracle):
    from raftsql_amd import step as S

    n = 5
    st = State(n, G0, 7800)
    with st.load(gpu_engine_cls(G0, n)) as a, st.load(gpu_engine_cls(G0, n), voters=False) as b, S.NodeEngine(G0, n, 0) as node:
        def code(f, *args):
            with pytest.raises(RaftqError) as ei:
                f(*args)
            return ei.value.code, str(ei.value)

        rc, msg = code(SweepSet, [a, b])
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        with SweepSet([b]) as s:
            rc, msg = code(b.load_voters, st.voters)
            assert rc == RAFTQ_ESTATE and "sweep set" in msg
            assert code(b.apply_voter_deltas, b.pack_voter_deltas([0], [1], [0]))[0] == RAFTQ_ESTATE
            s.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)
        node.load_voters(st.voters)
        hup = S.pack_msgs(np.arange(8, dtype=np.uint64), S.MSG_HUP)
        rc, msg = code(node.step_batch, hup)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        assert code(node.apply_log_deltas, [0], [1], [1])[0] == RAFTQ_ESTATE
        assert code(a.sweep, SWEEP_COMMIT | SWEEP_LDS)[0] == RAFTQ_EINVAL
        assert code(a.cycle, SWEEP_COMMIT | SWEEP_LDS)[0] == RAFTQ_EINVAL
        # masked results before, unmasked results after raftq_load_voters(h, NULL); and the refused calls go through
        want, n_changed = R.commit_advance(st.match, st.committed, st.voters)
        c = a.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)
        assert np.array_equal(a.read_committed(), want) and c.n_changed == n_changed
        a.load_voters(None)
        node.load_voters(None)
        assert (a.read_voters() == (1 << n) - 1).all()
        want, n_changed = oracle.commit_advance(st.match, st.committed)
        for flags in (SWEEP_COMMIT | SWEEP_NO_ADOPT, SWEEP_COMMIT | SWEEP_LDS | SWEEP_NO_ADOPT):
            c = a.sweep(flags)
            assert np.array_equal(a.read_committed(), want) and c.n_changed == n_changed
        with SweepSet([a, b]) as s:
            per, tot = s.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)
            assert tot.n_changed == 2 * n_changed and np.array_equal(a.read_committed(), want)
        out, touched = node.step_batch(hup)
        assert touched == 8


def test_clone_state_carries_the_masks(gpu_engine_cls):
    n = 4
    st = State(n, G0, 7900)
    with st.load(gpu_engine_cls(G0, n)) as a, gpu_engine_cls(G0, n) as b, st.load(gpu_engine_cls(G0, n), voters=False) as c:
        b.clone_state_from(a)
        assert np.array_equal(b.read_voters(), st.voters)
        want, n_changed = R.commit_advance(st.match, st.committed, st.voters, True, st.gate)
        got, changed = b.commit_advance(True)
        assert np.array_equal(got, want) and changed == n_changed
        b.clone_state_from(c)  # a source with no masks: the destination's are dropped
        assert (b.read_voters() == (1 << n) - 1).all()
        full = np.full(G0, (1 << n) - 1, np.uint16)
        want, n_changed = R.commit_advance(st.match, st.committed, full)
        got, changed = b.commit_advance(False)
        assert np.array_equal(got, want) and changed == n_changed
