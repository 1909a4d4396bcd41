"""CPU: the tally mirror's arithmetic (tests/ref_tally.py: build, ingest rule, outcome from a byte) held to tests/ref_numpy.py's
vote outcome -- exhaustively over all 4^N field patterns for N <= 5 (the 11 fields included), on 10^5 random words each for
N = 7 and 9; the no-carry claim of the nibble add at its extremes; and what the inputs of tests/test_tally_gpu.py cover."""
import itertools

import numpy as np
import pytest

from tests import ref_numpy as R
from tests import ref_tally as T


def _want(fields):
    """ref_numpy's outcome of [N][G] fields (a field of 3 is neither answer there too: it compares with 1 and 2)"""
    return R.vote_tally(fields)[0]


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_every_field_pattern(n):
    pats = np.array(list(itertools.product(range(4), repeat=n)), np.uint8).T  # [N][4^N]
    assert pats.shape == (n, 4 ** n)
    words = T.pack_words(pats)
    assert np.array_equal(T.fields(words, n), pats)
    tally = T.build(words, n)
    assert np.array_equal(tally & 15, (pats == 1).sum(axis=0)) and np.array_equal(tally >> 4, (pats == 2).sum(axis=0))
    assert np.array_equal(T.outcome_from_tally(tally, n), _want(pats))
    # bits of the word above the N fields are not counted (poll_word's mask)
    assert np.array_equal(T.build(words | np.uint32(0xFFFFFFFF << (2 * n) & 0xFFFFFFFF), n), tally)


@pytest.mark.parametrize("n", (7, 9))
def test_random_words(n):
    rng = np.random.default_rng(31000 + n)
    words = rng.integers(0, 1 << (2 * n), 100_000, dtype=np.uint64).astype(np.uint32)
    pats = T.fields(words, n)
    assert (pats == 3).any() and all((_want(pats) == k).any() for k in (0, 1, 2))
    assert np.array_equal(T.outcome_from_tally(T.build(words, n), n), _want(pats))


@pytest.mark.parametrize("n", (1, 2, 3, 5, 7, 9))
def test_the_nibble_add_never_carries(n):
    """four neighbouring groups share a 32-bit word: every peer of every one of them answers, all granting, all rejecting, and
    split -- each nibble ends at most at N <= 9 < 16 and the neighbours' bytes are what they would be alone"""
    for split in (0, n // 2, n):  # peers below `split` grant, the others reject
        votes = np.zeros((n, 8), np.uint8)
        tally = np.zeros(8, np.uint8)
        g = np.repeat(np.arange(8), n)
        p = np.tile(np.arange(n), 8)
        v = np.where(p < split, 1, 2)
        order = np.random.default_rng(31100 + n).permutation(g.size)
        adds = T.ingest(votes, tally, g[order], p[order], v[order])
        assert adds == 8 * n
        assert (tally == (split | ((n - split) << 4))).all()
        assert np.array_equal(tally, T.build(T.pack_words(votes), n))
        # every record again: answered slots take nothing, no byte moves
        assert T.ingest(votes, tally, g, p, 3 - v) == 0 and (tally == (split | ((n - split) << 4))).all()


@pytest.mark.parametrize("n", (1, 2, 3, 5, 7, 9))
def test_ingest_rule_against_the_build(n):
    """a random batch with duplicates and both answers per slot on random fields: the followed bytes are the rebuilt ones, the
    fields are first-in-batch-wins"""
    rng = np.random.default_rng(31200 + n)
    votes = rng.integers(0, 3, (n, 64)).astype(np.uint8)
    tally = T.build(T.pack_words(votes), n)
    g, p, v = rng.integers(0, 64, 500), rng.integers(0, n, 500), rng.integers(1, 3, 500)
    want = votes.copy()
    for gi, pi, vi in zip(g, p, v):  # sequential poll(): the first response of a peer stands
        if want[pi, gi] == 0:
            want[pi, gi] = vi
    T.ingest(votes, tally, g, p, v)
    assert np.array_equal(votes, want)
    assert np.array_equal(tally, T.build(T.pack_words(votes), n))
    assert np.array_equal(T.outcome_from_tally(tally, n), _want(votes))


@pytest.mark.parametrize("n", (1, 2, 3, 5, 7, 9))
def test_gpu_inputs_cover_the_outcomes_and_the_duplicates(n):
    st = T.gpu_state(n, 32000 + n)
    before = _want(st.votes)
    assert all((before == k).any() for k in (0, 1, 2))
    q = R.quorum(n)
    assert before[0] == 0 and before[1] == 0 and before[2] == 1 and before[3] == 2
    votes = st.votes.copy()
    tally = T.padded(T.build(T.pack_words(votes), n))
    g, p, v = T.gpu_vote_batch(n, 32050 + n)
    dup = [(int(a), int(b)) for a, b in zip(g, p)]
    assert dup.count((0, q - 1)) == 3 and dup.count((1, q - 1)) == 3 and len(set(dup)) < len(dup)
    T.ingest(votes, tally, g, p, v)
    after = _want(votes)
    assert np.array_equal(T.outcome_from_tally(tally[:T.G], n), after) and np.array_equal(tally[:T.G], T.build(T.pack_words(votes), n))
    assert all((after == k).any() for k in (0, 1, 2))
    assert (after[0], after[1], after[4], after[5]) == (1, 2, 1, 2)  # the deciding votes; first in batch position wins
    assert votes[0, 2] == 1  # the answered slot kept its answer
    # counted once: the bytes of groups 0 and 1 say q, not q + 2
    assert tally[0] == q and tally[1] == q << 4
