"""CPU: the masked decision stated three ways that must agree (tests/ref_voters.py):
  1. the existing oracle's per-group mci_sort / mci_count / poll on the voters' gathered column,
  2. the kernel's formulation -- zero the non-voters, sort descending, take index q_g - 1,
  3. the counting definition -- the largest i such that at least q_g voters have match >= i.
Exhaustive for N <= 5 (every mask, values in {0..3}^N), random for N = 6..9 with ties and values at 2^64 - 1.  The kernel
takes ANY position of the sorted order, so the comparator lists of raftq_kernels.hpp must sort every position: checked from
the source, and the whole masked selection is replayed through them."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import ref_voters as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "raftsql_amd", "csrc", "raftq_kernels.hpp")).read()


def _networks():
    body = SRC[SRC.index("select_quorum_network"):SRC.index("#undef CE")]
    nets = {1: []}
    parts = re.split(r"if constexpr \(N == (\d)\)", body)
    for k in range(1, len(parts), 2):
        nets[int(parts[k])] = [(int(a), int(b)) for a, b in re.findall(r"CE\((\d), (\d)\)", parts[k + 1])]
    return nets


def _exhaustive(n, values):
    """every (mask, value tuple): -> match [N, K], voters [K]"""
    tuples = np.array(list(itertools.product(values, repeat=n)), dtype=np.uint64).T  # [N, V]
    masks = np.arange(1 << n, dtype=np.uint16)
    match = np.tile(tuples, (1, masks.size))
    voters = np.repeat(masks, tuples.shape[1])
    return match, voters


@pytest.mark.parametrize("n", range(1, 6))
def test_three_statements_agree_exhaustively(oracle, n):
    match, voters = _exhaustive(n, range(4))
    k = R.candidate_kernel_form(match, voters)
    assert np.array_equal(k, R.candidate_counting_form(match, voters))
    assert np.array_equal(k, R.candidate_oracle_form(oracle, match, voters))
    assert np.array_equal(k, R.candidate_oracle_form(oracle, match, voters, count=True))
    assert (k[voters == 0] == 0).all()  # an empty mask commits nothing
    full = voters == (1 << n) - 1  # a full mask is the unmasked decision
    assert np.array_equal(k[full], np.sort(match[:, full], axis=0)[::-1][n // 2])


@pytest.mark.parametrize("n", range(1, 6))
def test_tally_agrees_with_the_oracle_exhaustively(oracle, n):
    votes, voters = _exhaustive(n, range(3))
    votes = votes.astype(np.uint8)
    out, won, lost = R.vote_tally(votes, voters)
    assert np.array_equal(out, R.tally_oracle_form(oracle, votes, voters))
    assert (won, lost) == (int((out == 1).sum()), int((out == 2).sum()))
    assert (out[voters == 0] == 0).all()  # an empty mask stays pending


def _random(n, k, seed):
    rng = np.random.default_rng(seed)
    match = rng.integers(0, 6, (n, k)).astype(np.uint64)  # a small range: ties
    top = rng.random((n, k)) < 0.1
    match[top] = R.U64_MAX - rng.integers(0, 2, int(top.sum())).astype(np.uint64)
    voters = rng.integers(0, 1 << n, k).astype(np.uint16)
    voters[:8] = np.array([0, (1 << n) - 1, 1, 1 << (n - 1), 3, (1 << n) - 2, 5, 0]) & ((1 << n) - 1)
    return match, voters, rng


@pytest.mark.parametrize("n", range(6, 10))
def test_three_statements_agree_on_random_groups(oracle, n):
    match, voters, rng = _random(n, 3000, 4100 + n)
    k = R.candidate_kernel_form(match, voters)
    assert np.array_equal(k, R.candidate_counting_form(match, voters))
    assert np.array_equal(k, R.candidate_oracle_form(oracle, match, voters))
    assert np.array_equal(k, R.candidate_oracle_form(oracle, match, voters, count=True))
    votes = rng.integers(0, 3, (n, 3000)).astype(np.uint8)
    assert np.array_equal(R.vote_tally(votes, voters)[0], R.tally_oracle_form(oracle, votes, voters))


def test_every_comparator_list_sorts_every_position():
    """0-1 principle over ALL outputs: the masked kernel reads any of positions 0 .. N/2, and which one is a per-group value."""
    nets = _networks()
    assert sorted(nets) == list(range(1, 10))
    for n, net in nets.items():
        assert all(a < b < n for a, b in net)
        inputs = np.array(list(itertools.product((0, 1), repeat=n)), dtype=np.uint64).T
        out = R.sort_through_network(net, inputs)
        assert np.array_equal(out, np.sort(inputs, axis=0)[::-1]), n


@pytest.mark.parametrize("n", range(1, 10))
def test_masked_selection_through_the_kernels_networks(n):
    """what sweep_voters_kernel does, with the lists it compiles: zero, the full network, element popcount / 2"""
    match, voters, _ = _random(n, 4000, 4200 + n)
    z = np.where(R.member_bits(voters, n), match, np.uint64(0))
    s = R.sort_through_network(_networks()[n], z)
    idx = (R.popcount16(voters) // 2).astype(np.int64)
    assert np.array_equal(np.take_along_axis(s, idx[None, :], axis=0)[0], R.candidate_counting_form(match, voters))


def test_hand_cases(oracle):
    m = np.array([[10], [7], [3], [99], [99]], dtype=np.uint64)
    three = np.array([0b00111], np.uint16)
    for f in (R.candidate_kernel_form, R.candidate_counting_form, lambda a, b: R.candidate_oracle_form(oracle, a, b)):
        assert f(m, three)[0] == 7                                  # voters {0,1,2} of five: the non-voters' 99s do not count
        assert f(m, np.array([0b11111], np.uint16))[0] == 10        # all five: [99, 99, 10, 7, 3] -> the third
    assert R.quorum(np.array([0b01111, 0b00111, 0b00001, 0], np.uint16)).tolist() == [3, 2, 1, 1]  # 4 voters -> q = 3
    assert R.candidate_kernel_form(m, np.array([0b01111], np.uint16))[0] == 7  # slots 0..3: [99, 10, 7, 3] -> the third
    # adding a voter lowers the candidate; the commit index stays
    c, n_changed = R.commit_advance(m, np.array([0], np.uint64), three)
    assert (c[0], n_changed) == (7, 1)
    with_new = np.array([[10], [7], [3], [0], [99]], dtype=np.uint64)  # slot 3 joins, its Match reset to 0
    four = np.array([0b01111], np.uint16)
    assert R.candidate_kernel_form(with_new, four)[0] == 3
    c2, n_changed = R.commit_advance(with_new, c, four)
    assert (c2[0], n_changed) == (7, 0)
    # a tally in which only non-voters grant stays pending
    votes = np.array([[0], [0], [0], [1], [1]], dtype=np.uint8)
    out, won, lost = R.vote_tally(votes, three)
    assert (int(out[0]), won, lost) == (0, 0, 0)
    assert R.vote_tally(votes, np.array([0b11000], np.uint16))[0][0] == 1
    # the gate applies to the masked candidate
    assert R.commit_advance(m, np.array([0], np.uint64), three, True, np.array([8], np.uint64))[0][0] == 0
    assert R.commit_advance(m, np.array([0], np.uint64), three, True, np.array([7], np.uint64))[0][0] == 7


def test_last_voter_delta_of_a_group_wins():
    match = np.arange(12, dtype=np.uint64).reshape(3, 4) + 1
    votes = np.ones((3, 4), np.uint8)
    voters = np.full(4, 7, np.uint16)
    m, v, k = R.apply_voter_deltas(match, votes, voters, [1, 2, 1], [3, 5, 6], [7, 1, 4])
    assert k.tolist() == [7, 6, 5, 7]
    assert m[:, 1].tolist() == [2, 6, 0] and v[:, 1].tolist() == [1, 1, 0]  # the first record of group 1 (reset 7) did nothing
    assert m[:, 2].tolist() == [0, 7, 11] and v[:, 2].tolist() == [0, 1, 1]
