"""CPU: the narrow mirror (tests/ref_narrow.py) selects what the rows select (tests/ref_numpy.py) wherever it is valid,
and says so exactly where a group's values fit 32 bits above their smallest."""
import itertools
import os
import re

import numpy as np
import pytest

from raftsql_amd import synth
from tests import ref_narrow as RN
from tests import ref_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "raftsql_amd", "csrc", "raftq_kernels.hpp")).read()
U64 = (1 << 64) - 1


def _same_sweep(match, committed, first_idx=None):
    mir = RN.build(match)
    assert mir.valid
    assert np.array_equal(mir.rows(), np.asarray(match, np.uint64))
    assert np.array_equal(RN.mci(mir), R.mci(match))
    assert np.array_equal(RN.mci(mir), R.mci_bruteforce(match))
    got, n = RN.commit_advance(mir, committed)
    want, wn = R.commit_advance(match, committed)
    assert np.array_equal(got, want) and n == wn
    if first_idx is not None:
        got, n = RN.commit_advance(mir, committed, True, first_idx)
        want, wn = R.commit_advance(match, committed, True, first_idx)
        assert np.array_equal(got, want) and n == wn


@pytest.mark.parametrize("n", range(1, 10))
def test_synth_state_is_valid_and_sweeps_the_same(n):
    st = synth.make_groups(5000, n, seed=synth.SEED_BASE + n, with_terms=True)
    spread = st.match.max(axis=0) - st.match.min(axis=0)
    assert int(spread.max()) < RN.SPAN
    _same_sweep(st.match, st.committed, st.first_idx_cur_term)


@pytest.mark.parametrize("n", range(1, 10))
def test_adversarial_block(n):
    """its 0-and-UINT64_MAX groups have no 32-bit offsets: the block as a whole is invalid (from two peers on); group
    by group, every group that fits sweeps the same"""
    st = synth.adversarial_block(n)
    mir = RN.build(st.match)
    spread = st.match.max(axis=0) - st.match.min(axis=0)
    assert mir.valid == bool((spread < np.uint64(RN.SPAN)).all())
    assert mir.valid == (n == 1)
    fits = np.nonzero(spread < np.uint64(RN.SPAN))[0]
    assert 0 < len(fits)
    _same_sweep(st.match[:, fits], st.committed[fits], st.first_idx_cur_term[fits])


@pytest.mark.parametrize("n", [2, 3, 5, 9])
def test_spread_at_the_edge(n):
    for base in (0, 1, 12345, (1 << 40) + 7, U64 - (RN.SPAN - 1)):
        m = np.full((n, 3), base, dtype=np.uint64)
        m[n - 1, 1] = base + RN.SPAN - 1  # exactly 2^32 - 1 above: the largest offset there is
        assert RN.build(m).valid
        _same_sweep(m, np.zeros(3, np.uint64))
        if base + RN.SPAN <= U64:
            m[0, 2] = base + RN.SPAN  # exactly 2^32 above: one too many
            assert not RN.build(m).valid


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8])
def test_values_next_to_two_to_the_64(n):
    rng = np.random.default_rng(n)
    m = (np.uint64(U64) - rng.integers(0, 1 << 31, (n, 257)).astype(np.uint64)).astype(np.uint64)
    m[:, 0] = U64
    m[0, 1] = U64
    c = (np.uint64(U64) - rng.integers(0, 1 << 31, 257).astype(np.uint64)).astype(np.uint64)
    _same_sweep(m, c, np.where(np.arange(257) % 3 == 0, 0, m.min(axis=0)).astype(np.uint64))


@pytest.mark.parametrize("n", range(1, 10))
def test_ties_at_position_q_minus_1(n):
    q = R.quorum(n)
    cols = []
    for base in (9, (1 << 33) + 9):
        cols.append([base + 5] * (q - 1) + [base] * (n - q + 1))      # the tie block starts exactly at q - 1
        cols.append([base + 5] * q + [base] * (n - q))                # ... ends exactly at q - 1
        cols.append([base] * n)                                        # all equal
        cols.append([base + 5] * (q - 1) + [base + 2] + [base] * (n - q))
    m = np.array(cols, dtype=np.uint64).T
    for perm in itertools.islice(itertools.permutations(range(n)), 24):
        _same_sweep(m[list(perm)], np.full(m.shape[1], 8, np.uint64))


def test_ingest_rule():
    """the four records of the issue, on one group each: at anchor + 2^32 - 1 (kept), at anchor + 2^32 (ends the mirror),
    below the anchor (nothing moves), equal to the current value (nothing moves)"""
    n = 5
    st = synth.make_groups(64, n, seed=synth.SEED_BASE + 77)
    for which, keeps in (("edge", True), ("over", False), ("below", True), ("equal", True)):
        match = st.match.copy()
        mir = RN.build(match)
        assert mir.valid
        a = int(mir.anchor[7])
        value = {"edge": a + RN.SPAN - 1, "over": a + RN.SPAN, "below": a - 1, "equal": int(match[2, 7])}[which]
        before = match.copy()
        RN.ingest(match, mir, [7], [2], [value])
        assert mir.valid == keeps
        assert np.array_equal(match[2, 7], max(int(before[2, 7]), value))
        if which in ("below", "equal"):
            assert np.array_equal(match, before)
        if keeps:
            assert np.array_equal(mir.rows(), match)
            assert np.array_equal(RN.mci(mir), R.mci(match))
            assert np.array_equal(mir.anchor, RN.build(before).anchor)  # ingest never moves an anchor


def test_ingest_is_order_independent_and_keeps_the_mirror():
    rng = np.random.default_rng(5)
    st = synth.make_groups(300, 5, seed=synth.SEED_BASE + 78)
    g = rng.integers(0, 300, 2000)
    p = rng.integers(0, 5, 2000)
    v = st.match[p, g].astype(np.int64) + rng.integers(-3000, 3000, 2000)
    v = np.maximum(v, 0)
    outs = []
    for order in (np.arange(2000), rng.permutation(2000)):
        match = st.match.copy()
        mir = RN.build(match)
        RN.ingest(match, mir, g[order], p[order], v[order])
        assert mir.valid and np.array_equal(mir.rows(), match)
        outs.append((match, mir.off.copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_body_rule_is_the_fewest_bytes():
    """DESIGN 4.1's table: narrow beats the self-row skip from N = 5 and every row from N = 3"""
    for n in range(1, 10):
        assert RN.body(n, False, False) == "all"
        assert RN.body(n, True, False) == ("skip" if n >= 2 else "all")
        assert RN.body(n, False, True) == ("narrow" if n >= 3 else "all")
        assert RN.body(n, True, True) == ("narrow" if n >= 5 else "skip" if n >= 2 else "all")
    assert RN.narrow_bytes(5) == (28, 32, 40)
    # ... and the kernel source states the same thresholds
    rule = SRC[SRC.index("tile_body(const SweepArgs& a)"):]
    rule = rule[:rule.index("\n}\n")]
    assert "N < 3" in rule and "N < 5 && skip != 0" in rule


# ---- the comparator lists at 32 bits: the narrow body runs select_quorum_network<N, uint32_t> over the offsets --------------
def _networks():
    body = SRC[SRC.index("select_quorum_network"):SRC.index("#undef CE")]
    nets = {}
    parts = re.split(r"if constexpr \(N == (\d)\)", body)
    for k in range(1, len(parts), 2):
        nets[int(parts[k])] = [(int(a), int(b)) for a, b in re.findall(r"CE\((\d), (\d)\)", parts[k + 1])]
    return nets


def _run_u32(net, v):
    v = np.array(v, dtype=np.uint32)
    for a, b in net:
        hi, lo = np.maximum(v[a], v[b]), np.minimum(v[a], v[b])  # v_max_u32 / v_min_u32
        v[a], v[b] = hi, lo
    return v


def test_one_comparator_list_for_both_widths():
    """the lists are not copied: one template over the value type, one compare-exchange"""
    assert SRC.count("CE(0, 3); CE(1, 4); CE(0, 2); CE(1, 3); CE(0, 1); CE(2, 4); CE(1, 2); CE(3, 4); CE(2, 3);") == 2  # N = 5, and N = 6 less its self row
    assert re.search(r"template <int N, typename T = uint64_t>\s*__device__ __forceinline__ T select_quorum_network\(T \(&v\)\[N\]\)", SRC)
    assert re.search(r"template <typename T>\s*__device__ __forceinline__ void ce_desc\(T& a, T& b\)", SRC)
    assert "select_quorum_network<N, uint32_t>" in SRC


def test_zero_one_principle_at_32_bits():
    top = 0xFFFFFFFF  # the 0-1 principle with the extreme values of the width: a signed compare would fail here
    for n, net in _networks().items():
        k = n // 2
        for bits in itertools.product((0, top), repeat=n):
            got = _run_u32(net, bits)
            assert int(got[k]) == sorted(bits, reverse=True)[k], (n, bits)
            assert all(got[i] >= got[i + 1] for i in range(n - 1))


def test_networks_select_the_quorum_offset():
    rng = np.random.default_rng(9)
    for n, net in _networks().items():
        off = rng.integers(0, 1 << 32, (n, 500), dtype=np.uint64).astype(np.uint32)
        off[:, :50] = rng.integers(0, 3, (n, 50)).astype(np.uint32)  # ties
        got = _run_u32(net, off)[n // 2]
        assert np.array_equal(got, np.sort(off, axis=0)[n - R.quorum(n)])
