"""CPU: the selection the commit sweep runs when it leaves the self row out (raftq_kernels.hpp select_other_network).
Its comparator lists, read from the kernel source, put the (q-1)-th largest of N-1 inputs at element N/2 - 1 (0-1
principle), and that value is the q-th largest of all N whenever the left-out value is their maximum, ties included."""
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "raftsql_amd", "csrc", "raftq_kernels.hpp")).read()


def _networks():
    start = SRC.index("select_other_network(uint64_t")
    body = SRC[start:SRC.index("#undef CE", start)]
    nets = {2: []}  # one other value: nothing to compare
    parts = re.split(r"if constexpr \(N == (\d)\)", body)
    for k in range(1, len(parts), 2):
        nets[int(parts[k])] = [(int(a), int(b)) for a, b in re.findall(r"CE\((\d), (\d)\)", parts[k + 1])]
    return nets


def _run(net, v):
    v = list(v)
    for a, b in net:
        if v[a] < v[b]:
            v[a], v[b] = v[b], v[a]
    return v


def test_every_peer_count_has_a_network():
    assert sorted(_networks()) == list(range(2, 10))
    assert "return v[N / 2 - 1];" in SRC[SRC.index("select_other_network(uint64_t"):]


def test_zero_one_principle_selects_rank_n_over_2_minus_1():
    for n, net in _networks().items():
        m, k = n - 1, n // 2 - 1
        for a, b in net:
            assert a < b < m, (n, a, b)  # v[N-1] holds no row on that path
        for bits in itertools.product((0, 1), repeat=m):
            assert _run(net, bits)[k] == sorted(bits, reverse=True)[k], (n, bits)


def test_leaving_out_the_maximum_keeps_the_quorum_index():
    """Every vector of values 0..3 over N slots whose slot s holds the maximum: the network over the other N-1 (in slot
    order, as tile_load reads them) gives the q-th largest of all N."""
    for n, net in _networks().items():
        q = n // 2 + 1
        for vals in itertools.product(range(4), repeat=n):
            top = max(vals)
            want = sorted(vals, reverse=True)[q - 1]
            for s in range(n):
                if vals[s] != top:
                    continue
                others = [vals[p] for p in range(n) if p != s]
                assert _run(net, others)[n // 2 - 1] == want, (n, vals, s)
