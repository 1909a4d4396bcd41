"""CPU: the yardstick of the two broadcasts over members (tests/ref_bcast_members.py) is itself checked.

With full masks both restatements are the unmasked ones the suite already holds the device to (tests/test_respond_gpu.py::expected
over the C oracle's Step, tests/test_wire_gpu.py::_propose_expect), exactly.  The inputs the GPU tests use discriminate -- as
counts: broadcasts that lost a recipient, that kept all N - 1, that have none; records of reasons 7 and 8.  And the mask-shrink
example takes the road the header describes."""
import numpy as np
import pytest

from oracle import pywire as W
from tests import ref_bcast_members as B
from tests import ref_step_voters as V


@pytest.mark.parametrize("seed,G,N,me,n", [(15100, 800, 5, 2, 3000), (15101, 300, 2, 1, 900), (15102, 500, 9, 0, 1500)])
def test_full_masks_are_the_unmasked_respond_table(oracle, seed, G, N, me, n):
    from tests.test_respond_gpu import expected
    from tests.test_wire_gpu import _node_filter

    st, _, s, off, at_tail = B.respond_input(seed, G, N, me, n)
    full = V.full_masks(N, G)
    plain = V.copy_state(st)
    wm, we, _ = W.wire_decode(s, off)
    _, rec = _node_filter(wm, we, G, N, me, True)
    lt0 = plain.last_term.copy()
    want_o = plain.step_batch(rec)  # the C oracle
    want_w, want_po, want_ans = expected(rec, want_o, lt0, at_tail, N, me)
    _, _, got_o, w, po, ans, bc = B.respond_want(st, full, s, off, at_tail)
    assert got_o.tobytes() == want_o.tobytes()
    assert w.tobytes() == want_w.tobytes() and np.array_equal(po, want_po) and np.array_equal(ans, want_ans)
    assert bc and all(len(b) == N - 1 for b in bc)


@pytest.mark.parametrize("N,me,n_props,n_host", [(3, 2, 200, 50), (5, 1, 300, 0), (2, 1, 33, 7)])
def test_full_masks_are_the_unmasked_proposals(N, me, n_props, n_host):
    from tests.test_wire_gpu import _propose_expect, _propose_setup

    G = 1024
    d, props, pe, pool, hm, he = _propose_setup(np.random.default_rng(15200 + N), G, N, me, n_props, n_host)
    want_m, want_e, new_last, new_lt = _propose_expect(d, N, me, props, pe, hm, he)
    s = B.propose_state(d, N, me)
    full = V.full_masks(N, G)
    assert not B.propose_verdict(s, full, props).any()
    msgs, keep, ents = B.propose_expect(s, full, props, pe, hm, he)
    assert keep.all() and msgs.tobytes() == want_m.tobytes() and ents.tobytes() == want_e.tobytes()
    assert np.array_equal(s.last_index, new_last) and np.array_equal(s.last_term, new_lt)
    stream, off = B.encode_positional(msgs, keep, ents, pool)
    want_s, want_off = W.wire_encode(want_m, want_e, pool)
    assert bytes(stream) == bytes(want_s) and np.array_equal(off, want_off)


def _counts(case, tail_appends=(True,)):
    seed, G, N, me, sizes = case
    _, voters, calls = B.respond_run(seed, G, N, me, sizes, tail_appends)
    bc = [b for c in calls for b in c["want"][6]]
    assert (voters == 0).sum() >= 1 and (np.array([bin(int(v)).count("1") for v in voters]) == 1).sum() >= 3
    return np.array((len(bc),) + B.bcast_counts(bc, N))


def test_the_large_respond_input_discriminates(oracle):
    n, lost, kept, none = _counts(B.RESPOND_BIG, (True, False))
    print("N = 5: %d broadcasts, %d lost a recipient, %d kept all, %d have none" % (n, lost, kept, none))
    assert lost >= 1 and kept >= 1 and none >= 1


@pytest.mark.parametrize("N", range(2, 10))
def test_the_respond_inputs_of_every_slot_discriminate(oracle, N):
    """per self slot: a broadcast that lost a recipient (or, at N = 2, has none) and one that kept all; over the slots: one with none"""
    tot = np.zeros(4, np.int64)
    for me in range(N):
        c = _counts(B.respond_slot_case(N, me), (True, False))
        assert c[1] >= 1 and c[2] >= 1, (N, me, c)
        tot += c
    print("N = %d: %d broadcasts, %d lost a recipient, %d kept all, %d have none" % ((N,) + tuple(tot)))
    assert tot[3] >= 1


@pytest.mark.parametrize("N,me,n_props,n_host", B.PROPOSE_SHAPES)
def test_the_propose_inputs_are_sound_and_lose_frames(N, me, n_props, n_host):
    s, voters, props, pe, pool, hm, he = B.propose_input(B.propose_seed(N, n_props), 8192, N, me, n_props, n_host)
    assert not B.propose_verdict(s, voters, props).any()
    msgs, keep, ents = B.propose_expect(s, voters, props, pe, hm, he)
    assert keep[: len(hm)].all() and keep[len(hm):].sum() >= n_props  # self votes and somebody else does: a frame per record
    if N > 2 and n_props > 1:
        assert not keep.all(), "a non-member's slot"
    stream, off = B.encode_positional(msgs, keep, ents, pool)
    assert len(off) == len(msgs) + 1 and (np.diff(off.astype(np.int64))[~keep] == 0).all() and (np.diff(off.astype(np.int64))[keep] > 0).all()


def test_the_refusal_inputs_hold_both_new_reasons():
    """what tests/test_bcast_members_gpu.py plants: self's bit cleared -> 7; {self} alone -> 8; the shrink example -> 8"""
    N, me = 3, 1
    s, voters, props, pe, pool, hm, he = B.propose_input(16100, 4096, N, me, 600, 50)
    v7, v8 = voters.copy(), voters.copy()
    g7, g8 = int(props["group"][17]), int(props["group"][400])
    v7[g7] &= ~np.uint16(1 << me)
    v8[g8] = 1 << me
    r7, r8 = B.propose_verdict(s, v7, props), B.propose_verdict(s, v8, props)
    assert (r7 == B.PROP_NO_MEMBER).sum() == 1 and r7[17] == B.PROP_NO_MEMBER and (r7 == B.PROP_COMMITS).sum() == 0
    assert (r8 == B.PROP_COMMITS).sum() == 1 and r8[400] == B.PROP_COMMITS and (r8 == B.PROP_NO_MEMBER).sum() == 0


def test_the_mask_shrink_example():
    """N = 5, self 0, Match 10, 8, 5, 5, 5, committed 5, voters {0, 1, 2}: reason 8; the tail report with the unchanged tail
    commits 8; then the proposal passes and maybeCommit does not move on its append"""
    from raftsql_amd.wire import PROP_DT

    s, voters = B.shrink_example()
    props = np.zeros(1, PROP_DT)
    props["group"], props["n_ents"] = 2, 1
    assert list(B.propose_verdict(s, voters, props)) == [B.PROP_COMMITS]
    assert not B.propose_verdict(s, V.full_masks(5, 4), props).any()  # every slot voting: 5 is held by a quorum, nothing moves
    got = V.apply_log_deltas(s, voters, [2], 10, 3)
    assert list(got) == [8] and int(s.committed[2]) == 8
    assert not B.propose_verdict(s, voters, props).any()
    r = V.from_node_state(s, 2, voters[2])
    r.prs[r.id].maybe_update(11)
    assert not r.maybe_commit() and r.committed == 8
