"""GPU: the two folds of the Tick host paths that no older test pins in every form.

test_round_parity_in_every_tick_form: raftq_tick_frames and raftq_tick_elect_frames(hup_cap = 0) are one implementation; the
parity of the two was held for the plain Tick (test_tick_elect_gpu.py::test_hup_cap_below_the_hup_count) and under CheckQuorum with
PreVote (test_tick_checks_gpu.py::test_hup_cap_zero_is_tick_frames).  Here: the four forms of the Tick -- plain, over voter masks,
with the failed checks listed, both -- on a handle and a twin, every comparison exact.

test_the_cq_word_under_every_writer: the host calls that read and rewrite the cq word (activity bits, leadTransferee, lead_elapsed)
interleaved against a numpy model of the 32-bit word.  The model is the layout as include/raftq.h states it, not the library's."""
import numpy as np
import pytest

from tests import _stepgen
from tests import test_tick_elect_gpu as TE
from tests import test_tick_frames_gpu as TF

pytestmark = pytest.mark.gpu

ET, SEED = TF.ET, TF.SEED
PATTERN = np.uint64(0x5AFE5AFE5AFE5AFE)


# ---- one device-built round -----------------------------------------------------------------------------------------------------------
def _handle(st, hb, voters, active, lead_elapsed):
    """a node's handle with the state loaded; voters: masks + raftq_tick_set_voters; active: CheckQuorum + raftq_tick_set_checks"""
    from raftsql_amd.wire import WireEngine

    e = WireEngine(st.G, st.N, st.self_peer)
    e.set_timers(ET, hb, SEED)
    if active is not None:
        e.set_check_quorum(True)
    _stepgen.load_engine(e, st)
    if voters is not None:
        e.load_voters(voters)
        e.set_tick_voters(True)
    if active is not None:
        e.load_activity(active, lead_elapsed)
        e.set_tick_checks(st.G)
    return e


@pytest.mark.parametrize("form", ["plain", "masks", "checks", "masks_checks"])
def test_round_parity_in_every_tick_form(form):
    """G = 2,100: three 1,024-group blocks, the last one partial.  Per tick the handle runs raftq_tick_frames, the twin
    raftq_tick_elect_frames with hup_cap 0: same bytes, frame_off, first N + 1 words of peer_off, counts, lists and state; the words
    of peer_off behind N + 1 that raftq_tick_frames was handed keep their pattern"""
    from raftsql_amd.engine import pinned_empty

    G, N, me, hb = 2100, 3, 1, 1
    rng = np.random.default_rng(31100 + len(form))
    st = TE.make_state(rng, G, N, me, hb)  # leaders in every block, the others' timers spread so that some fire on every tick
    voters = active = lead_elapsed = None
    if "masks" in form:
        voters = rng.integers(1, 1 << N, G).astype(np.uint16)
        voters[st.role == 2] |= np.uint16(1 << me)  # (a leader is a member of its group)
    if "checks" in form:
        active = rng.integers(0, 1 << N, G).astype(np.uint16)
        lead_elapsed = rng.integers(ET - 3, ET, G).astype(np.uint32)  # checks fall due within the three ticks
    n_lead = int((st.role == 2).sum())
    seen_hup = seen_beat = seen_chk = 0
    with _handle(st, hb, voters, active, lead_elapsed) as e, _handle(st, hb, voters, active, lead_elapsed) as twin:
        for t in range(3):
            beat_cap = [G, n_lead // 2, n_lead][t]  # every slot, fillers behind a cut round, the exact count
            bitmap = t == 1
            bf, be = TF.Bufs(e, beat_cap), TE.Bufs(twin, 0, beat_cap)
            po = pinned_empty(2 * (N + 1) + 2, np.uint64)
            po[:] = PATTERN
            s1, o1, p1, c1, h1, nh1, x1, nb1 = e.tick_frames(bf.out, bf.off[: bf.n_max + 1], po, beat_cap, hup_cap=0, beat_bitmap=bitmap, cap=bf.cap)
            assert (po[N + 1:] == PATTERN).all(), (form, t, "raftq_tick_frames wrote behind its N + 1 words of peer_off")
            s2, o2, p2, c2, camp, h2, nh2, x2, nb2 = twin.tick_elect_frames(None, be.out, be.off[: be.n_max + 1], be.po, 0, beat_cap,
                                                                            beat_bitmap=bitmap, cap=be.cap)
            what = f"{form} tick {t}: n_hup {nh1} n_beat {nb1} frames {c1.n_msgs} bytes {c1.bytes}"
            print(what)
            assert (nh1, nb1, int(c1.n_msgs), int(c1.n_ents), int(c1.n_malformed), int(c1.bytes)) == \
                   (nh2, nb2, int(c2.n_msgs), int(c2.n_ents), int(c2.n_malformed), int(c2.bytes)), what
            assert bytes(s1) == bytes(s2) and np.array_equal(o1, o2), what
            assert np.array_equal(bf.off[: bf.n_max + 1], be.off[: be.n_max + 1]), what  # (the entries past the last frame too)
            assert np.array_equal(p1, p2[: N + 1]), what
            assert len(camp) == 0 and len(h1) == len(h2) == 0 and np.array_equal(x1, x2), what
            assert bf.canaries_ok() and be.canaries_ok(N), what
            if "checks" in form:
                k1, k2 = e.last_tick_checks(), twin.last_tick_checks()
                assert np.array_equal(k1[0], k2[0]) and k1[1] == k2[1], what
                seen_chk += k1[1]
                for a, b in zip(e.read_activity(), twin.read_activity()):
                    assert np.array_equal(a, b), what
            for a, b in zip(e.read_tick(), twin.read_tick()):
                assert np.array_equal(a, b), what
            n1, n2 = e.read_node(), twin.read_node()
            assert all(np.array_equal(n1[k], n2[k]) for k in n1), what
            assert int(c1.n_msgs) > 0, what
            seen_hup, seen_beat = seen_hup + nh1, seen_beat + nb1
    assert seen_hup > 0 and seen_beat > 0 and ("checks" not in form or seen_chk > 0), (form, seen_hup, seen_beat, seen_chk)


# ---- one spelling of the cq word -------------------------------------------------------------------------------------------------------
def _code(f, *args):
    from raftsql_amd.engine import RaftqError

    with pytest.raises(RaftqError) as ei:
        f(*args)
    return ei.value.code


@pytest.mark.parametrize("N", [3, 9])
def test_the_cq_word_under_every_writer(N):
    """the model: word = active (bits 0 .. N - 1) | transferee << 12 (bits 12..15) | lead_elapsed << 16.  At N = 9 the top activity
    bit is bit 8 and transferee 10 fills its four-bit field"""
    from raftsql_amd import _lib
    from raftsql_amd.step import NodeEngine

    G = 130
    rng = np.random.default_rng(31200 + N)
    word = np.zeros(G, np.uint32)  # raftq_set_check_quorum allocates the state zeroed
    top = np.uint16((1 << N) - 1)

    def fields():
        return (word & np.uint32(0xFFF)).astype(np.uint16), ((word >> np.uint32(12)) & np.uint32(0xF)).astype(np.uint8), word >> np.uint32(16)

    def rand_active():
        a = rng.integers(0, 1 << N, G).astype(np.uint16)
        a[:2] = (top, 0)
        return a

    def rand_elapsed():
        le = rng.integers(0, 1 << 16, G).astype(np.uint32)
        le[1:3] = (65535, 0)
        return le

    def rand_transfer():
        tr = rng.integers(0, N + 1, G).astype(np.uint8)
        tr[:2] = (N, 0)  # slot N - 1: at N = 9 the value 9; 10 is refused below
        return tr

    with NodeEngine(G, N, 0) as e:
        e.set_check_quorum(True)
        e.set_lead_transfer(True)

        def same(what):
            act, tr, le = fields()
            got_a, got_le = e.read_activity()
            assert np.array_equal(got_a, act) and np.array_equal(got_le, le) and np.array_equal(e.read_transfer(), tr), what

        def both():
            a, le = rand_active(), rand_elapsed()
            e.load_activity(a, le)
            word[:] = a.astype(np.uint32) | (word & np.uint32(0xF000)) | (le << np.uint32(16))  # (a pending transferee stays)

        def active_only():
            a = rand_active()
            e.load_activity(a, None)
            word[:] = a.astype(np.uint32) | (word & np.uint32(0xFFFFF000))

        def elapsed_only():
            le = rand_elapsed()
            e.load_activity(None, le)
            word[:] = (word & np.uint32(0xFFFF)) | (le << np.uint32(16))

        def transfer():
            tr = rand_transfer()
            e.load_transfer(tr)
            word[:] = (word & np.uint32(0xFFFF0FFF)) | (tr.astype(np.uint32) << np.uint32(12))

        def refused():  # each leaves every word as it was
            bad_a, bad_le, bad_tr = rand_active(), rand_elapsed(), rand_transfer()
            bad_a[G - 1] = np.uint16(1 << N)  # a slot >= N
            bad_le[G - 1] = 65536
            bad_tr[G - 1] = N + 1  # (at N = 9: 10, which the field could hold)
            assert _code(e.load_activity, bad_a, rand_elapsed()) == _lib.RAFTQ_EINVAL
            assert _code(e.load_activity, bad_a, None) == _lib.RAFTQ_EINVAL
            assert _code(e.load_activity, rand_active(), bad_le) == _lib.RAFTQ_EINVAL
            assert _code(e.load_activity, None, bad_le) == _lib.RAFTQ_EINVAL
            assert _code(e.load_transfer, bad_tr) == _lib.RAFTQ_EINVAL

        same("zeroed")
        writers = [both, active_only, elapsed_only, transfer, refused]
        order = [writers[i] for i in rng.permutation(np.repeat(np.arange(len(writers)), 3))]
        for k, w in enumerate([both, transfer] + order):  # (the first two: every field is non-zero before anything is kept)
            w()
            same(f"N={N} call {k}: {w.__name__}")
        act, tr, le = fields()
        assert tr.max() == N and act.max() == top and le.max() == 65535 and tr.any() and (act >> (N - 1)).any()
        e.set_lead_transfer(False)  # clears every transferee and nothing else
        got_a, got_le = e.read_activity()
        assert np.array_equal(got_a, act) and np.array_equal(got_le, le)
        e.set_lead_transfer(True)
        assert not e.read_transfer().any()
        got_a, got_le = e.read_activity()
        assert np.array_equal(got_a, act) and np.array_equal(got_le, le)
