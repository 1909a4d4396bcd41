"""GPU: the streaming decoder's narrow output forms (include/raftq_wire.h: raftq_wire_decode_packed, raftq_step_frames_packed)
against the CPU oracle's decode and against a twin engine running the plain call -- never against the packed call itself.
What has to come out is worked out from the reference's 64-byte records by the rule's own Python statement
(tests/packed_rule.py); raftsql_amd.wire.expand_packed of what DID come out has to give those records back.

Shapes: 256 frames are a tile (one workgroup); n = 1, 2, 255, 256, 257, 513 are one lane, one quad of two heads, the 8-byte
edge of an odd last tile, exactly one tile, a tile boundary and a look-back across three tiles.

One departure from the letter of the issue, with its reason: it asks that "every one of the three tiles" of the 513-frame
node-shaped case hold both narrow and wide frames -- the third tile of 513 frames holds ONE frame and cannot.  The test
asserts what can hold and asks no less of the look-back: both full tiles hold both kinds, and the third tile's one frame is
wide, so that its place in wide[] is the sum of both tiles before it."""
import numpy as np
import pytest

from tests import packed_rule as R

pytestmark = pytest.mark.gpu

FORMS = [R.FORM_40, R.FORM_HEAD]


def _head_types(form):
    return R.RESPONSE_KINDS if form == R.FORM_HEAD else 0


@pytest.fixture(scope="module")
def eng():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test started without a visible GPU")
    from raftsql_amd.wire import WireEngine

    with WireEngine(64, 3, self_peer=0) as e:
        yield e


def _same(a, b, what=""):
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b), (what, len(a), len(b))
    if a.tobytes() != b.tobytes():
        for i in range(len(a)):
            assert a[i].tobytes() == b[i].tobytes(), (what, i, a[i], b[i])


CANARY = 0xA5


class _Bufs:
    """page-locked arrays of one packed call, with canary bytes behind narrow[n] and wide[wide_cap]"""

    def __init__(self, s, off, form, wide_cap, n_ents):
        from raftsql_amd import wire as W
        from raftsql_amd.engine import pinned_copy, pinned_empty

        self.n = len(off) - 1
        self.s, self.off = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
        self._narrow = pinned_empty(self.n * form + 64, np.uint8)
        self._wide = pinned_empty(wide_cap * 64 + 128, np.uint8)
        self._narrow[:] = CANARY
        self._wide[:] = CANARY
        self.narrow = self._narrow[: self.n * form].view(W._FORM_DT[form])
        self.wide = self._wide[: wide_cap * 64].view(W.WIRE_MSG_DT)
        self.ents = pinned_empty(n_ents + 1, W.WIRE_ENT_DT)

    def assert_canaries(self, form, wide_cap, what=""):
        assert np.all(self._narrow[self.n * form:] == CANARY), f"{what}: bytes behind narrow[n] were written"
        assert np.all(self._wide[wide_cap * 64:] == CANARY), f"{what}: bytes behind wide[wide_cap] were written"


def _check_decode(e, kind, seed, n, form, to_slot=0, head_types=None, wide_cap=None):
    """one raftq_wire_decode_packed call against the oracle's records of the corpus -> n_wide"""
    from raftsql_amd import _lib
    from raftsql_amd import wire as W
    from raftsql_amd.engine import pinned_empty

    s, off, m, we, bad = R.oracle_decode(kind, seed, n)
    ht = _head_types(form) if head_types is None else head_types
    want_narrow, want_wide = R.pack(m, to_slot, form, ht)
    cap = len(want_wide) if wide_cap is None else wide_cap
    b = _Bufs(s, off, form, cap, len(we))
    narrow, wide, ents, c, n_wide, rc = e.wire_decode_packed(b.s, b.off, form, to_slot, b.narrow, b.wide, b.ents, head_types=ht, check=False)
    what = f"{kind} n={len(m)} form={form} cap={cap}"
    b.assert_canaries(form, cap, what)
    assert n_wide == len(want_wide), what  # (what the rule's Python statement says)
    assert rc == (_lib.RAFTQ_OK if cap >= len(want_wide) else _lib.RAFTQ_EINVAL), what
    _same(narrow, want_narrow, what + " narrow")
    _same(wide, want_wide[:cap], what + " wide[] = the oracle's records at the wide positions, in frame order")
    if cap >= len(want_wide):
        _same(W.expand_packed(narrow, wide, to_slot, form), R.delivered(m, to_slot, form, ht), what + " expansion")
    # ents and counts: raftq_wire_decode's on the same input (and the oracle's)
    msgs, ents2 = pinned_empty(max(len(m), 1), W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT)
    c2 = _lib.WireCounts()
    import ctypes as C

    e._chk(e._lib.raftq_wire_decode(e._h, b.s.ctypes.data, len(b.s), b.off.ctypes.data, len(m), msgs.ctypes.data, ents2.ctypes.data, len(ents2), C.byref(c2)))
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (c2.n_msgs, c2.n_ents, c2.n_malformed, c2.bytes) and c.n_malformed == bad, what
    _same(ents, ents2[: int(c2.n_ents)], what + " ents")
    _same(ents, we, what + " ents (oracle)")
    _same(msgs[: len(m)], m, what + " the plain call")
    return n_wide


def _tiles_hold_both(m, form, to_slot=0):
    wide = ~R.is_narrow(m, to_slot, form, _head_types(form))
    for t0 in range(0, len(m) - 255, 256):  # the full tiles
        assert 0 < int(wide[t0:t0 + 256].sum()) < 256, (form, t0)
    return wide


# ---- parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
@pytest.mark.parametrize("kind,seed", [("node", 30), ("random", 40)])
def test_parity(eng, oracle, kind, seed, n, form):
    if kind == "node" and n == 513:
        m = R.oracle_decode(kind, seed + n, n)[2]
        wide = _tiles_hold_both(m, form)  # (from the rule's statement, not from the device)
        assert len(m) == 513 and wide[512], "the third tile's one frame is wide: its place comes from both tiles before it"
    n_wide = _check_decode(eng, kind, seed + n, n, form)
    if kind == "random" and n >= 255:
        assert n_wide > 0.9 * n


# ---- limits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_all_wide_and_none_wide(eng, oracle, form):
    # the node's frames read as another slot's: 513 wide frames, the full 256-record gather in every full tile
    assert _check_decode(eng, "node", 543, 513, form, to_slot=1) == 513
    # acknowledgements, heartbeats and votes only, every kind allowed as a head: not one wide frame
    assert _check_decode(eng, "acks", 544, 513, form, head_types=0xFFFFFFFF) == 0


@pytest.mark.parametrize("form", FORMS)
def test_malformed_hand_cases(eng, oracle, form):
    n_wide = _check_decode(eng, "malformed", 0, 0, form, to_slot=R.MALFORMED_TO_SLOT)
    m = R.oracle_decode("malformed", 0, 0)[2]
    assert int(((m["flags"] & 1) != 0).sum()) == 10 and 0 < n_wide < len(m) - 10


@pytest.mark.parametrize("form", FORMS)
def test_fuzz_with_noise_and_garbage_boundaries(eng, oracle, form):
    _check_decode(eng, "fuzz", 51, 0, form)
    _check_decode(eng, "noncanonical", 52, 0, form)


# ---- nothing beyond the arrays; capacity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [257, 513])
def test_short_wide_array(eng, oracle, n, form):
    """wide_cap exact, one short, and none at all: RAFTQ_EINVAL past the first, *n_wide right, the first wide_cap records right,
    canaries behind narrow[n] (odd n: the 8-byte edge) and wide[wide_cap] intact -- all checked in _check_decode"""
    m = R.oracle_decode("node", 60 + n, n)[2]
    total = int((~R.is_narrow(m, 0, form, _head_types(form))).sum())
    assert total > 2
    for cap in (total, total - 1, 0):
        assert _check_decode(eng, "node", 60 + n, n, form, wide_cap=cap) == total


# ---- launch shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_few_workers_and_no_readers(oracle, form, monkeypatch):
    """two worker workgroups for three tiles (a worker takes several), and no reader workgroups at all (every chunk is brought
    in by a worker): the overrides of tests/test_wire_gpu.py"""
    from raftsql_amd.wire import WireEngine

    monkeypatch.setenv("RAFTQ_WIRE_WGS", "2")
    monkeypatch.setenv("RAFTQ_WIRE_READERS", "0")
    with WireEngine(64, 3, self_peer=0) as e:
        _check_decode(e, "node", 543, 513, form)
        monkeypatch.delenv("RAFTQ_WIRE_READERS")
        _check_decode(e, "node", 543, 513, form)  # (the chunk ticket is re-based behind a launch without readers)
        monkeypatch.setenv("RAFTQ_WIRE_WGS", "1")
        _check_decode(e, "random", 553, 513, form)


# ---- Step: twin engines from one state ---------------------------------------------------------------------------------------
def _state_of(e):
    st = e.read_node()
    st["match"], st["votes"] = e.read_match(), e.read_votes()
    return st


def _assert_same_state(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _step_twins(N, me, tail_appends, frames_of, n_calls=2):
    from raftsql_amd import wire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, n = 64, 700
    rng = np.random.default_rng(900 + 10 * N + me + (100 if tail_appends else 0))
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    with WireEngine(G, N, me) as plain, WireEngine(G, N, me) as e40, WireEngine(G, N, me) as e8:
        for e in (plain, e40, e8):
            _stepgen.load_engine(e, st)
        for it in range(n_calls):
            s, off = frames_of(rng, n, st)
            ps, po = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
            msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(4 * n, W.WIRE_ENT_DT)
            tm, te, to, tc = plain.step_frames(ps, po, msgs, ents, tail_appends=tail_appends)
            tm, te = tm.copy(), te.copy()
            assert len(set(int(t) for t in to["type"])) >= 4  # the batch does exercise Step
            want_state = _state_of(plain)
            for e, form in ((e40, R.FORM_40), (e8, R.FORM_HEAD)):
                what = f"N={N} self={me} tail_appends={tail_appends} call {it} form {form}"
                ht = _head_types(form)
                want_narrow, want_wide = R.pack(tm, me, form, ht)
                assert 0 < len(want_wide) < n, what
                b = _Bufs(s, off, form, len(want_wide), 4 * n - 1)
                narrow, wide, ge, go, c, n_wide = e.step_frames_packed(b.s, b.off, form, b.narrow, b.wide, b.ents, head_types=ht,
                                                                       tail_appends=tail_appends)
                b.assert_canaries(form, len(want_wide), what)
                _same(go, to, what + " results")
                assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (tc.n_msgs, tc.n_ents, tc.n_malformed, tc.bytes), what
                _same(ge, te, what + " ents")
                assert n_wide == len(want_wide), what
                _same(narrow, want_narrow, what + " narrow")
                _same(wide, want_wide, what + " wide")
                # ... RAFTQ_MSGF_* and a MsgApp's overwritten reject_hint included
                _same(W.expand_packed(narrow, wide, me, form), R.delivered(tm, me, form, ht), what + " expansion = the twin's msgs")
                _assert_same_state(_state_of(e), want_state, what)
            if it == 0:  # a short wide array is no error here: the frames have been stepped
                s2, off2 = frames_of(rng, n, st)
                ps, po = pinned_copy(np.ascontiguousarray(s2)), pinned_copy(np.ascontiguousarray(off2, np.uint64))
                tm, te, to, tc = plain.step_frames(ps, po, msgs, ents, tail_appends=tail_appends)
                want_state = _state_of(plain)
                for e, form in ((e40, R.FORM_40), (e8, R.FORM_HEAD)):
                    ht = _head_types(form)
                    want_narrow, want_wide = R.pack(tm, me, form, ht)
                    cap = len(want_wide) // 2
                    b = _Bufs(s2, off2, form, cap, 4 * n - 1)
                    narrow, wide, ge, go, c, n_wide = e.step_frames_packed(b.s, b.off, form, b.narrow, b.wide, b.ents, head_types=ht,
                                                                           tail_appends=tail_appends)
                    b.assert_canaries(form, cap, "short wide[]")
                    assert n_wide == len(want_wide) > cap == len(wide)
                    _same(go, to, "results with a short wide array")
                    _same(narrow, want_narrow, "narrow with a short wide array")
                    _same(wide, want_wide[:cap], "the wide records that fit")
                    _same(ge, te, "ents with a short wide array")
                    _assert_same_state(_state_of(e), want_state, "short wide[]")


@pytest.mark.parametrize("tail_appends", [True, False])
@pytest.mark.parametrize("N,me", [(3, 0), (5, 1)])
def test_step_frames_packed_equals_step_frames(oracle, N, me, tail_appends):
    from tests.test_wire_gpu import _node_frames

    _step_twins(N, me, tail_appends, lambda rng, n, st: _node_frames(rng, n, st, me))


def test_step_frames_packed_through_the_sorted_walk(oracle):
    """700 frames over four of the 64 groups: far more than 32 of one group, the list walk gives the batch up and the call
    replays it through the sorted walk, which reads the decoder's 64-byte copy in HBM a second time"""
    import types

    from tests.test_wire_gpu import _node_frames

    def hot(rng, n, st):
        few = types.SimpleNamespace(G=4, N=st.N, term=st.term, last_index=st.last_index, last_term=st.last_term)
        return _node_frames(rng, n, few, 0)

    from oracle import pywire

    s, off = hot(np.random.default_rng(1), 700, _stepgen_state())
    g = pywire.wire_decode(s, off)[0]["group"]
    assert int(np.bincount(g[g < 4].astype(np.int64)).max()) > 32  # (the input does hold a run longer than the list walk takes)
    _step_twins(3, 0, True, hot, n_calls=1)


def _stepgen_state():
    from tests import _stepgen

    return _stepgen.random_state(np.random.default_rng(2), 64, 3, self_peer=0)


# ---- refusals: nothing is applied ----------------------------------------------------------------------------------------------
def test_refusals_apply_nothing(oracle):
    from raftsql_amd import _lib
    from raftsql_amd import wire as W
    from raftsql_amd.engine import RaftqError, pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen
    from tests.test_wire_gpu import _node_frames

    rng = np.random.default_rng(77)
    st = _stepgen.random_state(rng, 64, 3, 0)
    s, off = _node_frames(rng, 100, st, 0)
    n = 100
    ps, po = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
    with WireEngine(64, 3, 0) as e:
        _stepgen.load_engine(e, st)
        before = _state_of(e)

        def refused(code, call):
            with pytest.raises(RaftqError) as ei:
                call()
            assert ei.value.code == code
            _assert_same_state(_state_of(e), before, "a refused call applied something")

        for form in FORMS:
            dt = W._FORM_DT[form]
            narrow, wide, ents = pinned_empty(n + 2, dt), pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(4 * n, W.WIRE_ENT_DT)
            odd8 = pinned_empty((n + 2) * form + 16, np.uint8)[8:8 + n * form].view(dt)  # page-locked, 8 bytes off a quad
            assert odd8.ctypes.data % 16 == 8
            odd_wide = pinned_empty(64 * n + 64, np.uint8)[8:8 + 64 * n].view(W.WIRE_MSG_DT)
            for step in (False, True):
                def call(stream=ps, o=po, f=form, nar=narrow, wd=wide, en=ents, to_slot=0):
                    if step:
                        return e.step_frames_packed(stream, o, f, nar, wd, en)
                    return e.wire_decode_packed(stream, o, f, to_slot, nar, wd, en)

                refused(_lib.RAFTQ_EINVAL, lambda: call(stream=np.ascontiguousarray(s)))  # pageable stream
                refused(_lib.RAFTQ_EINVAL, lambda: call(nar=np.zeros(n, dt)))  # pageable narrow array
                refused(_lib.RAFTQ_EINVAL, lambda: call(wd=np.zeros(n, W.WIRE_MSG_DT)))  # pageable wide array
                refused(_lib.RAFTQ_EINVAL, lambda: call(nar=odd8))  # misaligned
                refused(_lib.RAFTQ_EINVAL, lambda: call(wd=odd_wide))
                refused(_lib.RAFTQ_EINVAL, lambda: call(f=7))  # no such form
                refused(_lib.RAFTQ_EINVAL, lambda: call(f=64))
                if not step:
                    refused(_lib.RAFTQ_EINVAL, lambda: call(to_slot=255))
            # a batch in flight
            e.step_submit(_stepgen.random_batch(rng, st, 10))
            for step in (False, True):
                with pytest.raises(RaftqError) as ei:
                    if step:
                        e.step_frames_packed(ps, po, form, narrow, wide, ents)
                    else:
                        e.wire_decode_packed(ps, po, form, 0, narrow, wide, ents)
                assert ei.value.code == _lib.RAFTQ_ESTATE
            e.step_collect()
            before = _state_of(e)  # (the collected batch's)
        # and the calls work on that handle afterwards
        narrow, wide = pinned_empty(n, W.WIRE_MSG40_DT), pinned_empty(n, W.WIRE_MSG_DT)
        _, _, _, _, n_wide, rc = e.wire_decode_packed(ps, po, R.FORM_40, 0, narrow, wide, None)
        assert rc == 0 and 0 < n_wide < n
    with WireEngine(64, 3, 0, msg_flags=False) as e:  # raftq_step_frames' own precondition
        _stepgen.load_engine(e, st)
        with pytest.raises(RaftqError) as ei:
            e.step_frames_packed(ps, po, R.FORM_40, pinned_empty(n, W.WIRE_MSG40_DT), pinned_empty(n, W.WIRE_MSG_DT), None)
        assert ei.value.code == _lib.RAFTQ_ESTATE
