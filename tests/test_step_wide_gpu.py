"""GPU: the Step family at 64-bit terms and indices, byte for byte against the references that are uint64 throughout -- the C
oracle, oracle/pywire, the Python restatements of the respond / lead / members rules.  Every test runs in the three bands of
tests/_widegen.py: tails within +-6 of 2^32 (a 32-bit temporary loses the carry), the same around 2^63 (a signed compare turns
round), and [2^64 - 2^12, 2^64 - 2^11) (bit 63 set everywhere, ten-byte varints).  tests/test_widegen.py shows on the CPU that
these inputs tell a narrow Step from a wide one.

Shapes: G = 3,000, or 4,099 (two 2,048-group tiles and a ragged third) where a sweep follows; at most 9,000 messages a batch;
every third batch on 30 groups, which gives runs of ~300 messages and so the stall replay through the sorted walk."""
import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd import _lib
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_bcast_members as B
from tests import ref_respond_lead as L
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

U = np.uint64
BANDS = WG.BAND_NAMES


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@pytest.fixture(scope="module")
def WireEngine(gpu_engine_cls):
    from raftsql_amd.wire import WireEngine

    return WireEngine


def _walk(monkeypatch, walk):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)


def _same64(got, want, msgs, what):
    assert got.dtype.itemsize == want.dtype.itemsize == 64 and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), msgs[bad[0]], got[bad[0]], want[bad[0]])


def _edge(band):
    """the value the hand-made cases are placed around: B, or a point inside the top band"""
    return WG.TOP_LO + 64 if band == "top" else WG.BANDS[band]


# ---- raftq_step_batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("N,me", WG.STEP_SHAPES)
@pytest.mark.parametrize("band", BANDS)
def test_step_wide(S, oracle, band, N, me, walk, monkeypatch):
    """ten batches of 9,000 through raftq_step_batch with full 64-byte results: every record is the oracle's, and every word of
    state at the end"""
    _walk(monkeypatch, walk)
    start, batches, final = WG.step_run(band, N, me)
    with S.NodeEngine(WG.STEP_G, N, me) as e:
        _stepgen.load_engine(e, start)
        _stepgen.assert_same_state(e, start)
        for it, (m, want, _, _) in enumerate(batches):
            got, touched = e.step_batch(m)
            assert touched == len(np.unique(m["group"]))
            _same64(got, want, m, (band, N, walk, it))
        _stepgen.assert_same_state(e, final)


@pytest.mark.parametrize("compact", [0, 1, 2], ids=["64-byte-results", "40-byte-results", "32-byte-results"])
@pytest.mark.parametrize("band", BANDS)
def test_step_wide_pipelined(S, oracle, band, compact):
    """step_submit / step_collect with two batches in flight, RAFTQ_MSGF_HOLD / RAFTQ_MSGF_SKIP on every other batch, in the
    three result formats (the narrow ones expanded as tests/test_step_gpu.py expands them)"""
    N, me = 5, 4
    start, batches, final = WG.step_run(band, N, me, True)
    with S.NodeEngine(WG.STEP_G, N, me) as e:
        _stepgen.load_engine(e, start)
        e.set_compact(compact)

        def collect(it):
            m, want, before, _ = batches[it]
            got, touched = e.step_collect()
            if compact == 2:
                assert got.dtype == S.OUT_S_DT
                _same64(S.expand_short(m, got, *before), want, m, (band, compact, it))
            elif compact == 1:
                assert got.dtype == S.OUT_C_DT
                live = want["type"] != S.OUT_SKIPPED  # (a 40-byte record names no group: a skipped one's is garbage by definition)
                _same64(S.expand_compact(m, got)[live], want[live], m[live], (band, compact, it))
                assert (got["type"][~live] == S.OUT_SKIPPED).all()
            else:
                _same64(got, want, m, (band, compact, it))

        for it in range(len(batches)):
            e.step_submit(batches[it][0])
            if it >= 1:
                collect(it - 1)
        collect(len(batches) - 1)
        _stepgen.assert_same_state(e, final)


@pytest.mark.parametrize("band", BANDS)
def test_step_wide_packed_inbound(S, oracle, band):
    """raftq_step_submit_packed: the 40-byte inbound records carry the same 64-bit term / index / aux / commit"""
    from tests.test_step_gpu import _widened

    N, me, G = 5, 2, WG.STEP_G
    rng = np.random.default_rng(21000 + BANDS.index(band))
    s = WG.lift(_stepgen.random_state(rng, G, N, me), band, rng)
    with S.NodeEngine(G, N, me) as e:
        _stepgen.load_engine(e, s)
        prev = None
        for it in range(6):
            m = WG.wide_batch(rng, s, 9000, hot_groups=rng.choice(G, 30, replace=False) if it % 3 == 2 else None)
            want = s.step_batch(_widened(m))
            e.step_submit_packed(S.pack_msgs40(m))
            if prev is not None:
                _same64(e.step_collect()[0], prev[1], prev[0], (band, it - 1))
            prev = (m, want)
        _same64(e.step_collect()[0], prev[1], prev[0], (band, "last"))
        _stepgen.assert_same_state(e, s)


# ---- the hand tables, lifted (tests/test_widegen.py holds the oracle to them) ------------------------------------------------------
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("table", ["tail_append", "barrier", "hold_skip", "alias"])
@pytest.mark.parametrize("band", BANDS)
def test_hand_tables_wide(S, oracle, band, table, walk, monkeypatch):
    _walk(monkeypatch, walk)
    if table == "tail_append":
        s, m, want = WG.lifted_tail_append_table(band)
    elif table == "alias":
        s, m, want, after, match_row = WG.alias_table(band)
    else:
        s, m, want, after = (WG.lifted_barrier_table if table == "barrier" else WG.lifted_hold_skip_table)(band)
    with S.NodeEngine(s.G, s.N, s.self_peer) as e:
        _stepgen.load_engine(e, s)
        ref = s.step_batch(m)
        got, _ = e.step_batch(m)
        _same64(got, ref, m, (band, table, walk))
        if table == "tail_append":
            _stepgen.check_tail_append_table(got, s, want)
        elif table == "alias":
            assert [int(t) for t in got["type"]][:2] == want[:2]
            node = e.read_node()
            for k, v in after.items():
                assert [int(x) for x in node[k]] == v, k
            assert [int(x) for x in e.read_match()[:, 2]] == match_row
        else:
            assert [int(t) for t in got["type"]] == want
            node = e.read_node()
            for k, v in after.items():
                assert [int(x) for x in node[k]] == v, k
        _stepgen.assert_same_state(e, s)


# ---- raftq_apply_log_deltas / _nowait ----------------------------------------------------------------------------------------------
def _delta_state(band, G, N, me):
    """by hand, around E = the band's edge: g % 3 == 0 a leader at term E + 1 whose log ends at (E - 2, E + 1), committed E - 5,
    the gate first_idx at E - 4 (even g) or E + 1 (odd g), one follower's Match at E - 2 - g % 4 and the others' at E - 6;
    the rest followers ending at (E - 2, E - 1), committed E - 4.  -> (NodeState, the reports)"""
    from oracle import pyoracle

    E = _edge(band)
    s = pyoracle.NodeState(G, N, me)
    g = np.arange(G)
    led = g % 3 == 0
    s.role[:] = np.where(led, 2, 0)
    s.term[:] = E + 1
    s.last_index[:] = E - 2
    s.last_term[:] = np.where(led, U(E + 1), U(E - 1))
    s.committed[:] = np.where(led, U(E - 5), U(E - 4))
    s.vote[:] = s.lead[:] = np.where(led, me + 1, (me + 1) % N + 1)
    s.first_idx[:] = np.where(led, np.where(g % 2 == 0, U(E - 4), U(E + 1)), U(0))
    for p in range(N):
        s.match[p] = np.where(led, U(E - 6), U(0))
    if N > 1:
        s.match[(me + 1) % N] = np.where(led, U(E - 2) - (g % 4).astype(U), U(0))
    s.match[me] = s.last_index
    # the reports: a leader's tail moves from E - 2 to E + 3; a follower's with commit_to E + 1 (g % 3 == 1: across E) or none
    li = np.full(G, E + 3, U)
    lt = s.term.copy()
    ct = np.where(g % 3 == 1, U(E + 1), U(0))
    return s, (g.astype(U), li, lt, ct)


@pytest.mark.parametrize("nowait", [False, True], ids=["waiting", "nowait"])
@pytest.mark.parametrize("band", BANDS)
def test_log_deltas_wide(S, oracle, band, nowait):
    E = _edge(band)
    for N, me in ((3, 1), (1, 0)):
        G = 3000
        s, rep = _delta_state(band, G, N, me)
        p = np.random.default_rng(3).permutation(G)
        rep = tuple(a[p] for a in rep)
        with S.NodeEngine(G, N, me) as e:
            _stepgen.load_engine(e, s)
            _stepgen.assert_same_state(e, s)
            want = s.apply_log_deltas(*rep)
            if nowait:
                e.apply_log_deltas_nowait(*rep)
            else:
                assert np.array_equal(e.apply_log_deltas(*rep), want), (band, N)
            _stepgen.assert_same_state(e, s)
        # known answers: a follower's commit_to crosses E; a leader commits what its quorum holds, if the gate lets it -- and a
        # one-peer handle its own append
        g = np.arange(G)
        assert (s.last_index == U(E + 3)).all()
        assert (s.committed[g % 3 == 1] == U(E + 1)).all() and (s.committed[g % 3 == 2] == U(E - 4)).all()
        led_open, led_shut = (g % 3 == 0) & (g % 2 == 0), (g % 3 == 0) & (g % 2 == 1)
        if N == 1:
            assert (s.committed[led_open] == U(E + 3)).all() and (s.committed[led_shut] == U(E + 3)).all()
        else:
            mci = U(E - 2) - (g % 4).astype(U)
            assert np.array_equal(s.committed[led_open], np.where(mci >= U(E - 4), mci, U(E - 5))[led_open])
            assert (s.committed[led_shut] == U(E - 5)).all()


# ---- Step, then the dense sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS)
def test_step_wide_then_dense_sweep(S, oracle, band):
    """after Step has moved the wide Match rows: the sweep, plain and gated, is the oracle's commit_advance / vote_tally on the
    oracle's state, whichever body it took -- the rows or, after narrow_rebuild(), the 32-bit mirror if the device holds one"""
    G, N, me = 4099, 5, 0
    rng = np.random.default_rng(22000 + BANDS.index(band))
    s = WG.lift(_stepgen.random_state(rng, G, N, me), band, rng)
    flags = _lib.SWEEP_COMMIT | _lib.SWEEP_VOTES | _lib.SWEEP_CHANGED | _lib.SWEEP_NO_ADOPT
    with S.NodeEngine(G, N, me) as e:
        _stepgen.load_engine(e, s)
        for it in range(3):
            m = WG.wide_batch(rng, s, 9000)
            _same64(e.step_batch(m)[0], s.step_batch(m), m, (band, it))
        oc, won, lost = oracle.vote_tally(s.votes)
        for rebuilt in (False, True):
            if rebuilt:
                e.narrow_rebuild()
            for gated in (False, True):
                want, n_changed = oracle.commit_advance(s.match, s.committed, gated, s.first_idx)
                c = e.sweep(flags | (_lib.SWEEP_GATED if gated else 0))
                what = (band, "gated" if gated else "plain", "rebuilt" if rebuilt else "as left by Step", "narrow() = %s" % e.narrow())
                got = e.read_committed()
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, (what, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), s.match[:, bad[0]])
                assert (c.n_changed, c.n_won, c.n_lost) == (n_changed, won, lost), what
                assert np.array_equal(e.read_outcome(), oc), what
                adv, n_adv = e.collect_changed()
                moved = np.flatnonzero(want != s.committed)
                assert n_adv == len(moved) and np.array_equal(adv["group"], moved.astype(U)), what
                assert np.array_equal(adv["old_commit"], s.committed[moved]) and np.array_equal(adv["new_commit"], want[moved]), what
        # NO_ADOPT: the sweeps left the live state alone (their what-if is what read_committed showed) -- Step goes on from it
        m = WG.wide_batch(rng, s, 9000)
        _same64(e.step_batch(m)[0], s.step_batch(m), m, (band, "behind the sweeps"))
        _stepgen.assert_same_state(e, s)


# ---- frames in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("tail_appends", [True, False])
@pytest.mark.parametrize("band", BANDS)
def test_step_frames_wide(S, WireEngine, oracle, band, tail_appends, walk, monkeypatch):
    """raftq_step_frames over frames whose varints are five to ten bytes long: tests/test_wire_gpu.py's check"""
    from tests.test_wire_gpu import _check_step_frames

    _walk(monkeypatch, walk)
    G, N, me = 3000, 5, 2
    rng = np.random.default_rng(23000 + 10 * BANDS.index(band) + tail_appends)
    st = WG.lift(_stepgen.random_state(rng, G, N, me), band, rng)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        types = set()
        for it, n in enumerate([1, 257, 9000, 700]):
            s, off = WG.wide_node_frames(rng, n, st, me)
            types |= _check_step_frames(e, st, s, off, tail_appends, f"{band} call {it}")
        assert {S.OUT_SKIPPED, S.OUT_HELD, S.OUT_DEFERRED} <= types and (not tail_appends or S.OUT_APPENDED in types)
        _stepgen.assert_same_state(e, st)


@pytest.mark.parametrize("band", BANDS)
def test_step_frames_packed_wide(S, WireEngine, oracle, band):
    """raftq_step_frames_packed, 40-byte form: the results are the oracle's, the narrow and wide records are what the rule's
    Python statement makes of the oracle's decode, and they expand to it"""
    from raftsql_amd import wire as PW
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests import packed_rule as R
    from tests.test_wire_gpu import _node_filter, _same

    G, N, me = 3000, 3, 1
    rng = np.random.default_rng(23500 + BANDS.index(band))
    st = WG.lift(_stepgen.random_state(rng, G, N, me), band, rng)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        for it, n in enumerate([513, 6000]):
            s, off = WG.wide_node_frames(rng, n, st, me)
            wm, we, _ = W.wire_decode(s, off)
            want_m, rec = _node_filter(wm, we, G, N, me, True)
            want_o = st.step_batch(rec)
            want_narrow, want_wide = R.pack(want_m, me, R.FORM_40)
            assert 0 < len(want_wide) < n
            narrow, wide = pinned_empty(n, PW._FORM_DT[R.FORM_40]), pinned_empty(len(want_wide), W.WIRE_MSG_DT)
            ents = pinned_empty(len(we) + 1, W.WIRE_ENT_DT)
            gn, gw, ge, go, c, n_wide = e.step_frames_packed(pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, U)),
                                                             R.FORM_40, narrow, wide, ents)
            what = f"{band} call {it}"
            _same(go, want_o, what + " results")
            assert (c.n_msgs, c.n_ents, c.bytes) == (n, len(we), len(s)) and n_wide == len(want_wide), what
            _same(ge, we, what + " entry headers")
            _same(gn, want_narrow, what + " narrow")
            _same(gw, want_wide, what + " wide")
            _same(PW.expand_packed(gn, gw, me, R.FORM_40), R.delivered(want_m, me, R.FORM_40), what + " expansion")
        _stepgen.assert_same_state(e, st)


# ---- frames out: raftq_step_frames_respond -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,me", [(3, 1), (5, 2)])
@pytest.mark.parametrize("band", BANDS)
def test_respond_wide(WireEngine, oracle, band, N, me):
    """random traffic with a leaders' bitmap: tests/test_respond_gpu.py's check, the restated table over the oracle's results"""
    from tests.test_respond_gpu import _check, _leaders_bitmap

    G = 3000
    rng = np.random.default_rng(24000 + 10 * BANDS.index(band) + N)
    st = WG.lift(_stepgen.random_state(rng, G, N, me), band, rng)
    answered = frames = 0
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        for it, n in enumerate([257, 9000, 1000]):
            s, off = WG.wide_node_frames(rng, n, st, me)
            a, f = _check(e, st, s, off, _leaders_bitmap(rng, st), it != 2, f"{band} N={N} call {it}", resp_off=it != 0)
            answered, frames = answered + a, frames + f
        _stepgen.assert_same_state(e, st)
    assert answered > 100 and frames > answered


@pytest.mark.parametrize("N,me", [(3, 0), (5, 2)])
@pytest.mark.parametrize("band", BANDS)
def test_respond_lead_wide(oracle, band, N, me):
    """raftq_respond_set_lead: becomeLeader's broadcast -- Index lastIndex - 1, the empty entry at (Term, lastIndex) -- against
    tests/ref_respond_lead.py"""
    from tests.test_respond_gpu import _leaders_bitmap
    from tests.test_respond_lead_gpu import _check, _engine

    G = 3000
    rng = np.random.default_rng(24500 + 10 * BANDS.index(band) + N)
    small, cands, granters = L.one_grant_short(rng, G, N, me)
    st = WG.lift(small, band, rng)
    wins = []
    with _engine(st) as e:
        for it, (n_noise, n_grants, n_acks) in enumerate(((255, 150, 80), (6000, 300, 200))):
            s, off = WG.wide_lead_call(rng, st, cands, granters, n_noise, n_grants, n_acks)
            w = _check(e, st, s, off, _leaders_bitmap(rng, st), f"{band} N={N} call {it}", resp_off=it != 0)
            wins.append(len(w["wins"]))
    assert min(wins) >= 20, wins


@pytest.mark.parametrize("band", BANDS)
def test_respond_lead_over_members_wide(oracle, band):
    """the same with voter masks loaded and raftq_bcast_set_voters on: the win is a quorum of the group's own voters and the
    broadcast goes to its members"""
    from tests.test_respond_gpu import _leaders_bitmap
    from tests.test_respond_lead_gpu import _check, _engine

    G, N, me = 3000, 5, 1
    rng = np.random.default_rng(24800 + BANDS.index(band))
    voters = V.random_masks(rng, N, G)
    small, cands, granters = L.one_grant_short(rng, G, N, me, voters)
    st = WG.lift(small, band, rng)
    wins = []
    with _engine(st, voters=voters) as e:
        for it, (n_noise, n_grants, n_acks) in enumerate(((2000, 150, 100), (3000, 150, 100))):
            s, off = WG.wide_lead_call(rng, st, cands, granters, n_noise, n_grants, n_acks)
            w = _check(e, st, s, off, _leaders_bitmap(rng, st), f"{band} call {it}", voters, resp_off=it != 0)
            wins.append(len(w["wins"]))
    assert min(wins) >= 20, wins


@pytest.mark.parametrize("band", BANDS)
def test_every_result_a_commit_broadcast_fills_the_cap_it_can_reach(WireEngine, oracle, band):
    """N = 3, every group led here, one committing ack per group, every at-tail bit set: every result is a commit broadcast to
    both followers whose Term, Index, LogTerm and Commit take ten varint bytes each in b63 and top (five in b32).  The call gets
    exactly respond_cap(n) bytes of a buffer 64 bytes longer; the tail keeps its 0xEE.  A frame is RAFTQ_RESPOND_FRAME_MAX bytes
    less what its varints fall short of ten: in b63 and top only the group id does, so the total is
    n * (N - 1) * (RAFTQ_RESPOND_FRAME_MAX - 10 + len(varint(group))).  No reachable group id takes ten bytes (a handle has fewer
    than 2^32 groups), so the bound itself is never reached."""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import RESPOND_FRAME_MAX
    from tests.test_respond_gpu import ANSWERED, _bitmap, _leader_state, expected
    from tests.test_wire_gpu import _node_filter

    G, N, me = 4099, 3, 0
    E = _edge(band)
    last, term = E + 2, E + 1
    st = _leader_state(G, N, me, last=10, term=3)
    st = WG.shift(st, U(term - 3), U(last - 10))
    assert (st.last_index == U(last)).all() and (st.committed == U(last - 2)).all() and (st.first_idx == U(last - 9)).all()
    rng = np.random.default_rng(25000)
    m = np.zeros(G, W.WIRE_MSG_DT)
    m["group"] = rng.permutation(G)
    m["type"], m["term"], m["index"], m["to"] = 4, term, last, me
    m["from"] = 1 + rng.integers(0, 2, G)
    s, off = W.wire_encode(m)
    at = _bitmap(G, np.arange(G))
    n = G
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        cap = e.respond_cap(n)
        assert cap == n * (N - 1) * RESPOND_FRAME_MAX
        buf = pinned_empty(cap + 64, np.uint8)
        buf[:] = 0xEE
        msgs, po = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(N + 1, U)
        ro = pinned_empty(n * (N - 1) + 1, U)
        gm, ge, go, got_s, got_off, got_po, c, rc = e.step_frames_respond(
            pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, U)), msgs, None, pinned_copy(at), buf[:cap], ro, po)
        wm, we, _ = W.wire_decode(s, off)
        _, rec = _node_filter(wm, we, G, N, me, True)
        lt0 = st.last_term.copy()
        want_o = st.step_batch(rec)
        assert (want_o["type"] == 5).all() and ((want_o["flags"] & 2) != 0).all() and (want_o["commit"] == U(last)).all()
        want_w, want_po, want_ans = expected(rec, want_o, lt0, at, N, me)
        assert want_ans.all() and len(want_w) == n * (N - 1) and (want_w["type"] == 3).all()
        for k, v in (("term", term), ("index", last), ("log_term", term), ("commit", last)):
            assert (want_w[k] == U(v)).all(), k
        want_s, want_off = W.wire_encode(want_w)
        assert ((go["flags"] & ANSWERED) != 0).all()
        assert bytes(got_s) == bytes(want_s) and np.array_equal(got_off, want_off) and np.array_equal(got_po, want_po)
        assert rc.n_msgs == n * (N - 1) and rc.bytes == len(want_s)
        assert bytes(buf[cap:]) == b"\xee" * 64 and bytes(buf[len(want_s):cap]) == b"\xee" * (cap - len(want_s))
        vl = lambda v: max(1, (int(v).bit_length() + 6) // 7)  # noqa: E731
        short = sum(10 - vl(v) for v in (term, last, term, last))  # 0 in b63 and top
        total = sum((N - 1) * (RESPOND_FRAME_MAX - 10 + vl(g) - short) for g in range(G))
        if band != "b32":
            assert short == 0
        assert len(got_s) == total, (len(got_s), total)
        _stepgen.assert_same_state(e, st)


# ---- proposals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,me,n_props,n_host", [(3, 2, 700, 300), (5, 1, 2000, 0)])
@pytest.mark.parametrize("band", BANDS)
def test_propose_frames_wide(oracle, band, N, me, n_props, n_host):
    """raftq_propose_frames with every tail within 3 below B, so that a record's entries cross it inside one MsgApp, and one
    record of 1,024 entries: tests/test_wire_gpu.py's check -- stream, offsets, counts, the state after, the 0xEE tail, and the
    quorum's acks committing the new tail"""
    from tests.test_wire_gpu import _check_propose

    G = 8192
    rng = np.random.default_rng(26000 + 10 * BANDS.index(band) + N)
    _check_propose(G, N, me, *WG.wide_propose_setup(rng, band, G, N, me, n_props, n_host))


# ---- over members --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("band", BANDS)
def test_step_voters_wide(S, band, walk, monkeypatch):
    """raftq_step_set_voters, N = 5, random masks with the edge cases planted: every result byte and every state word against
    tests/ref_step_voters.py, tail reports between the batches"""
    from tests.test_step_voters_gpu import _engine, _leaky_state, _tail_reports

    _walk(monkeypatch, walk)
    n, me, G = 5, 4, 3000
    rng = np.random.default_rng(27000 + BANDS.index(band))
    small, voters = _leaky_state(rng, G, n, me)
    s = WG.lift(small, band, rng)
    with _engine(S, V.copy_state(s), voters) as e:
        for rnd in range(3):
            m = WG.wide_batch(rng, s, 5000, hot_groups=rng.choice(G, 30, replace=False) if rnd == 1 else None)
            want = V.step_batch(s, voters, m)
            got, touched = e.step_batch(m)
            assert touched == len(np.unique(m["group"]))
            _same64(got, want, m, (band, walk, rnd))
            _stepgen.assert_same_state(e, s)
            rep = _tail_reports(rng, s)
            WG.guard(rep[1], rep[3])
            assert np.array_equal(e.apply_log_deltas(*rep), V.apply_log_deltas(s, voters, *rep)), rnd
            _stepgen.assert_same_state(e, s)


@pytest.mark.parametrize("band", BANDS)
def test_bcast_voters_respond_wide(WireEngine, band):
    """raftq_bcast_set_voters, the commit broadcast over members: tests/test_bcast_members_gpu.py's check against
    tests/ref_bcast_members.py"""
    from tests.test_bcast_members_gpu import _check_call, _engine

    G, N, me = 3000, 5, 2
    rng = np.random.default_rng(28000 + BANDS.index(band))
    small, voters, planted = B._respond_start(rng, G, N, me)
    st = WG.lift(small, band, rng)
    with _engine(WireEngine, V.copy_state(st), voters) as e:
        n_bcasts = 0
        for it, n in enumerate([257, 6000]):
            s, off = WG.wide_node_frames(rng, n, st, me)
            at_tail = B.leaders_bitmap(rng, st) | B.bitmap(G, planted[st.role[planted] == 2])
            ta = it == 1
            want = B.respond_want(st, voters, s, off, at_tail, ta)
            n_bcasts += len(want[6])
            _check_call(e, dict(s=s, off=off, at_tail=at_tail, tail_appends=ta, want=want, after=st), f"{band} call {it}", resp_off=it != 0)
        assert n_bcasts >= 20, n_bcasts


@pytest.mark.parametrize("band", BANDS)
def test_bcast_voters_propose_wide(WireEngine, band):
    """raftq_bcast_set_voters, bcastAppend over members, with the tails of tests/_widegen.wide_propose_setup"""
    from tests.test_bcast_members_gpu import _check_propose_members

    G, N, me = 8192, 5, 1
    rng = np.random.default_rng(29000 + BANDS.index(band))
    d, props, pe, pool, hm, he = WG.wide_propose_setup(rng, band, G, N, me, 1500, 200)
    s = B.propose_state(d, N, me)
    voters = B.propose_masks(rng, N, G, me, props["group"])
    _check_propose_members(WireEngine, s, voters, props, pe, pool, hm, he)
