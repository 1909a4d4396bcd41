"""GPU: CheckQuorum (raftq_set_check_quorum; tick_check_kernel, the four rules in NodeT::step of every walk kernel) against
tests/ref_check_quorum.py: every result byte, every word of state, the activity arrays.

Tick shapes (the issue's): G in {5, 1027, 2500} -- a lone partial lane, one group past a 1,024-group block, three blocks and no
multiple of 4 --, N in {1, 3, 5, 9} (a bit above a byte), self in {0, N - 1}, election_tick in {1, 3, 10}, heartbeat_tick in
{1, 2}, 2 * election_tick ticks each, once over every slot and once over voter masks.  Step: G = 194 groups, batches of 512
records, N in {1, 3, 5, 9}; a batch with 40 records of one group (more than kMaxRun = 32: the sorted walk).  What each Step input
shows of the feature is asserted on the reference alone by tests/test_check_quorum_ref.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from oracle import pyoracle
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_raft_py as R
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

CASES = Q.case_list()
SEED = 0x5EED
_ids = lambda kw: "-".join(str(v) for v in kw.values())  # noqa: E731


def _band(band, masks=False):
    """the band case (64-bit terms and indices, tests/_widegen.py) of the list with this band"""
    return next(c for c in CASES if c.get("band") == band and bool(c.get("masks")) == masks)


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@functools.lru_cache(maxsize=None)
def _case(key):
    return Q.step_case(**dict(key))


def _key(kw):
    return tuple(sorted(kw.items()))


def _engine(S, s, voters, active, lead_elapsed, on=True, cls=None):
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer)
    _stepgen.load_engine(e, s)
    e.set_timers(Q.ELECTION_TICK, 1, SEED)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
    if on:
        e.set_check_quorum(True)
        e.load_activity(active, lead_elapsed)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), msgs[bad[0]], got[bad[0]], want[bad[0]])


def _same_after(e, after, what=""):
    s, active, lead_elapsed = after
    _stepgen.assert_same_state(e, s)
    a, le = e.read_activity()
    assert np.array_equal(a, active), (what, "active")
    assert np.array_equal(le, lead_elapsed), (what, "lead_elapsed")


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- Tick --------------------------------------------------------------------------------------------------------------------------
def _tick_engine(S, g, n, me, et, ht, role, el, ac, le, voters, on=True):
    e = S.NodeEngine(g, n, me)
    e.set_timers(et, ht, SEED)
    e.load_roles(role, el)
    if voters is not None:
        e.load_voters(voters)
        e.set_tick_voters(True)
    if on:
        e.set_check_quorum(True)
        e.load_activity(ac, le)
    return e


@pytest.mark.parametrize("masks", [False, True], ids=["all-slots", "masks"])
@pytest.mark.parametrize("n", [1, 3, 5, 9])
@pytest.mark.parametrize("g", [5, 1027, 2500])
def test_tick_against_the_reference(S, g, n, masks):
    for me, et, ht in itertools.product(sorted({0, n - 1}), (1, 3, 10), (1, 2)):
        what = (g, n, me, et, ht, masks)
        role, el, ac, le, voters = Q.tick_input(g, n, me, et, seed=9600 + 7 * g + 100 * n + 10 * et + ht + me, masks=masks)
        seen = set()
        with _tick_engine(S, g, n, me, et, ht, role, el, ac, le, voters) as e:
            prev_lost = None
            for t in range(2 * et):
                el, act, ac, le, n_hup, n_beat = Q.tick_array(pyoracle, role, el, ac, le, voters, me, n, et, ht, SEED, t)
                assert e.tick() == (n_hup, n_beat), (what, t)
                g_act, g_el, g_role = e.read_tick()
                assert np.array_equal(g_act, act) and np.array_equal(g_el, el) and np.array_equal(g_role, role), (what, t)
                g_ac, g_le = e.read_activity()
                assert np.array_equal(g_ac, ac) and np.array_equal(g_le, le), (what, t)
                for k, collect in ((1, e.collect_hups), (2, e.collect_beats), (3, e.collect_checks)):
                    ids, cnt = collect()
                    assert cnt == int((act == k).sum()) and np.array_equal(ids, np.flatnonzero(act == k)), (what, t, k)
                ids, cnt = e.collect_checks(cap=1)  # the count is the full one, the list is cut
                assert cnt == int((act == 3).sum()) and len(ids) == min(cnt, 1), (what, t)
                # a failing group raises no beat this tick, and -- the check not stepped -- raises it on the next
                if prev_lost is not None and et > 1:
                    assert np.all(act[prev_lost] == 2), (what, t)
                prev_lost = act == 3
                seen |= set(np.unique(act).tolist())
        if g >= 1000:
            assert seen >= ({0, 2} if n == 1 and not masks else {0, 1, 2, 3}), (what, seen)


def test_tick_switch_off_twin(S):
    """the same inputs with the switch off tick as they always did: the plain oracle, no action 3, an empty check list"""
    g, n, me, et, ht = 1027, 5, 4, 3, 1
    role, el, ac, le, _ = Q.tick_input(g, n, me, et, seed=9700)
    with _tick_engine(S, g, n, me, et, ht, role, el, ac, le, None, on=False) as e:
        for t in range(2 * et):
            el, act, n_hup, n_beat = pyoracle.tick(role, el, et, ht, SEED, t)
            assert e.tick() == (n_hup, n_beat)
            g_act, g_el, _ = e.read_tick()
            assert np.array_equal(g_act, act) and np.array_equal(g_el, el) and not (g_act == 3).any()
            ids, cnt = e.collect_checks()
            assert cnt == 0 and len(ids) == 0
            assert np.array_equal(e.collect_beats()[0], np.flatnonzero(act == 2))


# ---- Step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=_ids)
def test_step_batch_against_the_reference(S, kw):
    start, voters, m, want, after = _case(_key(kw))
    with _engine(S, start[0], voters, start[1], start[2]) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, kw)
        _same_after(e, after, kw)


@pytest.mark.parametrize("kw", [CASES[2], CASES[7], CASES[8], _band("b32", masks=True)], ids=_ids)
def test_step_packed_records_and_result_formats(S, kw):
    """the 40-byte inbound record takes type 12 too; the three result formats say the same -- around 2^32 too, where expand_short
    adds its 32-bit offsets to a last_index / committed on either side of the boundary"""
    start, voters, m, _, _ = _case(_key(kw))
    m40 = S.pack_msgs40(np.array(m))
    # what the device widens them to (include/raftq_step.h: a packed record carries no RAFTQ_MSGF_*, no count, one of log_term / reject_hint)
    m = np.zeros(len(m40), S.MSG_DT)
    for k in ("group", "from", "type", "reject", "term", "index", "commit"):
        m[k] = m40[k]
    hint = m40["type"] == S.MSG_APP_RESP
    m["log_term"], m["reject_hint"] = np.where(hint, 0, m40["aux"]), np.where(hint, m40["aux"], 0)
    after = (V.copy_state(start[0]), start[1].copy(), start[2].copy())
    want = Q.step_batch(after[0], voters, after[1], after[2], m)
    assert (want["type"][m["type"] == Q.MsgCheckQuorum] == S.OUT_NONE).all() and ((want["flags"] & S.OUTF_STEPPED_DOWN) != 0).any()
    for fmt in (0, 1, 2):
        with _engine(S, start[0], voters, start[1], start[2]) as e:
            e.set_compact(fmt)
            e.step_submit_packed(m40)
            recs, _ = e.step_collect()
            if fmt == 0:
                got = recs
            elif fmt == 1:
                got = S.expand_compact(np.array(m), recs)
            else:
                got = S.expand_short(np.array(m), recs, start[0].last_index, start[0].committed)
            _same_records(got, want, m, (kw, fmt))
            _same_after(e, after, (kw, fmt))


@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_step_both_walks(S, monkeypatch, walk):
    """a batch with 40 records of one group takes the sorted walk by itself; RAFTQ_STEP_WALK=sort sends every batch there"""
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)
    for kw in (CASES[8], CASES[9], _band("b63")):
        start, voters, m, want, after = _case(_key(kw))
        assert not kw.get("hot") or np.bincount(m["group"].astype(np.int64)).max() > 32
        with _engine(S, start[0], voters, start[1], start[2]) as e:
            got, _ = e.step_batch(np.array(m))
            _same_records(got, want, m, (kw, walk))
            _same_after(e, after, (kw, walk))


def test_pipelined_ack_saves_the_leader(S):
    """submit / collect with a check behind an acknowledgement of the same group in ONE batch: the ack must save the leader; and
    a second batch in flight behind it sees the cleared bits"""
    n, me, g = 3, 0, 64
    s = pyoracle.NodeState(g, n, me)
    s.role[:], s.term[:], s.lead[:], s.vote[:], s.last_index[:], s.last_term[:], s.first_idx[:] = 2, 4, me + 1, me + 1, 9, 4, 1
    s.match[me] = 9
    ac, le = np.zeros(g, np.uint16), np.full(g, 2, np.uint32)
    grp = np.arange(g, dtype=np.uint64)
    saved = grp[::2]
    b1 = np.concatenate([S.pack_msgs(saved, S.MSG_APP_RESP, term=4, frm=2, index=3, reject=1), S.pack_msgs(grp, S.MSG_CHECK_QUORUM)])
    b2 = S.pack_msgs(grp, S.MSG_CHECK_QUORUM)
    start = (V.copy_state(s), ac.copy(), le.copy())
    w1 = Q.step_batch(s, None, ac, le, b1)
    w2 = Q.step_batch(s, None, ac, le, b2)
    down = (w1["flags"] & R.FlagSteppedDown) != 0
    assert np.array_equal(np.unique(b1["group"][down]), grp[1::2]) and not down[:len(saved)].any()
    assert np.array_equal(np.flatnonzero((w2["flags"] & R.FlagSteppedDown) != 0), saved)  # the bits were cleared: the next check fails
    with _engine(S, start[0], None, start[1], start[2]) as e:
        e.step_submit(b1)
        e.step_submit(b2)
        code, _ = _code(e.read_activity)  # a state call while batches are in flight
        assert code == RAFTQ_ESTATE
        g1, _ = e.step_collect()
        g2, _ = e.step_collect()
        _same_records(g1, w1, b1, "first batch")
        _same_records(g2, w2, b2, "second batch")
        _same_after(e, (s, ac, le), "pipelined")


def test_frames_respond_builds_no_frame_for_a_lease_ignored_vote(S):
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WIRE_ENT_DT, WIRE_MSG_DT, WireEngine

    n, me, g = 3, 1, 8
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.lead[:], s.last_index[:], s.last_term[:] = 4, 3, 6, 4
    s.elapsed[:] = np.where(np.arange(g) % 2 == 0, 0, Q.ELECTION_TICK + 1)  # even groups in lease, odd ones out of it
    w = np.zeros(g, W.WIRE_MSG_DT)
    w["group"], w["type"], w["term"], w["from"], w["to"], w["index"], w["log_term"] = np.arange(g), R.MsgVote, 5, 0, me, 9, 5
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    for on in (True, False):
        with _engine(S, s, None, np.zeros(g, np.uint16), np.zeros(g, np.uint32), on=on, cls=WireEngine) as e:
            out, peer_off = pinned_empty(e.respond_cap(g), np.uint8), pinned_empty(n + 1, np.uint64)
            resp_off = pinned_empty(g * (n - 1) + 1, np.uint64)
            _, _, outs, _, _, _, _, rc = e.step_frames_respond(pinned_copy(stream), pinned_copy(off), pinned_empty(g, WIRE_MSG_DT), pinned_empty(4, WIRE_ENT_DT),
                                                               None, out, resp_off, peer_off)
            ignored = (np.arange(g) % 2 == 0) & on
            assert np.array_equal(outs["type"], np.where(ignored, S.OUT_NONE, S.OUT_VOTE_RESP)), on
            assert np.array_equal((outs["flags"] & 0x10) != 0, ~ignored), on  # RAFTQ_OUTF_ANSWERED: a frame was built
            assert np.array_equal(outs["term"], np.where(ignored, 4, 5)), on
            assert int(rc.n_msgs) == int((~ignored).sum()), on


def test_round_trip_tick_list_step_campaign(S):
    """Tick -> raftq_collect_checks -> Step(RAFTQ_MSG_CHECK_QUORUM) -> a stepped-down group campaigns on a later Tick"""
    n, me, g, et = 3, 0, 1027, 3
    s = pyoracle.NodeState(g, n, me)
    s.role[:], s.term[:], s.lead[:], s.vote[:], s.last_index[:], s.last_term[:], s.first_idx[:] = 2, 2, me + 1, me + 1, 5, 2, 1
    s.match[me] = 5
    ac = np.where(np.arange(g) % 3 == 0, 0, 0b010).astype(np.uint16)  # every third leader has heard from nobody
    le = np.full(g, et - 1, np.uint32)  # every check falls due on the first tick
    cut = np.flatnonzero(np.arange(g) % 3 == 0)
    with S.NodeEngine(g, n, me) as e:
        _stepgen.load_engine(e, s)
        e.set_timers(et, 1, SEED)
        e.set_check_quorum(True)
        e.load_activity(ac, le)
        assert e.tick() == (0, g - len(cut))
        ids, cnt = e.collect_checks()
        assert cnt == len(cut) and np.array_equal(ids, cut)
        late = ids[::2]  # half of them get an acknowledgement before the check is stepped
        batch = np.concatenate([S.pack_msgs(late, S.MSG_HEARTBEAT_RESP, term=2, frm=2), S.pack_msgs(ids, S.MSG_CHECK_QUORUM)])
        got, _ = e.step_batch(batch)
        chk = got[len(late):]
        down = np.isin(ids, late, invert=True)
        assert np.all(chk["type"] == S.OUT_NONE)
        assert np.array_equal(chk["flags"], np.where(down, S.OUTF_STEPPED_DOWN, 0))
        assert np.array_equal(chk["role"], np.where(down, 0, 2)) and np.array_equal(chk["lead"], np.where(down, 0, me + 1))
        assert np.all(chk["term"] == 2) and np.all(chk["vote"] == me + 1)
        gone = ids[down]
        hupped = np.zeros(g, bool)
        for _ in range(2 * et + 2):
            e.tick()
            h, _ = e.collect_hups()
            hupped[h.astype(np.int64)] = True
        assert np.array_equal(np.flatnonzero(hupped), gone)  # exactly the stepped-down groups' election timers have fired
        got, _ = e.step_batch(S.pack_msgs(gone, S.MSG_HUP))
        assert np.all(got["type"] == S.OUT_CAMPAIGN) and np.all(got["term"] == 3)


# ---- the switch off, and what the switch closes ------------------------------------------------------------------------------------
def test_step_switch_off_twin(S):
    """without the switch the same traffic minus type 12 steps as the C oracle says; type 12 fails its batch and applies nothing"""
    start, voters, m, want, after = _case(_key(CASES[2]))
    m = np.array(m)
    plain = m[m["type"] != Q.MsgCheckQuorum]
    s = V.copy_state(start[0])
    want_plain = s.step_batch(plain)
    with _engine(S, start[0], None, None, None, on=False) as e:
        code, text = _code(e.step_batch, m)
        assert code == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, start[0])
        got, _ = e.step_batch(plain)
        _same_records(got, want_plain, plain, "switch off")
        _stepgen.assert_same_state(e, s)
        e.tick()
        assert e.collect_checks()[1] == 0
    assert want_plain.tobytes() != Q.step_batch(V.copy_state(start[0]), None, start[1].copy(), start[2].copy(), plain).tobytes()  # (the switch matters here)


def test_refusals_and_argument_checks(S):
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine, SweepSet

    g, n = 100, 3
    with S.NodeEngine(g, n, 1) as e:
        lib, h = e._lib, e._h
        # switch off: the activity calls have no state to speak of, the list is empty
        for f in (lambda: e.load_activity(np.zeros(g, np.uint16), None), e.read_activity):
            code, text = _code(f)
            assert code == RAFTQ_ESTATE and "raftq_set_check_quorum is off" in text
        assert _code(e.set_check_quorum, 2)[0] == RAFTQ_EINVAL
        e.set_timers(70000, 1, 1)
        code, text = _code(e.set_check_quorum, True)
        assert code == RAFTQ_EINVAL and "65535" in text
        e.set_timers(10, 1, 1)
        e.set_check_quorum(True)
        a, le = e.read_activity()
        assert not a.any() and not le.any()  # allocated zeroed
        code, text = _code(e.set_timers, 65536, 1, 1)
        assert code == RAFTQ_EINVAL and "65535" in text
        e.set_timers(65535, 1, 1)
        e.set_timers(10, 1, 1)
        bad = np.zeros(g, np.uint16)
        bad[g - 1] = 1 << n
        assert _code(e.load_activity, bad, None)[0] == RAFTQ_EINVAL
        assert _code(e.load_activity, None, np.full(g, 65536, np.uint32))[0] == RAFTQ_EINVAL
        assert not e.read_activity()[0].any()  # nothing loaded
        e.load_activity(np.full(g, 0b101, np.uint16), None)
        e.load_activity(None, np.full(g, 7, np.uint32))  # either half alone
        a, le = e.read_activity()
        assert np.all(a == 0b101) and np.all(le == 7)
        # the five calls the switch closes, each with "check quorum" in the text
        nh, nb = C.c_uint64(0), C.c_uint64(0)
        po = (C.c_uint64 * 16)()
        calls = {
            "raftq_tick_collect": lambda: lib.raftq_tick_collect(h, None, 0, C.byref(nh), None, 0, C.byref(nb)),
            "raftq_tick_collect_lists": lambda: lib.raftq_tick_collect_lists(h, 0, 0, 0, C.byref(nh), C.byref(nb)),
            "raftq_tick_frames": lambda: lib.raftq_tick_frames(h, 0, 0, 0, C.byref(nh), C.byref(nb), None, 0, None, po, None),
            "raftq_tick_elect_frames": lambda: lib.raftq_tick_elect_frames(h, 0, 0, 0, C.byref(nh), C.byref(nb), None, None, 0, None, po, None),
        }
        e.load_roles(np.full(g, 2, np.uint8))
        before = e.read_tick()
        for name, call in calls.items():
            assert call() == RAFTQ_ESTATE, name
            text = lib.raftq_last_error(h).decode()
            assert "check quorum" in text and name in text, (name, text)
        with QuorumEngine(g, n) as other, SweepSet([e, other]) as ss:
            with pytest.raises(RaftqError) as ei:
                ss.tick()
            assert ei.value.code == RAFTQ_ESTATE and "check quorum" in str(ei.value)
        for x, y in zip(before, e.read_tick()):
            assert np.array_equal(x, y)  # none of them ticked
        # the clone copies the arrays when both handles hold them, never the switch
        with S.NodeEngine(g, n, 1) as d:
            d.clone_state_from(e)
            assert _code(d.read_activity)[0] == RAFTQ_ESTATE
            d.set_check_quorum(True)
            d.clone_state_from(e)
            a, le = d.read_activity()
            assert np.all(a == 0b101) and np.all(le == 7)
        e.set_check_quorum(False)
        assert _code(e.read_activity)[0] == RAFTQ_ESTATE
        e.set_check_quorum(True)
        assert not e.read_activity()[0].any() and not e.read_activity()[1].any()  # zeroed again
    # the Tick needs to know self, masks or not
    with QuorumEngine(g, n) as q:
        q.set_check_quorum(True)
        q.load_roles(np.full(g, 2, np.uint8))
        code, text = _code(q.tick)
        assert code == RAFTQ_ESTATE and "raftq_set_self" in text
        assert _lib.load().raftq_set_self(q._h, 0) == 0
        assert q.tick() == (0, g)
