"""GPU: raftq_respond_set_lead (include/raftq_wire.h) -- raftq_step_frames_respond answers RAFTQ_OUT_BECAME_LEADER with becomeLeader's
broadcast, built on the device: the *_lead_kernel walks, resp_scatter_lead_kernel (over members: resp_scatter_lead_voters_kernel) and the entry headers in the encoder's input.

The expected frames come from tests/ref_respond_lead.py -- tests/test_respond_gpu.py::expected with the new rule restated from the
header -- run over the oracle's Step results and marshalled by oracle/pywire.  Everything but "switch off" fails on a tree without
the switch.

One case of the request has no input: "a win behind a result that ended the prefix".  Only MsgHup makes a candidate, frames carry
no MsgHup (the decoder skips it), and of what a candidate can be sent and stay a candidate -- MsgVote, MsgVoteResp, MsgAppResp,
MsgHeartbeatResp -- nothing ends the prefix; a MsgProp does, and holds every later frame of its group (RAFTQ_OUT_DEFERRED: not
stepped).  test_a_grant_behind_a_held_frame_wins_nothing pins that down; the rule itself is the `if (!host_owns)` around the walk's
table and the `if not s[1]` around the restatement's."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from tests import ref_respond_lead as L
from tests import ref_step_voters as V
from tests.test_respond_gpu import _bitmap, _call, _leaders_bitmap
from tests.test_respond_gpu import expected as expected_off
from tests.test_wire_gpu import _node_filter, _node_frames, _same

pytestmark = pytest.mark.gpu

ANSWERED = L.ANSWERED
WIN_FLOOR = 40  # wins the oracle must find in every random call (the seeds below were chosen on the CPU to meet it)


def _engine(st, lead=True, voters=None):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    e = WireEngine(st.G, st.N, st.self_peer)
    _stepgen.load_engine(e, st)
    if voters is not None:
        e.load_voters(voters)
        e.set_bcast_voters(True)
    if lead:
        e.set_respond_lead(True)
    return e


def _check(e, st, s, off, at_tail, what, voters=None, tail_appends=True, resp_off=True):
    """one call against the oracle + the restatement; st (the oracle state) moves with it -> the reference's dict"""
    from tests import _stepgen

    w = L.want(st, s, off, at_tail, voters, tail_appends)
    gm, ge, go, got_s, got_off, got_po, c, rc = _call(e, s, off, len(w["ents"]), at_tail, tail_appends, resp_off=resp_off)
    n = len(off) - 1
    assert (c.n_msgs, c.n_ents, c.bytes) == (n, len(w["ents"]), len(s)), what
    _same(gm, w["m"], f"records, {what}")
    _same(ge, w["ents"], f"entry headers, {what}")
    ans = (go["flags"] & ANSWERED) != 0
    assert np.array_equal(ans, w["answered"]), (what, np.nonzero(ans != w["answered"])[0][:10])
    go = go.copy()
    go["flags"] &= np.uint8(~ANSWERED & 0xFF)
    _same(go, w["outs"], f"results, {what}")
    assert np.array_equal(got_po, w["peer_off"]), (what, got_po, w["peer_off"])
    assert rc.n_msgs == w["n_frames"] and rc.bytes == len(w["stream"]), what
    assert bytes(got_s) == bytes(w["stream"]), what
    if resp_off:
        assert np.array_equal(got_off, w["off"]), what
    _stepgen.assert_same_state(e, st)
    w["got"] = (go, W.wire_decode(got_s, got_off) if resp_off and len(got_s) else None, got_po)
    return w


# ---- the directed cases ------------------------------------------------------------------------------------------------------------
def _grant(g, frm, term=7):
    return dict(group=g, type=L.MSG_VOTE_RESP, term=term, **{"from": frm})


def test_one_grant_builds_the_broadcast(oracle):
    """N = 3, a candidate at term 7 whose log ends at (10, term 2): LogTerm is neither the term nor the term before it"""
    G, N, me = 4, 3, 0
    st = L.candidate_state(G, N, me)
    with _engine(st) as e:
        s, off = L.frames([_grant(1, 2)], me)
        w = _check(e, st, s, off, None, "one grant")
        go, (sent, ents, _), po = w["got"]
    assert go["type"][0] == 4 and w["answered"][0] and w["wins"] == [0]  # RAFTQ_OUT_BECAME_LEADER, flagged
    assert list(po) == [0, 0, 1, 2] and list(sent["to"]) == [1, 2]
    assert (sent["type"] == L.MSG_APP).all() and (sent["term"] == 7).all() and (sent["index"] == 10).all() and (sent["log_term"] == 2).all()
    assert (sent["commit"] == 8).all() and (sent["from"] == me).all() and (sent["group"] == 1).all() and (sent["n_ents"] == 1).all()
    for k in range(2):
        en = ents[int(sent["ent_first"][k])]
        assert (int(en["term"]), int(en["index"]), int(en["data_len"]), int(en["type"])) == (7, 11, 0, 0)


@pytest.mark.parametrize("bitmap", ["clear", "none"])
def test_an_ack_behind_the_win_is_answered_too(oracle, bitmap):
    """the broadcast leaves every follower at the tail: the ack that commits the empty entry gets the usual empty MsgApps, behind
    the entry frame in every peer's slice -- with the caller's bit clear, and with no bitmap at all"""
    G, N, me = 4, 3, 0
    st = L.candidate_state(G, N, me)
    with _engine(st) as e:
        s, off = L.frames([_grant(1, 2), dict(group=1, type=L.MSG_APP_RESP, term=7, index=11, **{"from": 2})], me)
        w = _check(e, st, s, off, _bitmap(G, []) if bitmap == "clear" else None, bitmap)
        go, (sent, ents, _), po = w["got"]
    assert w["answered"].all() and list(po) == [0, 0, 2, 4]
    assert list(sent["to"]) == [1, 1, 2, 2] and list(sent["n_ents"]) == [1, 0, 1, 0]
    assert list(sent["index"]) == [10, 11, 10, 11] and list(sent["log_term"]) == [2, 7, 2, 7] and list(sent["commit"]) == [8, 11, 8, 11]
    assert int(st.committed[1]) == 11


def test_switch_off_is_the_call_as_it_was(oracle):
    """the same frames into a handle that never saw the switch, one that had it on and off again, and the old restatement: results,
    flags and bytes are the same, and the win ends its group's prefix"""
    from tests import _stepgen

    G, N, me = 600, 3, 1
    rng = np.random.default_rng(5100)
    st, cands, granters = L.one_grant_short(rng, G, N, me)
    a, b = _engine(st, lead=False), _engine(st, lead=False)
    with a, b:
        b.set_respond_lead(True)
        b.set_respond_lead(False)
        assert a.respond_cap(10) == b.respond_cap(10) == 10 * (N - 1) * 83
        s, off = L.random_call(rng, st, cands, granters, 700, 80, 60)
        at = _leaders_bitmap(rng, st, 1.0)
        wm, we, _ = W.wire_decode(s, off)
        _, rec = _node_filter(wm, we, G, N, me, True)
        lt0 = st.last_term.copy()
        outs = st.step_batch(rec)
        want_w, want_po, want_ans = expected_off(rec, outs, lt0, at, N, me)
        want_s = W.wire_encode(want_w)[0]
        wins = outs["type"] == 4
        assert wins.sum() >= WIN_FLOOR and not want_ans[wins].any()
        for e in (a, b):
            gm, ge, go, got_s, got_off, got_po, c, rc = _call(e, s, off, len(we), at)
            assert np.array_equal((go["flags"] & ANSWERED) != 0, want_ans)
            go = go.copy()
            go["flags"] &= np.uint8(~ANSWERED & 0xFF)
            _same(go, outs, "results")
            assert bytes(got_s) == bytes(want_s) and np.array_equal(got_po, want_po) and rc.n_msgs == len(want_w)
            _stepgen.assert_same_state(e, st)


def test_a_grant_behind_a_held_frame_wins_nothing(oracle):
    """the nearest input to "a win behind a result that ended the prefix" (the module's docstring): a MsgProp ends the prefix and
    holds the grant behind it -- no win, nothing answered, no frame; the group next to it wins as usual"""
    G, N, me = 4, 3, 0
    st = L.candidate_state(G, N, me)
    with _engine(st) as e:
        s, off = L.frames([dict(group=1, type=L.MSG_PROP, term=0, **{"from": 1}), _grant(1, 2), _grant(2, 1)], me)
        w = _check(e, st, s, off, None, "held")
        go, _, po = w["got"]
    assert list(go["type"]) == [11, 9, 4] and list(w["answered"]) == [False, False, True] and po[-1] == 2  # HELD, DEFERRED, BECAME_LEADER
    assert int(st.role[1]) == 1 and int(st.role[2]) == 2


# ---- every cluster size and slot ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(seed, G, N, me, sizes, masked=False):
    """the inputs of a run of calls, computed once and never changed (the references move with a copy)"""
    rng = np.random.default_rng(seed)
    voters = None
    if masked:
        voters = V.random_masks(rng, N, G)
    st, cands, granters = L.one_grant_short(rng, G, N, me, voters)
    start = V.copy_state(st)
    calls = []
    for n_noise, n_grants, n_acks in sizes:
        s, off = L.random_call(rng, st, cands, granters, n_noise, n_grants, n_acks)
        at = _leaders_bitmap(rng, st)
        calls.append((s, off, at))
        L.want(st, s, off, at, voters)  # (moves st: the next call's frames follow the state)
    return start, voters, calls


def _run_case(case):
    """-> the answered wins of every call, as the reference counts them"""
    start, voters, calls = _random_case(*case)
    st = V.copy_state(start)
    wins = []
    with _engine(st, voters=voters) as e:
        for it, (s, off, at) in enumerate(calls):
            w = _check(e, st, s, off, at, f"{case} call {it}", voters, resp_off=it != 1)
            wins.append(len(w["wins"]))
    return wins


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8, 9])
def test_every_cluster_size_and_slot(oracle, N):
    for me in range(N):
        wins = _run_case((5200 + 16 * N + me, 400, N, me, ((300, 60, 40),)))
        assert min(wins) >= 20, (N, me, wins)


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("seed", [5301, 5302])
def test_random_batches(oracle, walk, seed, monkeypatch):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    wins = _run_case((seed, 3000, 5, 2, ((1, 1, 0), (255, 200, 100), (9000, 300, 200))))
    assert wins[0] == 1 and min(wins[1:]) >= WIN_FLOOR, wins  # (the first call is two frames, one of them the grant)


# ---- workgroup boundaries and the sorted walk -------------------------------------------------------------------------------------
def test_wins_at_the_workgroup_boundaries(oracle):
    """513 frames -- two workgroups of 256 and a lone lane -- with the wins at the first lane, a wave's last and the next one's first,
    a workgroup's last and the next one's first, and the lone lane; every other frame is a heartbeat to a follower group"""
    G, N, me, n = 600, 5, 3, 513
    positions = (0, 63, 64, 255, 256, 512)
    st = L.candidate_state(G, N, me)
    st.votes[(me + 1) % N] = 1  # (N = 5: two grants, the third wins)
    fol = np.arange(G) >= 6
    st.role[fol], st.vote[fol], st.votes[:, fol] = 0, 0, 0
    others = [p for p in range(N) if p != me]
    rows, k = [], 0
    for i in range(n):
        if i in positions:
            rows.append(_grant(positions.index(i), (me + 2) % N))
        else:
            rows.append(dict(group=6 + k, type=L.MSG_HB, term=7, commit=9, **{"from": others[k % (N - 1)]}))
            k += 1
    with _engine(st) as e:
        s, off = L.frames(rows, me)
        w = _check(e, st, s, off, None, "boundaries")
    assert w["wins"] == list(positions) and w["answered"].all() and w["n_frames"] == 6 * (N - 1) + (n - 6)


def test_a_long_run_with_the_win_goes_through_the_sorted_walk(oracle):
    """more than 32 frames of one group: the list walk stalls, the replay answers through step_lead_kernel and the layout -- with
    the entry headers -- is made again"""
    G, N, me = 8, 3, 1
    st = L.candidate_state(G, N, me)
    rows = [dict(group=5, type=L.MSG_VOTE, term=7, index=10, log_term=2, **{"from": 0}) for _ in range(20)]  # refused: we are a candidate
    rows += [_grant(5, 2)]
    rows += [dict(group=5, type=L.MSG_APP_RESP, term=7, index=11, **{"from": 2 * (k % 2)}) for k in range(15)]
    rows += [_grant(3, 0)]
    with _engine(st) as e:
        s, off = L.frames(rows, me)
        w = _check(e, st, s, off, None, "long run")
    assert w["wins"] == [20, 36] and w["answered"][:22].all() and int(st.committed[5]) == 11


# ---- over members ---------------------------------------------------------------------------------------------------------------------
def test_the_broadcast_goes_to_the_members(oracle):
    """N = 5, voters {0, 1, 2}: frames to slots 1 and 2 only; a group whose only voter is this node wins on a non-voter's answer and
    is answered with zero frames"""
    G, N, me = 4, 5, 0
    st = L.candidate_state(G, N, me)
    voters = np.full(G, 0b00111, np.uint16)
    voters[2] = 0b00001
    with _engine(st, voters=voters) as e:
        s, off = L.frames([_grant(1, 1), _grant(2, 3)], me)
        w = _check(e, st, s, off, None, "members", voters)
        go, (sent, ents, _), po = w["got"]
    assert list(go["type"]) == [4, 4] and w["answered"].all() and w["wins"] == [0, 1]
    assert list(po) == [0, 0, 1, 2, 2, 2] and list(sent["to"]) == [1, 2] and (sent["group"] == 1).all() and (sent["n_ents"] == 1).all()


def test_random_batches_over_members(oracle):
    wins = _run_case((5400, 4000, 5, 1, ((2000, 150, 100), (3000, 150, 100)), True))
    assert min(wins) >= WIN_FLOOR, wins


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_its_twin(oracle):
    """a cap one byte under the new bound, the switch with a batch in flight, on = 2: each is refused, and after each everything that
    can be read of the handle is what a twin that saw no refusal holds; then both take a whole call"""
    from raftsql_amd import _lib
    from raftsql_amd import step as S
    from raftsql_amd.engine import RaftqError
    from tests import _refusals as R

    G, N, me = 1024, 5, 2
    rng = np.random.default_rng(5500)
    st, cands, granters = L.one_grant_short(rng, G, N, me)
    s, off = L.random_call(rng, st, cands, granters, 400, 100, 60)
    n = len(off) - 1
    n_ents = len(W.wire_decode(s, off)[1])

    def code(f, *a, **kw):
        with pytest.raises(RaftqError) as ei:
            f(*a, **kw)
        return ei.value.code

    with R.engine(st) as e, R.engine(st) as t:
        for x in (e, t):
            x.set_respond_lead(True)
        assert e.respond_cap(n) == n * (N - 1) * 109
        assert code(_call, e, s, off, n_ents, None, cap=e.respond_cap(n) - 1) == _lib.RAFTQ_EINVAL
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "cap one below the bound")
        assert code(e.set_respond_lead, 2) == _lib.RAFTQ_EINVAL
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "on = 2")
        m = S.pack_msgs(np.array([0], np.uint64), S.MSG_HEARTBEAT_RESP, term=st.term[:1], frm=(me + 1) % N)
        for x in (e, t):
            x.step_submit(m)
        assert code(e.set_respond_lead, False) == _lib.RAFTQ_ESTATE  # a batch in flight
        for x in (e, t):
            x.step_collect()
        st.step_batch(m)
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "the switch with a batch in flight")
        # (the refused settings left the switch on: the wins are answered)
        w = _check(e, V.copy_state(st), s, off, None, "after the refusals")
        assert len(w["wins"]) >= WIN_FLOOR
        _check(t, st, s, off, None, "the twin")
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "behind the whole call")
