"""GPU: the fused Tick calls and the device-built rounds under CheckQuorum and PreVote (raftq_tick_set_checks: tick_check_kernel behind
raftq_tick_collect / _collect_lists / raftq_tick_frames / raftq_tick_elect_frames, tick_lists32_checks_kernel's third list,
elect_build_cq_kernel / elect_build_cq_voters_kernel) against tests/ref_tick_checks.py.

Nothing expected comes from the code under test: every figure, list, record and byte is the composed reference's, which
tests/test_tick_checks_ref.py holds against the references it composes and a hand table; that file also shows that every case's
inputs discriminate.  Beside the reference each case drives a TWIN handle through the route a handle with the switches on had before:
raftq_tick, raftq_collect_hups / _beats / _checks, raftq_step_batch of the MsgHup records -- same results, same state.

Shapes (the issue's): G in {1, 129, 3149}, N in {2, 3, 5} and 9 once, heartbeat_tick 1 and 3, election_tick 10 with lead_elapsed
preloaded so that checks fall due within the three ticks every case runs; CheckQuorum alone, with PreVote, and both over voter masks.
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from oracle import pywire as W
from tests import _stepgen
from tests import ref_pre_vote as PV
from tests import ref_tick_checks as R
from tests import ref_voters as RV
from tests import test_tick_elect_gpu as TE
from tests import test_tick_frames_gpu as TF

pytestmark = pytest.mark.gpu

ET, SEED = R.ET, R.SEED
CASES = R.case_list()
_ids = lambda c: "-".join(str(v) for v in c)  # noqa: E731


def _engine(scene, chk_cap=None, checks=True):
    """a node's handle with the scene loaded and its switches on (both in front of the load: raftq_load_roles takes role 3 only under
    raftq_set_pre_vote); checks=False: the twin, which never hears of raftq_tick_set_checks"""
    from raftsql_amd.wire import WireEngine

    st = scene["st"]
    e = WireEngine(st.G, st.N, st.self_peer)
    e.set_timers(ET, scene["hb"], SEED)
    e.set_check_quorum(True)
    if scene["pre_vote"]:
        e.set_pre_vote(True)
    _stepgen.load_engine(e, st)
    if scene["voters"] is not None:
        e.load_voters(scene["voters"])
        e.set_tick_voters(True)
        e.set_step_voters(True)
    e.load_activity(scene["active"], scene["lead_elapsed"])
    if checks:
        e.set_tick_checks(st.G if chk_cap is None else chk_cap)
    return e


def _bits(words, g):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:g]


def _code(f, *args, **kw):
    from raftsql_amd.engine import RaftqError

    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


def _same_after(e, after, what):
    st, active, le = after
    _stepgen.assert_same_state(e, st)
    a, l = e.read_activity()
    assert np.array_equal(a, active), (what, "active")
    assert np.array_equal(l, le), (what, "lead_elapsed")


def _twin_route(twin, r, hup_cap, what):
    """today's route on the twin: raftq_tick, the three collect calls, raftq_step_batch of the MsgHup records"""
    from raftsql_amd import step as S

    assert twin.tick() == (len(r["hups"]), len(r["beats"])), what
    for got, want in ((twin.collect_hups(), r["hups"]), (twin.collect_beats(), r["beats"]), (twin.collect_checks(), r["checks"])):
        assert got[1] == len(want) and np.array_equal(got[0], want), what
    built = r["hups"][:hup_cap].astype(np.uint64)
    if len(built):
        outs, _ = twin.step_batch(S.pack_msgs(built, R.MSG_HUP))
        assert outs.tobytes() == r["outs"].tobytes(), what
    _same_after(twin, r["after"], what + " (twin)")


def check_round(e, twin, scene, r, hup_cap, beat_cap, chk_cap, bitmap, what, frame_off=True, sweep=True):
    """one raftq_tick_elect_frames under the switch against the reference's round r (and the twin's route, when given)"""
    from raftsql_amd import _lib

    st = scene["st"]
    G, N, voters = st.G, st.N, scene["voters"]
    b = TE.Bufs(e, hup_cap, beat_cap, frame_off)
    assert b.n_max == r["n_max"]
    got_s, _, got_po, c, got_camp, got_h, nh, second, nb = e.tick_elect_frames(
        b.camp[:hup_cap] if hup_cap else None, b.out, b.off[: b.n_max + 1] if frame_off else None, b.po, hup_cap, beat_cap, beat_bitmap=bitmap, cap=b.cap)
    got_c, nc = e.last_tick_checks()
    print(f"{what}: n_hup {nh} n_beat {nb} checks {nc} frames {c.n_msgs} bytes {c.bytes} campaigned {len(r['built'])}")
    assert (nh, nb, nc) == (len(r["hups"]), len(r["beats"]), len(r["checks"])), what
    assert np.array_equal(got_h, r["hups"][:hup_cap]), what
    assert np.array_equal(got_c, r["checks"][:chk_cap]), what
    assert np.array_equal(_bits(second, G), r["act"] == 2) if bitmap else np.array_equal(second, r["beats"][:beat_cap]), what
    assert got_camp.tobytes() == r["camp"].tobytes(), what
    assert np.array_equal(got_po, r["po"]), (what, got_po, r["po"])
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (r["frames"], 0, 0, len(r["stream"])), what
    assert bytes(got_s) == bytes(r["stream"]), what
    if frame_off:
        assert np.array_equal(b.off[: b.n_max + 1], r["off"]), what  # zero-length slots, and the total past the last slot
    assert b.canaries_ok(N), what
    g_act, g_el, g_role = e.read_tick()
    s1 = r["after"][0]
    assert np.array_equal(g_act, r["act"]) and np.array_equal(g_el, s1.elapsed) and np.array_equal(g_role, s1.role), what
    _same_after(e, r["after"], what)
    if hup_cap < len(r["hups"]):  # the MsgHup groups beyond the cap: nothing of them was touched
        rest, s0 = r["hups"][hup_cap:].astype(np.int64), r["before"][0]
        assert np.array_equal(s1.role[rest], s0.role[rest]) and np.array_equal(s1.term[rest], s0.term[rest]), what
    if chk_cap < len(r["checks"]):  # the checks beyond the cap come from the Tick's bitmap
        rest, n = e.collect_checks()
        assert n == len(r["checks"]) and np.array_equal(rest, r["checks"]), what
    if twin is not None:
        _twin_route(twin, r, hup_cap, what)
    if sweep:  # the dense rows and the vote words as the sweep and the tally read them
        e.sweep(_lib.SWEEP_COMMIT | _lib.SWEEP_VOTES | _lib.SWEEP_NO_ADOPT)
        if voters is None:
            want_c, want_o = pyoracle.commit_advance(s1.match, s1.committed)[0], pyoracle.vote_tally(s1.votes)[0]
        else:
            want_c, want_o = RV.commit_advance(s1.match, s1.committed, voters)[0], RV.vote_tally(s1.votes, voters)[0]
        assert np.array_equal(e.read_committed(), want_c) and np.array_equal(e.read_outcome(), want_o), what


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_rounds_match_the_reference_and_the_twin(oracle, case):
    """three fused calls in a row per scene: both flags values, with and without frame_off, every cap at G"""
    mode, g, n = case[:3]
    for k, scene in enumerate(R.scenes(*case)):
        rounds = R.play(scene)
        with _engine(scene) as e, _engine(scene, checks=False) as twin:
            for t, r in enumerate(rounds):
                check_round(e, twin, scene, r, g, g, g, bitmap=(t + scene["hb"]) % 2 == 0, what=f"{mode} G={g} N={n} scene {k} tick {t}",
                            frame_off=t != 1, sweep=t == 2)


def _tick_only(scene, ticks=R.TICKS):
    """the reference's Ticks alone (nobody campaigns) -> [(act, hups, beats, checks, (st, active, lead_elapsed) after)]"""
    st, active, le = R.copy_case(scene["st"], scene["active"], scene["lead_elapsed"])
    out = []
    for t in range(ticks):
        act = R.tick(st, active, le, scene["voters"], scene["hb"], t)
        out.append((act,) + tuple(np.flatnonzero(act == a).astype(np.uint32) for a in (1, 2, 3)) + (R.copy_case(st, active, le),))
    return out


@pytest.mark.parametrize("case", [("cq", 3149, 3), ("cq_pv_masks", 3149, 5), ("cq_masks", 129, 2), ("cq_pv", 1, 3)], ids=_ids)
def test_the_three_other_calls(oracle, case):
    """raftq_tick_collect, raftq_tick_collect_lists and raftq_tick_frames under the switch: the lists or the bitmap, the third list (from
    raftq_collect_checks behind the copying form), and a heartbeat round that holds no group with action 3"""
    mode, g, n = case
    for k, scene in enumerate(R.scenes(mode, g, n)):
        ticks = _tick_only(scene)
        with _engine(scene) as a, _engine(scene) as b, _engine(scene) as c:
            for t, (act, hups, beats, checks, after) in enumerate(ticks):
                what = f"{mode} G={g} N={n} scene {k} tick {t}"
                bitmap = t % 2 == 0
                h1, nh1, b1, nb1 = a.tick_collect()
                assert (nh1, nb1) == (len(hups), len(beats)) and np.array_equal(h1, hups) and np.array_equal(b1, beats), what
                c1, nc1 = a.collect_checks()
                assert nc1 == len(checks) and np.array_equal(c1, checks), what
                h2, nh2, s2, nb2 = b.tick_collect_lists(None, None, beat_bitmap=bitmap)
                c2, nc2 = b.last_tick_checks()
                assert (nh2, nb2, nc2) == (len(hups), len(beats), len(checks)) and np.array_equal(h2, hups) and np.array_equal(c2, checks), what
                assert np.array_equal(_bits(s2, g), act == 2) if bitmap else np.array_equal(s2, beats), what
                bufs = TF.Bufs(c, g)
                w, keep, want_po = R.beats_round(after[0], scene["voters"], beats, g)
                want_s, want_off = R.M.encode_members(w, keep, bufs.n_max)
                got_s, _, got_po, cnt, h3, nh3, s3, nb3 = c.tick_frames(bufs.out, bufs.off[: bufs.n_max + 1], bufs.po, g, beat_bitmap=bitmap, cap=bufs.cap)
                c3, nc3 = c.last_tick_checks()
                assert (nh3, nb3, nc3) == (len(hups), len(beats), len(checks)) and np.array_equal(h3, hups) and np.array_equal(c3, checks), what
                assert np.array_equal(_bits(s3, g), act == 2) if bitmap else np.array_equal(s3, beats), what
                assert (cnt.n_msgs, cnt.bytes) == (int(keep.sum()), len(want_s)) and bytes(got_s) == bytes(want_s), what
                assert np.array_equal(got_po, want_po) and np.array_equal(bufs.off[: bufs.n_max + 1], want_off) and bufs.canaries_ok(), what
                assert not np.isin(w["group"], checks).any(), what  # no frame for a group whose check failed
                assert int(got_po[n]) == len(beats) * (n - 1), what  # the slices add up: fillers included
                for x in (a, b, c):
                    g_act, g_el, _ = x.read_tick()
                    assert np.array_equal(g_act, act) and np.array_equal(g_el, after[0].elapsed), what
                    _same_after(x, after, what)


def test_the_copying_form_leaves_no_third_list(oracle):
    from raftsql_amd._lib import RAFTQ_ESTATE

    scene = R.scenes("cq", 129, 3)[0]
    with _engine(scene) as e:
        assert _code(e.last_tick_checks)[0] == RAFTQ_ESTATE  # no fused call yet
        e.tick_collect_lists()
        assert e.last_tick_checks()[1] >= 0
        e.tick_collect()
        assert _code(e.last_tick_checks)[0] == RAFTQ_ESTATE  # the last call was the copying form
        e.tick_collect_lists()
        e.tick()
        assert _code(e.last_tick_checks)[0] == RAFTQ_ESTATE  # ... or a plain raftq_tick
        e.tick_collect_lists()
        e.set_tick_checks(0)
        assert _code(e.last_tick_checks)[0] == RAFTQ_ESTATE  # the switch is a call on the handle too


# ---- caps --------------------------------------------------------------------------------------------------------------------------
def _caps_scene():
    """CheckQuorum with PreVote over masks, G = 3149, N = 3, with enough failing checks for a cap to cut"""
    base = R.scenes("cq_pv_masks", 3149, 3)[0]
    scene = dict(base, active=base["active"].copy(), lead_elapsed=base["lead_elapsed"].copy())
    lead = np.flatnonzero(base["st"].role == 2)[::4]
    scene["active"][lead], scene["lead_elapsed"][lead] = 0, ET - 1
    return scene


@pytest.mark.parametrize("which", ["hup_cap", "beat_cap", "chk_cap"])
def test_a_cap_below_its_count(oracle, which):
    """the listed prefix is exact, the total is the full count, the remaining checks come from raftq_collect_checks, the MsgHup groups
    beyond hup_cap are not campaigned and nothing of them is touched"""
    scene = _caps_scene()
    g = scene["st"].G
    st, active, le = R.copy_case(scene["st"], scene["active"], scene["lead_elapsed"])
    look = R.play(scene, ticks=1)[0]  # (a look ahead: the cap is relative to this tick's count)
    count = {"hup_cap": len(look["hups"]), "beat_cap": len(look["beats"]), "chk_cap": len(look["checks"])}[which]
    assert count > 8, (which, count)
    caps = dict(hup_cap=g, beat_cap=g, chk_cap=g)
    caps[which] = count // 3
    with _engine(scene, chk_cap=caps["chk_cap"]) as e, _engine(scene, checks=False) as twin:
        for t in range(2):
            before = R.copy_case(st, active, le)
            r = R.round_(st, active, le, scene["voters"], scene["hb"], t, caps["hup_cap"], caps["beat_cap"], scene["pre_vote"])
            r["before"], r["after"] = before, R.copy_case(st, active, le)
            check_round(e, twin, scene, r, caps["hup_cap"], caps["beat_cap"], caps["chk_cap"], bitmap=which != "beat_cap" and t == 1,
                        what=f"{which} {caps[which]} of {count} tick {t}", sweep=False)


def test_hup_cap_zero_is_tick_frames(oracle):
    """byte for byte, list for list -- and nobody campaigns"""
    scene = R.scenes("cq_pv", 3149, 3)[0]
    g, n = scene["st"].G, scene["st"].N
    with _engine(scene) as e, _engine(scene) as f:
        for t, (act, hups, beats, checks, after) in enumerate(_tick_only(scene, 2)):
            be, bf = TE.Bufs(e, 0, g), TF.Bufs(f, g)
            s1, o1, p1, c1, camp, h1, nh1, x1, nb1 = e.tick_elect_frames(None, be.out, be.off[: be.n_max + 1], be.po, 0, g, beat_bitmap=t == 0, cap=be.cap)
            k1 = e.last_tick_checks()
            s2, o2, p2, c2, h2, nh2, x2, nb2 = f.tick_frames(bf.out, bf.off[: bf.n_max + 1], bf.po, g, hup_cap=0, beat_bitmap=t == 0, cap=bf.cap)
            k2 = f.last_tick_checks()
            assert (nh1, nb1, int(c1.n_msgs), int(c1.bytes), len(camp), len(h1)) == (nh2, nb2, int(c2.n_msgs), int(c2.bytes), 0, 0)
            assert (nh1, nb1, k1[1]) == (len(hups), len(beats), len(checks)) and len(beats) > 0
            assert bytes(s1) == bytes(s2) and np.array_equal(o1, o2) and np.array_equal(p1[: n + 1], p2) and np.array_equal(x1, x2)
            assert np.array_equal(k1[0], k2[0]) and np.array_equal(k1[0], checks) and k1[1] == k2[1]
            assert be.canaries_ok(n) and bf.canaries_ok()
            for x in (e, f):
                _same_after(x, after, f"hup_cap 0 tick {t}")


# ---- the scan path -----------------------------------------------------------------------------------------------------------------
def test_the_scan_path(oracle):
    """the smallest handle of more than 16,384 tick waves: all three lists take their offsets from scan_partials_kernel (the third
    pass is new); CheckQuorum with PreVote; timers fire and checks fail in the first and the last block too"""
    G, N, me, hb = 16385 * 256, 2, 1, 1
    rng = np.random.default_rng(28700)
    st = pyoracle.NodeState(G, N, me)
    edge = [0, 5, 1023, G - 1024, G - 7, G - 1]
    fire = np.unique(np.concatenate([edge, rng.integers(0, G, 300)]))
    st.elapsed[fire] = 2 * ET - 1  # d = ElectionTick > any draw: these fire, nobody else is past the timeout
    st.term[fire] = TF._spread(rng, len(fire))
    st.last_index[fire] = TF._spread(rng, len(fire))
    st.last_term[fire] = st.term[fire]
    st.role[fire[::5]] = 1  # some of them candidates: they turn pre-candidate
    st.vote[fire[::5]] = me + 1
    st.votes[me, fire[::5]] = 1
    st.match[me] = st.last_index
    lead = np.setdiff1d(np.unique(np.concatenate([[1, 6, 1022, G - 1023, G - 8, G - 2], rng.integers(0, G, 200)])), fire)
    st.role[lead], st.lead[lead], st.vote[lead], st.first_idx[lead] = 2, me + 1, me + 1, 1
    st.term[lead] = TF._spread(rng, len(lead))
    st.last_index[lead] = TF._spread(rng, len(lead))
    st.last_term[lead] = st.term[lead]
    st.match[me] = st.last_index
    st.committed[lead] = (st.last_index[lead] * rng.random(len(lead))).astype(np.uint64)
    st.match[1 - me][lead] = (st.last_index[lead] * rng.random(len(lead))).astype(np.uint64)
    active, le = np.zeros(G, np.uint16), np.zeros(G, np.uint32)
    le[lead] = ET - 1                    # every leader's check is due ...
    active[lead[::2]] = 1 << (1 - me)    # ... every second one has heard from its peer
    scene = dict(st=st, active=active, lead_elapsed=le, voters=None, hb=hb, pre_vote=True)
    hup_cap, beat_cap, chk_cap = 512, 64, 64
    r = R.play(scene, hup_cap, beat_cap, ticks=1)[0]
    assert len(r["hups"]) == len(fire) and len(r["checks"]) == len(lead) - len(lead[::2]) and len(r["beats"]) == len(lead[::2])
    assert len(r["checks"]) > chk_cap and (r["outs"]["type"] == R.OUT_PRE_CAMPAIGN).all()
    with _engine(scene, chk_cap=chk_cap) as e:
        check_round(e, None, scene, r, hup_cap, beat_cap, chk_cap, True, "scan path", sweep=False)


# ---- Step afterwards ---------------------------------------------------------------------------------------------------------------
def _msgs_of_frames(stream, off, lo, hi, frm):
    """peer frames [lo, hi) of a call's output, decoded by the wire oracle -> the raftq_msg_t records their addressee steps"""
    from raftsql_amd import step as S

    wm, _, bad = W.wire_decode(stream, np.ascontiguousarray(off[lo:hi + 1]))
    assert bad == 0 and (wm["from"] == frm).all()
    m = S.pack_msgs(wm["group"].astype(np.uint64), 0, frm=frm)
    m["type"], m["term"], m["index"], m["log_term"] = wm["type"], wm["term"], wm["index"], wm["log_term"]
    return m, wm


def test_step_afterwards(oracle):
    """three nodes: node 0's fused call starts a pre-election in every group; the MsgPreVote frames it produced are stepped by nodes 1
    and 2, their MsgPreVoteResps by node 0 -- the pre-election is won, the real campaign follows and is won too; ref_pre_vote agrees
    with every handle at every step"""
    G, N, hb = 200, 3, 1
    rng = np.random.default_rng(28800)
    ss, acts, les = [], [], []
    terms = TF._spread(rng, G, 1, 3)
    for k in range(N):  # the same terms and equal logs everywhere, nobody leads
        s = pyoracle.NodeState(G, N, k)
        ss.append(s)
        s.term[:] = terms
        s.last_index[:], s.last_term[:] = 5, terms
        s.match[k] = 5
        s.elapsed[:] = 2 * ET - 1 if k == 0 else rng.integers(0, 3, G)
        acts.append(np.zeros(G, np.uint16))
        les.append(np.zeros(G, np.uint32))
    scenes = [dict(st=ss[k], active=acts[k], lead_elapsed=les[k], voters=None, hb=hb, pre_vote=True) for k in range(N)]
    es = [_engine(scenes[0])] + [_engine(scenes[k], checks=False) for k in (1, 2)]
    try:
        term0 = ss[0].term.copy()
        r = R.play(scenes[0], ticks=1)[0]
        assert (r["outs"]["type"] == R.OUT_PRE_CAMPAIGN).all() and len(r["built"]) == G
        check_round(es[0], None, scenes[0], r, G, G, G, False, "the pre-elections")
        ref = [r["after"]] + [R.copy_case(ss[k], acts[k], les[k]) for k in (1, 2)]
        stream, off, po = r["stream"], r["off"], r["po"]

        def step(k, m, what):
            want = PV.step_batch(ref[k][0], None, ref[k][1], ref[k][2], m, ET)
            got, _ = es[k].step_batch(m)
            assert got.tobytes() == want.tobytes(), what
            _same_after(es[k], ref[k], what)
            return want

        inbox = []
        for p in (1, 2):  # the frames to peer p, as the device wrote them, are what the reference's host would have sent
            m, wm = _msgs_of_frames(stream, off, int(po[N + 1 + p]), int(po[N + 2 + p]), 0)
            routed = PV.route(0, r["outs"], N)[p]
            assert (wm["type"] == PV.MsgPreVote).all() and (wm["to"] == p).all() and m.tobytes() == routed.tobytes()
            outs = step(p, m, f"MsgPreVote at node {p}")
            assert (outs["type"] == PV.OutPreVoteResp).all() and (outs["reject"] == 0).all()
            inbox.append(PV.route(p, outs, N)[0])
        won = step(0, inbox[0], "the first grant: a quorum, the campaign follows")
        assert (won["type"] == R.OUT_CAMPAIGN).all() and np.array_equal(ref[0][0].term, term0 + 1) and (ref[0][0].role == 1).all()
        late = step(0, inbox[1], "the second grant: a candidate ignores it")
        assert (late["type"] == 0).all()
        votes = PV.route(0, won, N)
        resp = [PV.route(p, step(p, votes[p], f"MsgVote at node {p}"), N)[0] for p in (1, 2)]
        lead = step(0, resp[0], "the first MsgVoteResp")
        assert (lead["type"] == R.OUT_BECAME_LEADER).all() and (ref[0][0].role == 2).all()
        step(0, resp[1], "the second MsgVoteResp")
    finally:
        for e in es:
            e.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine, SweepSet, pinned_empty
    from raftsql_amd.step import OUT_S_DT

    EINVAL, ESTATE = _lib.RAFTQ_EINVAL, _lib.RAFTQ_ESTATE
    scene = R.scenes("cq_pv", 129, 3)[0]
    st = scene["st"]
    G, N = st.G, st.N
    start = (st, scene["active"], scene["lead_elapsed"])
    with _engine(scene, checks=False) as e:
        lib, h = e._lib, e._h
        nh, nb, cnt = C.c_uint64(0), C.c_uint64(0), _lib.WireCounts()
        cap = e.respond_cap(2 * G)
        n_max = 2 * G * (N - 1)
        out, off, po = pinned_empty(cap + 16, np.uint8), pinned_empty(n_max + 2, np.uint64), pinned_empty(2 * (N + 1) + 2, np.uint64)
        camp = pinned_empty(G + 1, OUT_S_DT)
        hups, beats = np.zeros(G, np.uint64), np.zeros(G, np.uint64)

        def elect(camp_, out_, cap_, off_=off, po_=po):
            return lib.raftq_tick_elect_frames(h, 0, G, G, C.byref(nh), C.byref(nb), camp_.ctypes.data, out_.ctypes.data, cap_, off_.ctypes.data,
                                               po_.ctypes.data, C.byref(cnt))

        def frames(out_, cap_):
            return lib.raftq_tick_frames(h, 0, G, G, C.byref(nh), C.byref(nb), out_.ctypes.data, cap_, off.ctypes.data, po.ctypes.data, C.byref(cnt))

        calls = {
            "raftq_tick_collect": lambda: lib.raftq_tick_collect(h, hups.ctypes.data, G, C.byref(nh), beats.ctypes.data, G, C.byref(nb)),
            "raftq_tick_collect_lists": lambda: lib.raftq_tick_collect_lists(h, 0, G, G, C.byref(nh), C.byref(nb)),
            "raftq_tick_frames": lambda: frames(out, cap),
            "raftq_tick_elect_frames": lambda: elect(camp, out, cap),
        }

        def unmoved(what):
            act, el, role = e.read_tick()
            assert not act.any() and np.array_equal(el, st.elapsed) and np.array_equal(role, st.role), what  # did not tick
            _same_after(e, start, what)

        # the switch off: each of the four refuses with the text it has today, and has not ticked
        for name, call in calls.items():
            assert call() == ESTATE, name
            text = lib.raftq_last_error(h).decode()
            assert ("pre vote" if name == "raftq_tick_elect_frames" else "check quorum") in text and name in text, (name, text)
            unmoved(name)
        assert _code(e.last_tick_checks)[0] == ESTATE
        e.set_pre_vote(False)  # ... and without PreVote the election round's refusal is CheckQuorum's
        assert calls["raftq_tick_elect_frames"]() == ESTATE and "check quorum" in lib.raftq_last_error(h).decode()
        e.set_pre_vote(True)
        e.set_tick_checks(G)
        e.set_tick_checks(0)  # off again is off
        assert calls["raftq_tick_collect_lists"]() == ESTATE
        # the switch on: what the calls always refused is refused before the Tick and before the campaigns
        e.set_tick_checks(G)
        assert _code(e.last_tick_checks)[0] == ESTATE  # no fused call has run yet
        assert elect(camp, out, cap - 1) == EINVAL  # cap one byte under the worst case
        assert frames(out, e.respond_cap(G) - 1) == EINVAL
        assert elect(np.zeros(G, OUT_S_DT), out, cap) == EINVAL  # pageable camp
        assert elect(camp, np.zeros(cap, np.uint8), cap) == EINVAL  # pageable out
        assert frames(np.zeros(cap, np.uint8), cap) == EINVAL
        assert elect(camp, out, cap, np.zeros(n_max + 1, np.uint64)) == EINVAL  # pageable frame_off
        assert elect(camp, out, cap, off, np.zeros(2 * (N + 1), np.uint64)) == EINVAL  # pageable peer_off
        assert lib.raftq_tick_collect_lists(h, 2, G, G, C.byref(nh), C.byref(nb)) == EINVAL  # unknown flag
        unmoved("argument checks under the switch")
        assert _code(e.last_tick_checks)[0] == ESTATE
        # raftq_set_tick keeps refusing a member with CheckQuorum on
        with QuorumEngine(G, N) as other, SweepSet([e, other]) as ss:
            code, text = _code(ss.tick)
            assert code == ESTATE and "check quorum" in text
        unmoved("raftq_set_tick")
        # the clone copies state, never the switch
        with _engine(scene, checks=False) as d:
            d.clone_state_from(e)
            assert _code(d.tick_collect_lists)[0] == ESTATE
        # none of it ticked or campaigned: the first accepted call is the reference's first round
        r = R.play(scene, ticks=1)[0]
        check_round(e, None, scene, r, G, G, G, True, "after the refusals")
    # CheckQuorum off: the switch has no effect
    from raftsql_amd.wire import WireEngine

    with WireEngine(G, N, st.self_peer) as q:
        q.set_timers(ET, 1, SEED)
        s0 = R.V.copy_state(st)
        s0.role[s0.role == 3] = 1
        _stepgen.load_engine(q, s0)
        q.set_tick_checks(7)
        el, act, rh, rb = oracle.tick(s0.role, s0.elapsed, ET, 1, SEED, 0)
        got_h, n_h, got_b, n_b = q.tick_collect_lists()
        assert (n_h, n_b) == (rh, rb) and np.array_equal(got_h, np.flatnonzero(act == 1)) and np.array_equal(got_b, np.flatnonzero(act == 2))
        assert _code(q.last_tick_checks)[0] == ESTATE
