"""GPU: raftq_tick_elect_frames (include/raftq_wire.h) -- raftq_tick_frames plus the election round the Tick calls for: Step(MsgHup)
applied on the device to the groups whose timers fired, their MsgVotes marshalled behind the heartbeats.

Nothing expected comes from the code under test: the MsgHup / MsgBeat groups are oracle.pyoracle.tick's; the state after the
campaigns and the result records are NodeState.step_batch's on pack_msgs(hups[:hup_cap], MSG_HUP) (the contract adds
RAFTQ_OUTF_ANSWERED to the flags: the host sends nothing); the heartbeats are test_tick_frames_gpu.want_frames'; the bytes are
oracle.pywire.wire_encode's.  The Tick half is also compared with a twin handle driven through raftq_tick_collect_lists."""
import ctypes as C

import numpy as np
import pytest

from oracle import pywire as W
from tests import test_tick_frames_gpu as TF

pytestmark = pytest.mark.gpu

MSG_HUP, MSG_VOTE, MSG_VOTE_RESP = 0, 5, 6
OUT_CAMPAIGN, OUT_BECAME_LEADER = 3, 4
OUTF_HARDSTATE, OUTF_ANSWERED = 0x01, 0x10
CANARY, CANARY64 = TF.CANARY, TF.CANARY64
ET, SEED = TF.ET, TF.SEED


def make_state(rng, G, N, me, hb, wide64=False):
    """test_tick_frames_gpu.make_state with the non-leaders' timers spread over [0, 2 * ElectionTick): some fire on every tick"""
    s = TF.make_state(rng, G, N, me, hb, wide64)
    s.elapsed[:] = np.where(s.role == 2, s.elapsed, rng.integers(0, 2 * ET, G))
    return s


def plan(oracle, st, hb, ticks, hup_cap=None):
    """the oracle alone, on a copy: per tick (MsgHup groups, candidates among the campaigned ones)"""
    import copy

    from raftsql_amd import step as S

    s = copy.deepcopy(st)
    seen = []
    for t in range(ticks):
        el, act, _, _ = oracle.tick(s.role, s.elapsed, ET, hb, SEED, t)
        s.elapsed[:] = el
        built = np.nonzero(act == 1)[0][: s.G if hup_cap is None else hup_cap]
        seen.append((int((act == 1).sum()), int((s.role[built] == 1).sum())))
        s.step_batch(S.pack_msgs(built.astype(np.uint64), MSG_HUP))
    return seen


class Bufs:
    """page-locked camp / out / frame_off / peer_off for one pair of caps, canaries behind what the call may write"""

    def __init__(self, e, hup_cap, beat_cap, frame_off=True):
        from raftsql_amd.engine import pinned_empty
        from raftsql_amd.step import OUT_S_DT

        self.hup_cap = hup_cap
        self.n_max = (beat_cap + hup_cap) * (e.n_peers - 1)
        self.cap = e.respond_cap(beat_cap + hup_cap)
        self.out = pinned_empty(self.cap + 64, np.uint8)
        self.off = pinned_empty(self.n_max + 1 + 8, np.uint64) if frame_off else None
        self.po = pinned_empty(2 * (e.n_peers + 1) + 2, np.uint64)
        self.camp = pinned_empty(hup_cap + 2, OUT_S_DT)
        self.out[:] = CANARY
        self.po[:] = CANARY64
        self.camp.view(np.uint8)[:] = CANARY
        if self.off is not None:
            self.off[:] = CANARY64

    def canaries_ok(self, n_peers):
        return (bool((self.out[self.cap:] == CANARY).all()) and (self.off is None or bool((self.off[self.n_max + 1:] == CANARY64).all()))
                and bool((self.camp[self.hup_cap:].view(np.uint8) == CANARY).all()) and bool((self.po[2 * (n_peers + 1):] == CANARY64).all()))


def want_round(st, hups, beats, hup_cap, beat_cap):
    """the oracle's heartbeat and election round on st (which MOVES: the campaigns are stepped) ->
    (wire records of both sections, peer_off [2 (N + 1)], camp records, campaigned ids, candidates among them)"""
    from raftsql_amd import step as S

    N, me = st.N, st.self_peer
    beat_w, beat_po = TF.want_frames(st, beats, beat_cap)  # (led groups and campaigning groups are disjoint)
    built = np.asarray(hups[:hup_cap], np.int64)
    again = int((st.role[built] == 1).sum())
    outs = st.step_batch(S.pack_msgs(built.astype(np.uint64), MSG_HUP)) if len(built) else np.zeros(0, S.OUT_DT)
    assert (outs["type"] == OUT_CAMPAIGN).all() and (outs["flags"] == OUTF_HARDSTATE).all(), "the oracle does not campaign for a group the Tick flagged MsgHup"
    camp = np.zeros(len(built), S.OUT_S_DT)
    for k in ("term", "index", "vote", "lead", "type", "reject", "role"):
        camp[k] = outs[k]
    camp["commit"] = outs["log_term"]  # the 32-byte record carries a campaign's lastTerm there (include/raftq_step.h)
    camp["flags"] = outs["flags"] | OUTF_ANSWERED
    recs = [beat_w]
    for p in range(N):
        if p == me:
            continue
        w = np.zeros(len(built), W.WIRE_MSG_DT)
        w["group"], w["type"], w["to"], w["from"] = built, MSG_VOTE, p, me
        w["term"], w["index"], w["log_term"] = outs["term"], outs["index"], outs["log_term"]
        recs.append(w)
    po = np.zeros(2 * (N + 1), np.uint64)
    po[: N + 1] = beat_po
    po[N + 1] = beat_po[N]
    po[N + 2:] = beat_po[N] + np.cumsum([0 if p == me else len(built) for p in range(N)]).astype(np.uint64)
    return np.concatenate(recs), po, camp, built, again


def check_tick(oracle, e, twin, st, tick_no, hb, hup_cap, beat_cap, bitmap, what, frame_off=True, sweep=True, twin_state=True, keep=None):
    """one raftq_tick_elect_frames against the oracle (st moves with it) and, when given, the twin's raftq_tick_collect_lists
    -> (MsgHup groups, MsgBeat groups, frames, candidates that campaigned again)"""
    from raftsql_amd import _lib
    from tests import _stepgen

    G, N = st.G, st.N
    if twin is not None and twin_state:
        twin.load_roles(st.role, st.elapsed)  # (the twin only ticks: it gets the roles the campaigns left)
    el, act, rh, rb = oracle.tick(st.role, st.elapsed, ET, hb, SEED, tick_no)
    st.elapsed[:] = el
    role_ticked = st.role.copy()
    hups, beats = np.nonzero(act == 1)[0].astype(np.uint32), np.nonzero(act == 2)[0].astype(np.uint32)
    want_w, want_po, want_camp, built, again = want_round(st, hups, beats, hup_cap, beat_cap)
    want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    b = Bufs(e, hup_cap, beat_cap, frame_off)
    got_s, got_off, got_po, c, got_camp, got_h, nh, second, nb = e.tick_elect_frames(
        b.camp[:hup_cap] if hup_cap else None, b.out, b.off[: b.n_max + 1] if frame_off else None, b.po, hup_cap, beat_cap, beat_bitmap=bitmap, cap=b.cap)
    print(f"{what}: n_hup {nh} n_beat {nb} frames {c.n_msgs} bytes {c.bytes} campaigned {len(built)} again {again}")
    assert (nh, nb) == (rh, rb), what
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (len(want_w), 0, 0, len(want_s)), what
    assert np.array_equal(got_po, want_po), (what, got_po, want_po)
    assert bytes(got_s) == bytes(want_s), what
    if frame_off:
        full = np.full(b.n_max + 1, len(want_s), np.uint64)  # entries past the last frame all hold the total
        full[: len(want_off)] = want_off
        assert np.array_equal(b.off[: b.n_max + 1], full), what
    assert b.canaries_ok(N), what
    if keep is not None:
        keep.update(stream=bytes(got_s), off=None if got_off is None else got_off.copy(), po=got_po.copy())
    assert got_camp.tobytes() == want_camp.tobytes(), what
    assert np.array_equal(got_h, hups[: min(hup_cap, G)]), what
    if bitmap:
        bits = np.unpackbits(second.view(np.uint8), bitorder="little")
        assert len(second) == (G + 63) // 64 and np.array_equal(bits[:G], (act == 2).astype(np.uint8)) and not bits[G:].any(), what
    else:
        assert np.array_equal(second, beats[: min(beat_cap, G)]), what
    got_act, got_el, got_role = e.read_tick()
    assert np.array_equal(got_act, act) and np.array_equal(got_el, st.elapsed) and np.array_equal(got_role, st.role), what
    if twin is not None:
        t_h, t_nh, t_second, t_nb = twin.tick_collect_lists(hup_cap, beat_cap, beat_bitmap=bitmap)
        assert (t_nh, t_nb) == (nh, nb) and np.array_equal(t_h, got_h) and np.array_equal(t_second, second), what
        if twin_state:
            for a, w in zip(twin.read_tick(), (act, el, role_ticked)):
                assert np.array_equal(a, w), what
    _stepgen.assert_same_state(e, st)
    if sweep:  # the dense rows, the vote words and the self-max word as the sweep reads them
        e.sweep(_lib.SWEEP_COMMIT | _lib.SWEEP_VOTES | _lib.SWEEP_NO_ADOPT)
        assert np.array_equal(e.read_committed(), oracle.commit_advance(st.match, st.committed)[0]), what
        assert np.array_equal(e.read_outcome(), oracle.vote_tally(st.votes)[0]), what
    return len(hups), len(beats), len(want_w), again


def _pair(G, N, me, st, hb):
    return TF._pair(G, N, me, st, hb)


def _seed(N, G, hb):
    return 11100 + 16 * N + hb + G


@pytest.mark.parametrize("N", [2, 3, 5, 9])
@pytest.mark.parametrize("G", [3149, 129, 1])
def test_campaigns_match_the_oracle(oracle, N, G):
    """three ticks in a row, heartbeat_tick 1 and 3, both flags values, with and without frame_off"""
    for hb in (1, 3):
        rng = np.random.default_rng(_seed(N, G, hb))
        me = int(rng.integers(0, N))
        st = make_state(rng, G, N, me, hb)
        if G >= 129:  # the oracle alone: every tick campaigns, some candidate campaigns again
            seen = plan(oracle, st, hb, 3)
            assert all(h > 0 for h, _ in seen) and sum(a for _, a in seen) > 0, seen
        e, twin = _pair(G, N, me, st, hb)
        with e, twin:
            for t in range(3):
                nh, nb, nf, again = check_tick(oracle, e, twin, st, t, hb, G, G, bitmap=(t + hb) % 2 == 0, what=f"N={N} G={G} hb={hb} tick {t}",
                                               frame_off=t != 1)
                assert nf == (nh + nb) * (N - 1)


def test_sixty_four_bit_terms_and_indices(oracle):
    """terms at 2^62 .. 2^64 - 2 (a campaign adds 1), lastIndex / lastTerm up to 2^64 - 1: 10-byte varints in every field"""
    G, N, me, hb = 300, 3, 1, 1
    rng = np.random.default_rng(11200)
    st = make_state(rng, G, N, me, hb, wide64=True)
    top = np.uint64(2**64 - 1)
    free = st.role != 2
    st.term[free] = np.minimum(st.term[free], top - np.uint64(1))
    g0, g1 = np.nonzero(free)[0][:2]
    st.term[g0], st.elapsed[g0] = top - np.uint64(1), 2 * ET - 1  # fires whatever the draw: the new term is 2^64 - 1
    st.last_index[g1], st.last_term[g1], st.elapsed[g1] = top, top, 2 * ET - 1
    st.match[me][g1] = top
    assert int(st.term.min()) >= 2**62
    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        for t in range(2):
            nh, nb, nf, _ = check_tick(oracle, e, twin, st, t, hb, G, G, bitmap=t == 0, what=f"64-bit tick {t}")
            assert nh > 5
            if t == 0:
                assert int(st.term[g0]) == 2**64 - 1 and st.role[g0] == 1 and st.role[g1] == 1


def test_hup_cap_below_the_hup_count(oracle):
    """only the first hup_cap MsgHup groups move, *n_hup is still the total, nothing behind cap, frame_off's or camp's end is touched;
    hup_cap = 0 is raftq_tick_frames, byte for byte"""
    from tests import _stepgen
    from raftsql_amd.wire import WireEngine

    G, N, me, hb = 2500, 3, 2, 1
    rng = np.random.default_rng(11300)
    st = make_state(rng, G, N, me, hb)
    n_lead = int((st.role == 2).sum())
    e = WireEngine(G, N, me)
    tw = WireEngine(G, N, me)  # the twin here is a node's handle too: with hup_cap = 0 it answers raftq_tick_frames
    with e, tw:
        for x in (e, tw):
            x.set_timers(ET, hb, SEED)
        _stepgen.load_engine(e, st)
        for t, pick in enumerate(["third", 1, 0, "less", "all", "more"]):
            el, act, n, _ = oracle.tick(st.role, st.elapsed, ET, hb, SEED, t)  # (a look ahead: the caps are relative to this tick's count)
            assert n > 8, "the timers were meant to fire on every tick"
            hup_cap = {"third": n // 3, "less": n - 1, "all": n, "more": n + 7}.get(pick, pick)
            beat_cap = n_lead // 2 if t % 2 == 0 else n_lead - 1
            _stepgen.load_engine(tw, st)
            if hup_cap == 0:  # the twin makes the same tick through raftq_tick_frames
                b = TF.Bufs(tw, beat_cap)
                t_s, t_off, t_po, t_c, t_h, t_nh, t_second, t_nb = tw.tick_frames(b.out, b.off[: b.n_max + 1], b.po, beat_cap, hup_cap=0, beat_bitmap=True,
                                                                                  cap=b.cap)
                keep = {}
                nh, nb, nf, _ = check_tick(oracle, e, None, st, t, hb, 0, beat_cap, True, "hup_cap 0", sweep=False, keep=keep)
                assert (t_nh, t_nb, int(t_c.n_msgs), len(t_h)) == (nh, nb, nf, 0)
                assert keep["stream"] == bytes(t_s) and np.array_equal(keep["off"], t_off) and np.array_equal(keep["po"][: N + 1], t_po)
                assert np.array_equal(b.off[: b.n_max + 1], np.concatenate([t_off, np.full(b.n_max + 1 - len(t_off), len(t_s), np.uint64)]))
            else:
                nh, nb, nf, _ = check_tick(oracle, e, tw, st, t, hb, hup_cap, beat_cap, t % 2 == 1, f"hup_cap {hup_cap}", sweep=False, twin_state=False)
            assert nh == n and nb == n_lead and nf == (min(hup_cap, n) + min(beat_cap, n_lead)) * (N - 1)


def test_step_afterwards(oracle):
    """granting MsgVoteResps make the device-campaigned groups leaders exactly as the oracle's (every byte of the results), and the
    next tick's heartbeats for them are right"""
    from raftsql_amd import step as S

    G, N, me, hb = 1500, 3, 1, 1
    rng = np.random.default_rng(11400)
    st = make_state(rng, G, N, me, hb)
    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        nh, _, _, _ = check_tick(oracle, e, twin, st, 0, hb, G, G, True, "the campaigns")
        cand = np.nonzero(st.role == 1)[0].astype(np.uint64)
        assert nh > 50 and len(cand) >= nh
        m = S.pack_msgs(rng.permutation(cand), MSG_VOTE_RESP, frm=(me + 1) % N)
        m["term"] = st.term[m["group"].astype(np.int64)]
        want = st.step_batch(m)
        got, _ = e.step_batch(m)
        assert got.tobytes() == want.tobytes()
        assert (want["type"] == OUT_BECAME_LEADER).all()
        lead0 = int((st.role == 2).sum())
        _, nb, _, _ = check_tick(oracle, e, twin, st, 1, hb, G, G, False, "the new leaders' heartbeats")
        assert nb == lead0 and lead0 > nh


def test_campaigns_follow_whatever_writes_the_state(oracle):
    """the campaigns come from the device's CURRENT state: after raftq_load_match, an adopted sweep, acks through the batching
    turn's ingest and Step batches (tests/test_tick_frames_gpu.py::test_frames_follow_whatever_writes_the_state's pattern)"""
    from raftsql_amd import _lib
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me, hb = 3000, 5, 2, 1
    rng = np.random.default_rng(11500)
    st = _stepgen.random_state(rng, G, N, me)
    st.elapsed[:] = np.where(st.role == 2, 0, rng.integers(0, 2 * ET, G))
    campaigned = 0
    with WireEngine(G, N, me) as e:
        e.set_timers(ET, hb, SEED)
        _stepgen.load_engine(e, st)
        for t, move in enumerate(["none", "load_match", "sweep", "step", "deltas", "step", "sweep", "step"]):
            if move == "load_match":
                lead = st.role == 2
                for p in range(N):
                    if p != me:
                        st.match[p] = np.where(lead, (st.last_index * rng.random(G)).astype(np.uint64), st.match[p])
                e.load_match(st.match, st.committed)
            elif move == "sweep":
                e.sweep(_lib.SWEEP_COMMIT | _lib.SWEEP_GATED)
                st.committed[:] = oracle.commit_advance(st.match, st.committed, True, st.first_idx)[0]
            elif move == "deltas":
                k = 800
                g, p = rng.integers(0, G, k).astype(np.uint64), rng.integers(0, N, k).astype(np.uint32)
                v = (st.last_index[g.astype(np.int64)] * rng.random(k)).astype(np.uint64)
                e.apply_deltas(g, p, v)
                np.maximum.at(st.match, (p.astype(np.int64), g.astype(np.int64)), v)
            elif move == "step":
                m = _stepgen.random_batch(rng, st, 4000)
                want = st.step_batch(m)
                got, _ = e.step_batch(m)
                assert np.array_equal(got, want)
            nh, _, _, _ = check_tick(oracle, e, None, st, t, hb, G, G, bitmap=t % 2 == 0, what=f"after {move} (tick {t})", sweep=False)
            campaigned += nh
    assert campaigned > 200


def test_the_scan_path(oracle):
    """the smallest handle of more than 16,384 tick waves (the offsets come from scan_partials_kernel): a few hundred timers fire,
    in the first and the last block too"""
    from oracle import pyoracle
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me, hb = 16385 * 256, 2, 1, 1
    rng = np.random.default_rng(11600)
    st = pyoracle.NodeState(G, N, me)
    fire = np.unique(np.concatenate([[0, 5, 1023, G - 1024, G - 7, G - 1], rng.integers(0, G, 300)]))
    st.elapsed[fire] = 2 * ET - 1  # d = ElectionTick > any draw: these fire, nobody else is past the timeout
    st.term[fire] = TF._spread(rng, len(fire))
    st.last_index[fire] = TF._spread(rng, len(fire))
    st.last_term[fire] = st.term[fire]
    st.match[me] = st.last_index
    with WireEngine(G, N, me) as e:
        e.set_timers(ET, hb, SEED)
        _stepgen.load_engine(e, st)
        nh, nb, nf, _ = check_tick(oracle, e, None, st, 0, hb, 512, 0, True, "scan path", sweep=False)
        assert nh == len(fire) and nb == 0 and nf == nh


def test_refusals_have_neither_ticked_nor_campaigned(oracle):
    """every refusal of the header's table returns its code before anything is enqueued: the next accepted call is the oracle's
    FIRST tick on unchanged state"""
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine, RaftqError, pinned_empty
    from raftsql_amd.step import OUT_S_DT
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me, hb = 700, 3, 0, 1
    rng = np.random.default_rng(11700)
    st = make_state(rng, G, N, me, hb)
    lib = _lib.load()

    def raw(h, flags, hup_cap, beat_cap, camp, out, cap, off, po):
        nh, nb, c = C.c_uint64(0), C.c_uint64(0), _lib.WireCounts()
        return lib.raftq_tick_elect_frames(h, flags, hup_cap, beat_cap, C.byref(nh), C.byref(nb), camp.ctypes.data if camp is not None else None,
                                           out.ctypes.data if out is not None else None, cap, off.ctypes.data if off is not None else None,
                                           po.ctypes.data, C.byref(c))

    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        cap = e.respond_cap(2 * G)
        n_max = 2 * G * (N - 1)
        out, off, po = pinned_empty(cap + 16, np.uint8), pinned_empty(n_max + 2, np.uint64), pinned_empty(2 * (N + 1) + 2, np.uint64)
        camp = pinned_empty(G + 1, OUT_S_DT)
        EINVAL, ESTATE = _lib.RAFTQ_EINVAL, _lib.RAFTQ_ESTATE
        assert raw(e._h, 0, G, G, camp, out, cap - 1, off, po) == EINVAL  # cap one byte under the bound
        assert raw(e._h, 0, G, 0, camp, out, e.respond_cap(G) - 1, off, po) == EINVAL  # ... with the campaigns alone
        assert raw(e._h, 0, G, G, np.zeros(G, OUT_S_DT), out, cap, off, po) == EINVAL  # pageable camp
        assert raw(e._h, 0, G, G, camp, np.zeros(cap, np.uint8), cap, off, po) == EINVAL  # pageable out
        assert raw(e._h, 0, G, G, camp, out, cap, np.zeros(n_max + 1, np.uint64), po) == EINVAL  # pageable frame_off
        assert raw(e._h, 0, G, G, camp, out, cap, off, np.zeros(2 * (N + 1), np.uint64)) == EINVAL  # pageable peer_off
        assert raw(e._h, 0, G, G, camp.view(np.uint8)[8:], out, cap, off, po) == EINVAL  # page-locked, but not 16-byte aligned
        assert raw(e._h, 0, G, G, camp, out[8:], cap, off, po) == EINVAL
        assert raw(e._h, 0, G, G, camp, out, cap, off[1:], po) == EINVAL
        assert raw(e._h, 0, G, G, camp, out, cap, off, po[1:]) == EINVAL
        assert raw(e._h, 0, G, G, None, out, cap, off, po) == EINVAL  # camp may be NULL only when hup_cap == 0
        assert raw(e._h, 2, G, G, camp, out, cap, off, po) == EINVAL  # unknown flag
        assert raw(e._h, 0, 2**30, 2**30, camp, out, 2**62, None, po) == EINVAL  # (beat_cap + hup_cap) * (N - 1) >= 2^31
        assert raw(e._h, 0, 2**31, 0, camp, out, 2**62, None, po) == EINVAL
        assert raw(e._h, 0, 2**29, 0, camp, out, 2**62, None, po) == EINVAL  # that many frames beyond 2^31 bytes
        # a Step batch in flight
        m = _stepgen.random_batch(rng, st, 300)
        e.step_submit(m)
        assert raw(e._h, 0, G, G, camp, out, cap, off, po) == ESTATE
        got, _ = e.step_collect()
        assert np.array_equal(got, st.step_batch(m))
        # voter masks loaded
        e.load_voters(np.full(G, (1 << N) - 1, np.uint16))
        assert raw(e._h, 0, G, G, camp, out, cap, off, po) == ESTATE
        e.load_voters(None)
        with pytest.raises(RaftqError) as ei:  # the binding raises what the library returns
            e.tick_elect_frames(camp[:G], out, off, po, G, G, cap=cap - 1)
        assert ei.value.code == EINVAL
        # none of them ticked or campaigned: the state is the oracle's, and the first accepted call is tick 0
        _stepgen.assert_same_state(e, st)
        check_tick(oracle, e, twin, st, 0, hb, G, G, True, "after the refusals")
        check_tick(oracle, e, twin, st, 1, hb, G, G, False, "after the refusals, tick 1")
    # a single-peer handle; a handle that was never a node's
    with WireEngine(G, 1, 0) as one:
        po1 = pinned_empty(4, np.uint64)
        assert raw(one._h, 0, G, G, camp, out, cap, None, po1) == EINVAL
    with QuorumEngine(G, N) as q:
        assert raw(q._h, 0, G, G, camp, out, cap, off, po) == ESTATE
