"""GPU: Tick and its two device-built rounds over each group's own members (raftq_tick_set_voters; tick_voters_kernel,
beat_build_voters_kernel, elect_build_voters_kernel) against tests/ref_tick_members.py.

Nothing expected comes from the code under test: the masked Tick is oracle.pyoracle.tick with promotable() on top (held against
a per-group restatement of upstream by tests/test_tick_members_ref.py); the heartbeats are test_tick_frames_gpu.want_frames'
filtered by mask; the campaigns are ref_step_voters.step_batch's on the MsgHup messages; bytes and offsets are
oracle.pywire.wire_encode's, spread over the positional slots.

Shapes: G = 2,500 is three 1,024-group blocks, the last one partial; N in {2, 3, 5, 9} with self first, in the middle and last;
heartbeat_tick 1 and 3; one case of 10-byte varints; one case above 16,384 tick waves (the build kernels take their offsets
from the scan).  So that a twin that ignores its masks cannot pass, the INPUTS are held to the conditions _conditions states."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from tests import _stepgen
from tests import ref_step_voters as V
from tests import ref_tick_members as M
from tests import ref_voters as RV
from tests import test_tick_elect_gpu as TE
from tests import test_tick_frames_gpu as TF

pytestmark = pytest.mark.gpu

ET, SEED = TF.ET, TF.SEED
G0 = 2500
SHAPES = ((2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4), (9, 0), (9, 4), (9, 8))
TICKS = 6


def _masks(rng, st, hot=6):
    """ref_step_voters.random_masks with the edge cases planted: among the leaders an empty mask (an unused slot that leads by
    role) and self-absent; among the others {self} alone -- `hot` of them about to fire whatever the draw -- the full mask and
    self-absent with a timer that WOULD fire"""
    n, me, g = st.N, st.self_peer, st.G
    voters = V.random_masks(rng, n, g)
    empty, full, only_me, not_me = M.hand_masks(n, me)
    lead, free = np.flatnonzero(st.role == 2), np.flatnonzero(st.role != 2)
    lead, free = rng.permutation(lead), rng.permutation(free)
    voters[lead[:3]] = empty
    voters[lead[3:6]] = not_me
    voters[lead[6:8]] = full
    voters[free[:hot + 6]] = only_me
    st.elapsed[free[:hot]] = 2 * ET - 1  # elapsed + 1 - ElectionTick = ElectionTick > any draw
    voters[free[hot + 6:hot + 10]] = not_me
    st.elapsed[free[hot + 6:hot + 10]] = 2 * ET - 1
    voters[free[hot + 10:hot + 12]] = full
    voters[free[hot + 12:hot + 14]] = empty
    return voters


def _conditions(st, voters, built_beats, built_hups, role_before):
    """what the inputs must be for a pass to mean something (asserted on the reference's side, before anything is compared)"""
    n, me = st.N, st.self_peer
    others = ((1 << n) - 1) & ~(1 << me)
    vb, vh = voters[built_beats].astype(np.uint32), voters[built_hups].astype(np.uint32)
    free = role_before != 2
    idle = free & ~M.mine_of(voters, me)
    drop_b, drop_h = float(((vb & others) != others).mean()), float(((vh & others) != others).mean())
    solo = int((vh == (1 << me)).sum())
    empty_led = int((vb == 0).sum())
    if n >= 3:
        assert drop_b >= 1 / 3 and drop_h >= 1 / 3, (drop_b, drop_h)
    else:  # both arms occur
        assert 0 < drop_b < 1 and 0 < drop_h < 1, (drop_b, drop_h)
    assert idle.sum() >= free.sum() / 4, (int(idle.sum()), int(free.sum()))
    assert solo >= 5 and empty_led >= 1, (solo, empty_led)
    return drop_b, drop_h, solo, empty_led


def _engines(st, voters, hb, twin_switch=True):
    """the engine under test (masks loaded, the switch on) and a twin that only ticks, masked too"""
    from raftsql_amd.wire import WireEngine

    e, twin = WireEngine(st.G, st.N, st.self_peer), WireEngine(st.G, st.N, st.self_peer)
    for x in (e, twin):
        x.set_timers(ET, hb, SEED)
        _stepgen.load_engine(x, st)
        x.load_voters(voters)
    e.set_tick_voters(True)
    if twin_switch:
        twin.set_tick_voters(True)
    return e, twin


def _bits(words, g):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:g]


def _code(f, *args, **kw):
    from raftsql_amd.engine import RaftqError

    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- the Tick alone ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tick_plan(n, me, hb):
    """the reference, once per shape and never changed: start state, masks, per tick (elapsed, action, n_hup, n_beat)"""
    from oracle import pyoracle

    rng = np.random.default_rng(13500 + 16 * n + 4 * me + hb)
    st = TE.make_state(rng, G0, n, me, hb)
    voters = _masks(rng, st)
    start = V.copy_state(st)
    el, ticks = st.elapsed.copy(), []
    for t in range(TICKS):
        r = M.tick_array(pyoracle, st.role, el, voters, me, ET, hb, SEED, t)
        ticks.append(r)
        el = r[0]
    free = st.role != 2
    assert (free & ~M.mine_of(voters, me)).sum() >= free.sum() / 4
    assert sum(r[2] for r in ticks) > 50 and all(r[3] > 0 for r in ticks)
    # an unmasked Tick would differ: some group that may not campaign is past its timeout
    plain = pyoracle.tick(st.role, start.elapsed, ET, hb, SEED, 0)
    assert plain[2] > ticks[0][2]
    return start, voters, ticks


@pytest.mark.parametrize("n,me", SHAPES)
def test_tick_parity(oracle, n, me):
    """six consecutive ticks through raftq_tick, raftq_tick_collect, raftq_tick_collect_lists and raftq_tick_frames: action, elapsed,
    role, the lists or the bitmap and both counts are the reference's"""
    for hb in (1, 3):
        start, voters, ticks = _tick_plan(n, me, hb)
        a, b = _engines(start, voters, hb)
        c, d = _engines(start, voters, hb)
        with a, b, c, d:
            for t, (el, act, nh, nb) in enumerate(ticks):
                what = f"N={n} self={me} hb={hb} tick {t}"
                hups, beats = np.flatnonzero(act == 1), np.flatnonzero(act == 2)
                bitmap = t % 2 == 0
                assert a.tick() == (nh, nb), what
                h2, nh2, b2, nb2 = b.tick_collect()
                assert (nh2, nb2) == (nh, nb) and np.array_equal(h2, hups) and np.array_equal(b2, beats), what
                h3, nh3, s3, nb3 = c.tick_collect_lists(None, None, beat_bitmap=bitmap)
                assert (nh3, nb3) == (nh, nb) and np.array_equal(h3, hups), what
                assert np.array_equal(_bits(s3, G0), act == 2) if bitmap else np.array_equal(s3, beats), what
                bufs = TF.Bufs(d, 0)
                _, _, _, cnt, h4, nh4, s4, nb4 = d.tick_frames(None, None, bufs.po, 0, beat_bitmap=bitmap, cap=0)
                assert (nh4, nb4, cnt.n_msgs) == (nh, nb, 0) and np.array_equal(h4, hups), what
                for x in (a, b, c, d):
                    g_act, g_el, g_role = x.read_tick()
                    assert np.array_equal(g_act, act) and np.array_equal(g_el, el) and np.array_equal(g_role, start.role), what


# ---- raftq_tick_frames -----------------------------------------------------------------------------------------------------------
def _check_beats(oracle, e, twin, st, voters, tick_no, hb, beat_cap, bitmap, what, frame_off=True, seen=None):
    """one raftq_tick_frames over members against the reference (st.elapsed moves with it)"""
    G, N, me = st.G, st.N, st.self_peer
    role0 = st.role.copy()
    el, act, rh, rb = M.tick_array(oracle, st.role, st.elapsed, voters, me, ET, hb, SEED, tick_no)
    st.elapsed[:] = el
    hups, beats = np.flatnonzero(act == 1).astype(np.uint32), np.flatnonzero(act == 2).astype(np.uint32)
    w, keep, want_po = M.member_beats(st, voters, beats, beat_cap)
    b = TF.Bufs(e, beat_cap, frame_off)
    want_s, want_off = M.encode_members(w, keep, b.n_max)
    got_s, _, got_po, c, got_h, nh, second, nb = e.tick_frames(b.out, b.off[: b.n_max + 1] if frame_off else None, b.po, beat_cap, beat_bitmap=bitmap,
                                                               cap=b.cap)
    print(f"{what}: n_hup {nh} n_beat {nb} slots {len(keep)} member frames {int(keep.sum())} bytes {c.bytes}")
    assert (nh, nb) == (rh, rb), what
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (int(keep.sum()), 0, 0, len(want_s)), what
    assert np.array_equal(got_po, want_po), (what, got_po, want_po)
    assert bytes(got_s) == bytes(want_s), what
    if frame_off:
        assert np.array_equal(b.off[: b.n_max + 1], want_off), what  # zero-length slots, and the total past the last slot
        n_built = min(len(beats), beat_cap)
        for p in range(N):  # a peer's bytes are the member records to it alone, in group order
            sl = slice(int(want_po[p]), int(want_po[p + 1]))
            alone = W.wire_encode(w[sl][keep[sl]])[0] if keep[sl].any() else np.zeros(0, np.uint8)
            assert M.peer_bytes(got_s, b.off, got_po, p) == bytes(alone), (what, p)
            assert sl.stop - sl.start == (0 if p == me else n_built), what
    assert b.canaries_ok(), what
    assert np.array_equal(got_h, hups), what
    assert np.array_equal(_bits(second, G), act == 2) if bitmap else np.array_equal(second, beats[: min(beat_cap, G)]), what
    g_act, g_el, g_role = e.read_tick()
    assert np.array_equal(g_act, act) and np.array_equal(g_el, el) and np.array_equal(g_role, role0), what
    if twin is not None:
        t_h, t_nh, t_second, t_nb = twin.tick_collect_lists(None, beat_cap, beat_bitmap=bitmap)
        assert (t_nh, t_nb) == (nh, nb) and np.array_equal(t_h, got_h) and np.array_equal(t_second, second), what
        for x, y in zip(twin.read_tick(), (act, el, role0)):
            assert np.array_equal(x, y), what
    if seen is not None:
        seen.append((beats[:beat_cap].astype(np.int64), role0))
    return len(beats), int(keep.sum())


@pytest.mark.parametrize("n,me", SHAPES)
def test_heartbeats_go_to_members(oracle, n, me):
    """six ticks; beat_cap above, at and below the MsgBeat count and 0; with and without frame_off; both flags values"""
    for hb in (1, 3):
        rng = np.random.default_rng(13600 + 16 * n + 4 * me + hb)
        st = TF.make_state(rng, G0, n, me, hb)
        st.elapsed[:] = np.where(st.role == 2, st.elapsed, rng.integers(0, 2 * ET, G0))  # (some timers fire: the lists are not empty)
        voters = _masks(rng, st)
        n_lead = int((st.role == 2).sum())
        e, twin = _engines(st, voters, hb)
        seen, built_all = [], 0
        with e, twin:
            for t, pick in enumerate(["all", "more", 0, "half", "exact", "all"]):
                nb_next = M.tick_array(oracle, st.role, st.elapsed, voters, me, ET, hb, SEED, t)[3]  # (a look ahead: the caps follow the count)
                cap = {"all": G0, "more": nb_next + 7, "half": nb_next // 2, "exact": nb_next}.get(pick, pick)
                nb, nf = _check_beats(oracle, e, twin, st, voters, t, hb, cap, bitmap=(t + hb) % 2 == 0, what=f"N={n} self={me} hb={hb} tick {t} cap {pick}",
                                      frame_off=t != 1, seen=seen)
                assert nb == nb_next and nf <= min(nb, cap) * (n - 1)
                built_all += min(nb, cap)
            assert hb == 3 or built_all >= 3 * n_lead
        beats = np.concatenate([s[0] for s in seen])
        vb = voters[beats].astype(np.uint32)
        others = ((1 << n) - 1) & ~(1 << me)
        drop = float(((vb & others) != others).mean())
        assert (drop >= 1 / 3) if n >= 3 else (0 < drop < 1), drop
        assert (vb == 0).any(), "a built group with an empty mask: a leader by role that produces no frames"


# ---- raftq_tick_elect_frames -----------------------------------------------------------------------------------------------------
def _check_round(oracle, e, twin, st, voters, tick_no, hb, hup_cap, beat_cap, bitmap, what, frame_off=True, sweep=True, seen=None):
    """one raftq_tick_elect_frames over members against the reference (st moves with it) -> (MsgHup groups, MsgBeat groups, member frames)"""
    from raftsql_amd import _lib

    G, N, me = st.G, st.N, st.self_peer
    if twin is not None:
        twin.load_roles(st.role, st.elapsed)  # (the twin only ticks: it gets the roles the campaigns left)
    role0 = st.role.copy()
    el, act, rh, rb = M.tick_array(oracle, st.role, st.elapsed, voters, me, ET, hb, SEED, tick_no)
    st.elapsed[:] = el
    hups, beats = np.flatnonzero(act == 1).astype(np.uint32), np.flatnonzero(act == 2).astype(np.uint32)
    bw, bkeep, bpo = M.member_beats(st, voters, beats, beat_cap)
    before = V.copy_state(st) if hup_cap < len(hups) else None
    vw, vkeep, want_camp, built, outs = M.member_campaigns(st, voters, hups, hup_cap)
    w, keep = np.concatenate([bw, vw]), np.concatenate([bkeep, vkeep])
    want_po = np.zeros(2 * (N + 1), np.uint64)
    want_po[: N + 1] = bpo
    want_po[N + 1] = bpo[N]
    want_po[N + 2:] = bpo[N] + np.cumsum([0 if p == me else len(built) for p in range(N)]).astype(np.uint64)
    b = TE.Bufs(e, hup_cap, beat_cap, frame_off)
    want_s, want_off = M.encode_members(w, keep, b.n_max)
    got_s, _, got_po, c, got_camp, got_h, nh, second, nb = e.tick_elect_frames(
        b.camp[:hup_cap] if hup_cap else None, b.out, b.off[: b.n_max + 1] if frame_off else None, b.po, hup_cap, beat_cap, beat_bitmap=bitmap, cap=b.cap)
    lead_now = int((want_camp["type"] == M.OUT_BECAME_LEADER).sum())
    print(f"{what}: n_hup {nh} n_beat {nb} slots {len(keep)} member frames {int(keep.sum())} bytes {c.bytes} campaigned {len(built)} "
          f"leaders at once {lead_now}")
    assert (nh, nb) == (rh, rb), what
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (int(keep.sum()), 0, 0, len(want_s)), what
    assert np.array_equal(got_po, want_po), (what, got_po, want_po)
    assert bytes(got_s) == bytes(want_s), what
    if frame_off:
        assert np.array_equal(b.off[: b.n_max + 1], want_off), what
    assert b.canaries_ok(N), what
    assert got_camp.tobytes() == want_camp.tobytes(), what
    assert np.array_equal(got_h, hups[: min(hup_cap, G)]), what
    assert np.array_equal(_bits(second, G), act == 2) if bitmap else np.array_equal(second, beats[: min(beat_cap, G)]), what
    # a group whose only voter is self became leader and got no frame; no other group did
    solo = voters[built] == (1 << me)
    assert np.array_equal(want_camp["type"] == M.OUT_BECAME_LEADER, solo), what
    assert not (want_camp["flags"][solo] & M.OUTF_ANSWERED).any() and (want_camp["flags"][~solo] & M.OUTF_ANSWERED).all(), what
    g_act, g_el, g_role = e.read_tick()
    assert np.array_equal(g_act, act) and np.array_equal(g_el, st.elapsed) and np.array_equal(g_role, st.role), what
    if before is not None:  # the groups behind hup_cap are untouched
        rest = hups[hup_cap:].astype(np.int64)
        assert len(rest) and np.array_equal(st.role[rest], before.role[rest]) and np.array_equal(st.term[rest], before.term[rest]), what
    if twin is not None:
        t_h, t_nh, t_second, t_nb = twin.tick_collect_lists(hup_cap, beat_cap, beat_bitmap=bitmap)
        assert (t_nh, t_nb) == (nh, nb) and np.array_equal(t_h, got_h) and np.array_equal(t_second, second), what
        for x, y in zip(twin.read_tick(), (act, el, role0)):
            assert np.array_equal(x, y), what
    _stepgen.assert_same_state(e, st)
    if sweep:  # the dense rows and the vote words as the masked sweep and tally read them
        e.sweep(_lib.SWEEP_COMMIT | _lib.SWEEP_VOTES | _lib.SWEEP_NO_ADOPT)
        assert np.array_equal(e.read_committed(), RV.commit_advance(st.match, st.committed, voters)[0]), what
        assert np.array_equal(e.read_outcome(), RV.vote_tally(st.votes, voters)[0]), what
    if seen is not None:
        seen.append((beats[:beat_cap].astype(np.int64), built, role0))
    return len(hups), len(beats), int(keep.sum())


def _held_to_conditions(st, voters, seen):
    beats = np.concatenate([s[0] for s in seen])
    hups = np.concatenate([s[1] for s in seen])
    return _conditions(st, voters, beats, hups, seen[0][2])


@pytest.mark.parametrize("n,me", SHAPES)
def test_campaigns_go_to_voters(oracle, n, me):
    """six ticks; both caps above, at and below their counts; a candidate campaigns again; groups whose only voter is self become
    leader and beat (to nobody) from the next tick on"""
    for hb in (1, 3):
        rng = np.random.default_rng(13700 + 16 * n + 4 * me + hb)
        st = TE.make_state(rng, G0, n, me, hb)
        voters = _masks(rng, st)
        e, twin = _engines(st, voters, hb)
        seen, again = [], 0
        with e, twin:
            for t, pick in enumerate(["all", "all", "third", "exact", "more", "all"]):
                _, act, nh_next, nb_next = M.tick_array(oracle, st.role, st.elapsed, voters, me, ET, hb, SEED, t)
                assert nh_next > 8, "the timers were meant to fire on every tick"
                hup_cap = {"all": G0, "third": nh_next // 3, "exact": nh_next, "more": nh_next + 7}[pick]
                beat_cap = {"all": G0, "third": max(nb_next - 1, 0), "exact": nb_next, "more": nb_next // 2}[pick]
                again += int((st.role[np.flatnonzero(act == 1)[:hup_cap]] == 1).sum())
                nh, nb, nf = _check_round(oracle, e, twin, st, voters, t, hb, hup_cap, beat_cap, bitmap=(t + hb) % 2 == 0,
                                          what=f"N={n} self={me} hb={hb} tick {t} caps {pick}", frame_off=t != 1, sweep=t in (0, 3, 5), seen=seen)
                assert (nh, nb) == (nh_next, nb_next)
        assert again > 0, "a candidate was meant to campaign again"
        print("conditions (drop among beats, among campaigns, sole voters, empty led):", _held_to_conditions(st, voters, seen))


def test_sixty_four_bit_terms_and_indices(oracle):
    """terms at 2^62 .. 2^64 - 2, lastIndex / lastTerm up to 2^64 - 1: 10-byte varints in every field of the member frames"""
    G, n, me, hb = 300, 3, 1, 1
    rng = np.random.default_rng(13800)
    st = TE.make_state(rng, G, n, me, hb, wide64=True)
    top = np.uint64(2**64 - 1)
    free = st.role != 2
    st.term[free] = np.minimum(st.term[free], top - np.uint64(1))
    voters = _masks(rng, st)
    g1 = np.flatnonzero(free & M.mine_of(voters, me) & (voters != (1 << me)))[0]
    st.last_index[g1], st.last_term[g1], st.elapsed[g1] = top, top, 2 * ET - 1
    st.match[me][g1] = top
    assert int(st.term.min()) >= 2**62
    e, twin = _engines(st, voters, hb)
    seen = []
    with e, twin:
        for t in range(2):
            nh, nb, nf = _check_round(oracle, e, twin, st, voters, t, hb, G, G, bitmap=t == 0, what=f"64-bit tick {t}", seen=seen)
            assert (nh > 5 or t > 0) and nb > 50 and nf > 50  # (the planted timers fire at tick 0)
    assert st.role[g1] == 1
    _held_to_conditions(st, voters, seen)


def test_the_scan_path(oracle):
    """above 16,384 tick waves both build kernels take their block offsets from scan_partials_kernel: G = 4,196,000, N = 3, a few
    hundred groups act, in the first and the last block too"""
    from oracle import pyoracle
    from raftsql_amd.wire import WireEngine

    G, n, me, hb, cap = 4196000, 3, 1, 1, 1500
    assert G // 256 > 16384
    rng = np.random.default_rng(13900)
    st = pyoracle.NodeState(G, n, me)
    pick = rng.permutation(G)[:1000]
    lead = np.unique(np.concatenate([[1, 1022, G - 1023, G - 2], pick[:500]]))
    fire = np.setdiff1d(np.unique(np.concatenate([[0, 5, 1023, G - 1024, G - 7, G - 1], pick[500:]])), lead)
    for ids in (lead, fire):
        st.term[ids] = TF._spread(rng, len(ids))
        st.last_index[ids] = TF._spread(rng, len(ids))
        st.last_term[ids] = st.term[ids]
    st.role[lead], st.first_idx[lead], st.vote[lead], st.lead[lead] = 2, 1, me + 1, me + 1
    st.committed[lead] = (st.last_index[lead] * rng.random(len(lead))).astype(np.uint64)
    for p in range(n):
        st.match[p][lead] = (st.last_index[lead] * rng.random(len(lead))).astype(np.uint64)
    st.match[me] = st.last_index
    st.elapsed[fire] = 2 * ET - 1  # d = ElectionTick > any draw: these fire where self votes, nobody else is past the timeout
    voters = V.random_masks(rng, n, G)
    voters[fire[:8]] = 1 << me
    voters[lead[:2]] = 0
    e = WireEngine(G, n, me)
    with e:
        e.set_timers(ET, hb, SEED)
        _stepgen.load_engine(e, st)
        e.load_voters(voters)
        e.set_tick_voters(True)
        seen = []
        nh, nb, nf = _check_round(oracle, e, None, st, voters, 0, hb, cap, cap, True, "scan path", sweep=False, seen=seen)
        assert nb == len(lead) and 0 < nh < len(fire) and nh == int(M.mine_of(voters, me)[fire].sum())
    _held_to_conditions(st, voters, seen)


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_the_switch(oracle):
    """off (the default) with masks loaded: both calls are refused with RAFTQ_ESTATE and "voter masks", nothing ticks, and the plain
    Tick reads no mask; on: they go through.  -1 and 2 are RAFTQ_EINVAL, a batch in flight is RAFTQ_ESTATE, a handle that is no
    node's cannot run the masked Tick"""
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine
    from raftsql_amd.wire import WireEngine

    n, me, hb = 3, 2, 1
    rng = np.random.default_rng(14000)
    st = TE.make_state(rng, G0, n, me, hb)
    voters = _masks(rng, st)
    lib = _lib.load()
    with WireEngine(G0, n, me) as e, WireEngine(G0, n, me) as plain:
        for x in (e, plain):
            x.set_timers(ET, hb, SEED)
            _stepgen.load_engine(x, st)
            x.load_voters(voters)
        fb, eb = TF.Bufs(e, G0), TE.Bufs(e, G0, G0)
        rc, msg = _code(e.tick_frames, fb.out, fb.off[: fb.n_max + 1], fb.po, G0, cap=fb.cap)
        assert rc == _lib.RAFTQ_ESTATE and "voter masks" in msg
        rc, msg = _code(e.tick_elect_frames, eb.camp[:G0], eb.out, eb.off[: eb.n_max + 1], eb.po, G0, G0, cap=eb.cap)
        assert rc == _lib.RAFTQ_ESTATE and "voter masks" in msg
        _stepgen.assert_same_state(e, st)  # neither ticked
        assert lib.raftq_tick_set_voters(e._h, -1) == _lib.RAFTQ_EINVAL and lib.raftq_tick_set_voters(e._h, 2) == _lib.RAFTQ_EINVAL
        m = _stepgen.random_batch(rng, st, 50)
        e.set_step_voters(True)
        e.step_submit(m)
        assert _code(e.set_tick_voters, True)[0] == _lib.RAFTQ_ESTATE  # a batch in flight
        e.step_collect()
        e.set_step_voters(False)
        _stepgen.load_engine(e, st)  # (the batch moved the state)
        # off: the plain Tick on a masked handle reads no mask
        el, act, nh, nb = oracle.tick(st.role, st.elapsed, ET, hb, SEED, 0)
        assert plain.tick() == (nh, nb) and np.array_equal(plain.read_tick()[0], act)
        assert nh > M.tick_array(oracle, st.role, st.elapsed, voters, me, ET, hb, SEED, 0)[2]
        # on: both go through
        e.set_tick_voters(True)
        _check_round(oracle, e, None, st, voters, 0, hb, G0, G0, True, "switched on")
        _check_beats(oracle, e, None, st, voters, 1, hb, G0, False, "switched on, heartbeats alone")
        # off again: refused again, the parent's text
        e.set_tick_voters(False)
        rc, msg = _code(e.tick_frames, fb.out, fb.off[: fb.n_max + 1], fb.po, G0, cap=fb.cap)
        assert rc == _lib.RAFTQ_ESTATE and "voter masks" in msg
    with QuorumEngine(G0, n) as q:  # not a node's handle: promotable() cannot ask whether THIS node votes
        q.set_timers(ET, hb, SEED)
        q.load_roles(st.role, st.elapsed)
        q.load_voters(voters)
        assert q.tick() == oracle.tick(st.role, st.elapsed, ET, hb, SEED, 0)[2:]  # off: the parent's Tick does not ask
        assert lib.raftq_tick_set_voters(q._h, 1) == _lib.RAFTQ_OK
        assert lib.raftq_tick(q._h, None) == _lib.RAFTQ_ESTATE
        q.load_voters(None)
        assert lib.raftq_tick(q._h, None) == _lib.RAFTQ_OK  # no masks: what it always was


def test_masks_dropped_is_the_unmasked_call(oracle):
    """the switch on and the masks dropped by raftq_load_voters(h, NULL): the existing unmasked expectations, every frame"""
    n, me, hb = 5, 2, 1
    rng = np.random.default_rng(14100)
    st = TE.make_state(rng, G0, n, me, hb)
    voters = _masks(rng, st)
    e, twin = _engines(st, voters, hb)
    with e, twin:
        for x in (e, twin):
            x.load_voters(None)
        nh, nb, nf, _ = TE.check_tick(oracle, e, twin, st, 0, hb, G0, G0, bitmap=True, what="masks dropped, tick 0")
        assert nf == (nh + nb) * (n - 1)
        twin.load_roles(st.role, st.elapsed)
        nb, nf = TF.check_tick(oracle, e, twin, st, 1, hb, G0, bitmap=False, what="masks dropped, tick 1")
        assert nf == nb * (n - 1)
        for x in (e, twin):  # dropping the masks did not clear the switch: it is the handle's
            x.load_voters(voters)
        _check_round(oracle, e, twin, st, voters, 2, hb, G0, G0, True, "masks loaded again")


def test_both_switches(oracle):
    """raftq_tick_set_voters and raftq_step_set_voters on one handle: granting MsgVoteResps for the device-campaigned groups then
    elect over voters exactly as the masked statement does, and the next tick's rounds are right -- one consistent state"""
    from raftsql_amd import step as S

    n, me, hb = 5, 1, 1
    rng = np.random.default_rng(14200)
    st = TE.make_state(rng, G0, n, me, hb)
    voters = _masks(rng, st)
    e, twin = _engines(st, voters, hb)
    with e, twin:
        e.set_step_voters(True)
        nh, _, _ = _check_round(oracle, e, twin, st, voters, 0, hb, G0, G0, True, "the campaigns")
        cand = np.flatnonzero(st.role == 1).astype(np.uint64)
        assert nh > 50 and len(cand) > 50
        lead0 = int((st.role == 2).sum())
        for frm in ((me + 1) % n, (me + 2) % n):
            m = S.pack_msgs(rng.permutation(cand), TE.MSG_VOTE_RESP, frm=frm)
            m["term"] = st.term[m["group"].astype(np.int64)]
            want = V.step_batch(st, voters, m)
            got, _ = e.step_batch(m)
            assert got.tobytes() == want.tobytes()
        won = int((st.role == 2).sum()) - lead0
        assert 0 < won < len(cand), "some elections are won over the voters, some are not yet"
        _stepgen.assert_same_state(e, st)
        _, nb, _ = _check_round(oracle, e, twin, st, voters, 1, hb, G0, G0, False, "the new leaders' heartbeats")
        assert nb == lead0 + won
