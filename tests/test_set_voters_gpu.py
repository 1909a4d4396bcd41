"""GPU: sweep sets whose members hold voter masks (raftq_set_create_voters; sweep_set_voters_kernel, tick_set_voters_kernel).

One dispatch must leave every member exactly as raftq_step_async / raftq_tick on that member alone would.  Nothing expected comes
from the code under test: a masked member is held against tests/ref_voters.py (Tick: tests/ref_tick_members.py on top of the
oracle's tick), an unmasked member against the CPU oracle -- whole arrays, bit for bit -- and then against a twin handle that was
swept or ticked on its own.

Shapes are those of tests/test_voters_gpu.py, for the reasons given there: 3149 groups = several tiles and a ragged last one, 129 =
across one 128-group round of a wave, 1 = a single group; N = 1..9 takes both groups-per-lane settings of the masked kernel and
both vote-word widths.  Inputs are that file's State: non-voters hold the largest Match and a vote, empty / full / single-voter
masks are planted, the match range is small (ties)."""
import functools

import numpy as np
import pytest

from raftsql_amd._lib import (RAFTQ_EINVAL, RAFTQ_ESTATE, SET_GRID, SET_PERSISTENT, SWEEP_CACHED, SWEEP_CHANGED, SWEEP_COMMIT, SWEEP_GATED,
                              SWEEP_LDS, SWEEP_NO_ADOPT, SWEEP_STREAM, SWEEP_VOTES)
from raftsql_amd.engine import RaftqError, SweepSet
from tests import ref_tick_members as M
from tests import ref_voters as R
from tests.test_voters_gpu import SHAPES, G0, State, _advances, _same_list

pytestmark = pytest.mark.gpu

K = 3  # member 0: random masks, member 1: full masks loaded, member 2: no masks


def _full(n, g):
    return np.full(g, (1 << n) - 1, np.uint16)


def _states(n, g, seed):
    sts = [State(n, g, seed), State(n, g, seed + 1, leak=False), State(n, g, seed + 2, leak=False)]
    sts[1].voters = _full(n, g)
    sts[2].voters = None
    return sts


def _load(E, sts):
    return [st.load(E(st.g, st.n), voters=st.voters is not None) for st in sts]


def _want(oracle, st, committed, flags):
    """-> (committed', n_changed, outcome, won, lost) of one member: the masked reference, or the oracle for a member with no masks"""
    commit, gated = bool(flags & (SWEEP_COMMIT | SWEEP_GATED)), bool(flags & SWEEP_GATED)
    cw, nc, oc, w, l = committed, 0, None, 0, 0
    if st.voters is None:
        if commit:
            cw, nc = oracle.commit_advance(st.match, committed, gated, st.gate) if gated else oracle.commit_advance(st.match, committed)
        if flags & SWEEP_VOTES:
            oc, w, l = oracle.vote_tally(st.votes)
    else:
        if commit:
            cw, nc = R.commit_advance(st.match, committed, st.voters, gated, st.gate)
        if flags & SWEEP_VOTES:
            oc, w, l = R.vote_tally(st.votes, st.voters)
    return cw, nc, oc, w, l


def _close(es):
    for e in es:
        e.close()


FLAG_CASES = (
    ("commit", SWEEP_COMMIT | SWEEP_NO_ADOPT),
    ("gated", SWEEP_COMMIT | SWEEP_GATED | SWEEP_NO_ADOPT),
    ("votes", SWEEP_VOTES),
    ("commit+votes", SWEEP_COMMIT | SWEEP_VOTES | SWEEP_NO_ADOPT),
    ("changed", SWEEP_COMMIT | SWEEP_GATED | SWEEP_VOTES | SWEEP_CHANGED | SWEEP_NO_ADOPT),
    ("adopted", SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED),
)


@pytest.mark.parametrize("n", range(1, 10))
def test_parity_of_one_dispatch(gpu_engine_cls, oracle, n):
    """K = 3, every flag combination and the three cache policies: whole arrays equal to the reference and to a twin handle swept
    alone with raftq_step_async"""
    for k, g in enumerate(SHAPES):
        sts = _states(n, g, 16000 + 100 * n + 10 * k)
        es, twins = _load(gpu_engine_cls, sts), _load(gpu_engine_cls, sts)
        with SweepSet(es, voters=True) as s:
            assert len(s) == K
            committed = [st.committed for st in sts]
            for i, (name, flags) in enumerate(FLAG_CASES):
                policy = (0, SWEEP_STREAM, SWEEP_CACHED)[(n + k + i) % 3]
                what = (n, g, name, policy)
                per, tot = s.sweep(flags | policy)
                sums = [0, 0, 0]
                for m, (e, t, st) in enumerate(zip(es, twins, sts)):
                    cw, nc, oc, w, l = _want(oracle, st, committed[m], flags)
                    if g >= 100 and m == 0 and (flags & SWEEP_COMMIT) and name != "adopted":
                        assert 0 < nc < g, what  # the case has teeth
                    assert (per[m].n_changed, per[m].n_won, per[m].n_lost) == (nc, w, l), (what, m)
                    c1 = e.wait(want_counts=True)  # the member's own tallies of the same sweep (n_partials of the masked tile)
                    assert (c1.n_changed, c1.n_won, c1.n_lost) == (nc, w, l), (what, m)
                    ct = t.sweep(flags | policy)
                    assert (ct.n_changed, ct.n_won, ct.n_lost) == (nc, w, l), (what, m)
                    if flags & SWEEP_COMMIT:
                        got = e.read_committed()
                        assert np.array_equal(got, cw) and np.array_equal(got, t.read_committed()), (what, m)
                    if flags & SWEEP_VOTES:
                        got = e.read_outcome()
                        assert np.array_equal(got, oc) and np.array_equal(got, t.read_outcome()), (what, m)
                    if flags & SWEEP_CHANGED:
                        adv, total = e.collect_changed()
                        assert total == nc and _same_list(adv, committed[m], cw), (what, m)
                        tadv, ttotal = t.collect_changed()
                        assert ttotal == total and adv.tobytes() == tadv.tobytes(), (what, m)
                    if not flags & SWEEP_NO_ADOPT:
                        committed[m] = cw
                    for j, v in enumerate((nc, w, l)):
                        sums[j] += v
                assert (tot.n_changed, tot.n_won, tot.n_lost) == tuple(sums), what
            for e, st in zip(es, sts):  # a sweep writes neither rows nor votes nor masks
                assert np.array_equal(e.read_match(), st.match) and np.array_equal(e.read_votes(), st.votes)
                assert np.array_equal(e.read_voters(), _full(n, g) if st.voters is None else st.voters)
        _close(es + twins)


def test_members_on_different_commit_buffers(gpu_engine_cls, oracle):
    """the recipe of test_set_gpu.test_set_with_members_on_different_commit_buffers: a member swept (and adopted) on its own flips
    its double buffer; the masked dispatch reads every member's CURRENT commit index from this launch's table"""
    n = 5
    sts = _states(n, G0, 16900) + [State(n, G0, 16903)]
    es = _load(gpu_engine_cls, sts)
    first = [_want(oracle, st, st.committed, SWEEP_COMMIT | SWEEP_VOTES) for st in sts]
    with SweepSet(es, voters=True) as s:
        c = es[0].sweep(SWEEP_COMMIT)  # adopts: the masked member now reads buffer 1
        assert c.n_changed == first[0][1] > 0
        c = es[2].sweep(SWEEP_COMMIT)  # ... and so does the unmasked one
        assert c.n_changed == first[2][1]
        es[3].sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)  # no flip
        per, tot = s.sweep(SWEEP_COMMIT | SWEEP_VOTES)
        for m, (e, w, c) in enumerate(zip(es, first, per)):
            assert np.array_equal(e.read_committed(), w[0]) and np.array_equal(e.read_outcome(), w[2]), m
            assert (c.n_changed, c.n_won, c.n_lost) == (0 if m in (0, 2) else w[1], w[3], w[4]), m
        # a member swept on its own in between reports that sweep (same tile here, so the same number of partials)
        c3 = es[3].sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_NO_ADOPT)
        per_w, _ = s.wait(want_counts=True)
        assert (per_w[3].n_changed, per_w[3].n_won, per_w[3].n_lost) == (c3.n_changed, c3.n_won, c3.n_lost) == (0, first[3][3], first[3][4])
        # the buffers disagree the other way round now; nothing is left to advance
        per, tot = s.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)
        assert tot.n_changed == 0
        for e, w in zip(es, first):
            assert np.array_equal(e.read_committed(), w[0])
    _close(es)


@pytest.mark.parametrize("n", [5, 9], ids=["16-bit-vote-words", "32-bit-vote-words"])
def test_conf_changes_under_the_set(gpu_engine_cls, oracle, n):
    """between set sweeps: voter deltas with reset bits on a masked member, masks loaded on the so-far unmasked member (a pointer
    appears), masks dropped everywhere (the pointers disappear: the plain kernels again), a clone from a masked source"""
    g = G0
    rng = np.random.default_rng(17000 + n)
    sts = _states(n, g, 17000 + 10 * n)
    es = _load(gpu_engine_cls, sts)
    flags = SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED
    committed = [st.committed for st in sts]

    def sweep_and_compare(s, what):
        per, tot = s.sweep(flags)
        for m, (e, st) in enumerate(zip(es, sts)):
            cw, nc, oc, w, l = _want(oracle, st, committed[m], flags)
            assert (per[m].n_changed, per[m].n_won, per[m].n_lost) == (nc, w, l), (what, m)
            assert np.array_equal(e.read_committed(), cw) and np.array_equal(e.read_outcome(), oc), (what, m)
            adv, total = e.collect_changed()
            assert total == nc and _same_list(adv, committed[m], cw) and (cw >= committed[m]).all(), (what, m)
            committed[m] = cw
        return tot

    with SweepSet(es, voters=True) as s:
        sweep_and_compare(s, "first")
        # 1. a conf change on the masked member: replicas removed in some groups, slots reused (Match and vote reset) in others
        st = sts[0]
        group = rng.integers(0, g, 900).astype(np.uint64)  # groups repeat: the last record wins
        new_voters, reset = rng.integers(0, 1 << n, 900).astype(np.uint16), rng.integers(0, 1 << n, 900).astype(np.uint16)
        es[0].apply_voter_deltas(es[0].pack_voter_deltas(group, new_voters, reset))
        st.match, st.votes, st.voters = R.apply_voter_deltas(st.match, st.votes, st.voters, group, new_voters, reset)
        assert np.array_equal(es[0].read_voters(), st.voters) and np.array_equal(es[0].read_match(), st.match)
        # acks move on, so that the next sweep has something to decide
        for m, st in enumerate(sts):
            dg, dp = rng.integers(0, g, 2000).astype(np.uint64), rng.integers(0, n, 2000).astype(np.uint32)
            dv = rng.integers(0, 14, 2000).astype(np.uint64)
            es[m].apply_deltas(dg, dp, dv)
            st.match = oracle.apply_deltas(st.match, dg, dp, dv)
        tot = sweep_and_compare(s, "after voter deltas")
        assert tot.n_changed > 0
        # 2. the unmasked member gets masks: its pointer appears in the set's tables
        sts[2].voters = State(n, g, 17500 + n).voters
        es[2].load_voters(sts[2].voters)
        for m, st in enumerate(sts):
            dg, dp = rng.integers(0, g, 2000).astype(np.uint64), rng.integers(0, n, 2000).astype(np.uint32)
            dv = rng.integers(10, 30, 2000).astype(np.uint64)
            es[m].apply_deltas(dg, dp, dv)
            st.match = oracle.apply_deltas(st.match, dg, dp, dv)
        tot = sweep_and_compare(s, "after load_voters on the unmasked member")
        assert tot.n_changed > 0
        # ... and its first masks may as well arrive as deltas on a member that dropped them
        es[2].load_voters(None)
        es[2].apply_voter_deltas(es[2].pack_voter_deltas([7, 2048], [1, 2 % (1 << n) or 1], [0, 0]))
        sts[2].voters = _full(n, g)
        sts[2].voters[[7, 2048]] = [1, 2 % (1 << n) or 1]
        sweep_and_compare(s, "after the first masks arrived as deltas")
        # 3. a clone from a masked source into a member
        src_st = State(n, g, 17600 + n)
        with src_st.load(gpu_engine_cls(g, n)) as src:
            es[1].clone_state_from(src)
        sts[1].match, sts[1].votes, sts[1].voters = src_st.match, src_st.votes, src_st.voters
        sts[1].cur_term, sts[1].first_idx = src_st.cur_term, src_st.first_idx
        committed[1] = src_st.committed
        assert np.array_equal(es[1].read_voters(), src_st.voters)
        tot = sweep_and_compare(s, "after a clone from a masked source")
        assert tot.n_changed > 0
        # 4. every mask dropped: the pointers disappear, the results are the oracle's and a plain set's
        for m, st in enumerate(sts):
            es[m].load_voters(None)
            st.voters = None
            dg, dp = rng.integers(0, g, 2000).astype(np.uint64), rng.integers(0, n, 2000).astype(np.uint32)
            dv = rng.integers(20, 50, 2000).astype(np.uint64)
            es[m].apply_deltas(dg, dp, dv)
            st.match = oracle.apply_deltas(st.match, dg, dp, dv)
        twins = [gpu_engine_cls(g, n) for _ in es]
        for t, e in zip(twins, es):
            t.clone_state_from(e)
        with SweepSet(twins) as plain:
            per_p, tot_p = plain.sweep(flags)
        tot = sweep_and_compare(s, "after load_voters(None) everywhere")
        assert tot.n_changed > 0 and tot == tot_p
        for e, t in zip(es, twins):
            assert np.array_equal(e.read_committed(), t.read_committed()) and np.array_equal(e.read_outcome(), t.read_outcome())
        _close(twins)
    _close(es)


@pytest.mark.parametrize("n", [3, 7], ids=["4-groups-per-lane", "2-groups-per-lane"])
def test_persistent_mode_with_a_masked_member_is_the_grid_form(gpu_engine_cls, oracle, n):
    sts = _states(n, G0, 17700 + n)
    flags = SWEEP_COMMIT | SWEEP_GATED | SWEEP_VOTES | SWEEP_CHANGED | SWEEP_NO_ADOPT
    got = {}
    for mode in (SET_GRID, SET_PERSISTENT):
        es = _load(gpu_engine_cls, sts)
        with SweepSet(es, voters=True) as s:
            s.set_mode(mode, 5)
            per, tot = s.sweep(flags)
            got[mode] = [(e.read_committed(), e.read_outcome(), e.collect_changed()[0].tobytes(), c) for e, c in zip(es, per)] + [tot]
        _close(es)
    for m, st in enumerate(sts):
        cw, nc, oc, w, l = _want(oracle, st, st.committed, flags)
        for mode in (SET_GRID, SET_PERSISTENT):
            c, o, lst, cnt = got[mode][m]
            assert np.array_equal(c, cw) and np.array_equal(o, oc) and (cnt.n_changed, cnt.n_won, cnt.n_lost) == (nc, w, l), (mode, m)
        assert got[SET_GRID][m][2] == got[SET_PERSISTENT][m][2]
    assert got[SET_GRID][K] == got[SET_PERSISTENT][K]


@pytest.mark.parametrize("n", [3, 7])
def test_a_members_own_turn_between_set_sweeps(gpu_engine_cls, oracle, stage_mode, n):
    """raftq_cycle_packed on a masked member between two set sweeps: both equal the reference"""
    g = G0
    rng = np.random.default_rng(17800 + n)
    sts = _states(n, g, 17800 + 10 * n)
    es = _load(gpu_engine_cls, sts)
    flags = SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED
    committed = [st.committed for st in sts]
    with SweepSet(es, voters=True) as s:
        for rnd in range(2):
            per, tot = s.sweep(flags)
            for m, (e, st) in enumerate(zip(es, sts)):
                cw, nc, oc, w, l = _want(oracle, st, committed[m], flags)
                assert (per[m].n_changed, per[m].n_won, per[m].n_lost) == (nc, w, l), (rnd, m)
                assert np.array_equal(e.read_committed(), cw) and np.array_equal(e.read_outcome(), oc), (rnd, m)
                committed[m] = cw
            if rnd:
                break
            # the masked member's own batching turn: acks and votes in, its own masked sweep, its advance list out
            st, e = sts[0], es[0]
            dg, dp = rng.integers(0, g, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
            dv = rng.integers(0, 14, 1500).astype(np.uint64)
            vg, vp = rng.integers(0, g, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
            vv = rng.integers(1, 3, 1500).astype(np.uint8)
            st.match = oracle.apply_deltas(st.match, dg, dp, dv)
            st.votes = oracle.apply_vote_deltas(st.votes, vg, vp, vv)
            cw, nc, oc, w, l = _want(oracle, st, committed[0], flags)
            assert nc > 0
            adv16, total, c = e.cycle_packed(flags, e.pack_deltas16(dg, dp, dv), e.pack_vote_deltas(vg, vp, vv))
            assert total == nc and (c.n_changed, c.n_won, c.n_lost) == (nc, w, l)
            gr, old, new = _advances(committed[0], cw)
            assert np.array_equal(adv16["group"], gr) and np.array_equal(adv16["new_commit"], new)
            assert np.array_equal(e.read_committed(), cw) and np.array_equal(e.read_outcome(), oc)
            committed[0] = cw
            # ... and the other members move too, so that the second set sweep decides something everywhere
            for m in (1, 2):
                dg, dp = rng.integers(0, g, 1500).astype(np.uint64), rng.integers(0, n, 1500).astype(np.uint32)
                dv = rng.integers(5, 20, 1500).astype(np.uint64)
                es[m].apply_deltas(dg, dp, dv)
                sts[m].match = oracle.apply_deltas(sts[m].match, dg, dp, dv)
    _close(es)


# ---- the set Tick --------------------------------------------------------------------------------------------------------------
ET, HB, SEED, TICKS = 10, 1, 0x5eed, 14
GT = 2500  # three 1,024-group blocks, the last one partial


@functools.lru_cache(maxsize=None)
def _tick_plan(n, me):
    """inputs of the three members, once: roles mixed, timers spread up to the election tick, masks that leave self out of a good
    part of the groups"""
    rng = np.random.default_rng(18000 + 16 * n + me)
    plan = []
    for m in range(K):
        role = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), GT)
        elapsed = rng.integers(0, ET, GT).astype(np.uint32)
        voters = rng.integers(0, 1 << n, GT).astype(np.uint16)
        voters[rng.permutation(GT)[:4]] = [0, (1 << n) - 1, 1 << me, ((1 << n) - 1) & ~(1 << me)]
        plan.append((role, elapsed, voters))
    return plan


def _tick_engines(n, me, plan, switch0=True, self0=True):
    """member 0: masks + switch + self; member 1: masks, the switch off; member 2: no masks"""
    from raftsql_amd.engine import QuorumEngine
    from raftsql_amd.step import NodeEngine

    es = []
    for m, (role, elapsed, voters) in enumerate(plan):
        e = NodeEngine(GT, n, me) if (m != 0 or self0) else QuorumEngine(GT, n)
        e.set_timers(ET, HB, SEED)
        e.load_roles(role, elapsed)
        if m < 2:
            e.load_voters(voters)
        if m == 0 and switch0:
            e._chk(e._lib.raftq_tick_set_voters(e._h, 1))
        es.append(e)
    return es


def _same_tick(e, t, what):
    for a, b in zip(e.read_tick(), t.read_tick()):
        assert np.array_equal(a, b), what
    (h, nh), (th, tnh) = e.collect_hups(), t.collect_hups()
    (b, nb), (tb, tnb) = e.collect_beats(), t.collect_beats()
    assert nh == tnh and nb == tnb and np.array_equal(h, th) and np.array_equal(b, tb), what
    return nh, nb


@pytest.mark.parametrize("n,me", [(3, 1), (5, 0), (9, 8)])
def test_set_tick(gpu_engine_cls, oracle, n, me):
    """after every tick each member equals a twin ticked alone with raftq_tick, and the reference"""
    plan = _tick_plan(n, me)
    es, twins = _tick_engines(n, me, plan), _tick_engines(n, me, plan)
    unswitched = _tick_engines(n, me, plan, switch0=False)[0:1]  # member 0 as the default would tick it
    el = [p[1].copy() for p in plan]
    differs_act = differs_el = False
    hups = beats = 0
    with SweepSet(es, voters=True) as s:
        for t in range(TICKS):
            s.tick()
            s.wait()
            for m, (e, tw) in enumerate(zip(es, twins)):
                what = (n, me, "tick", t, "member", m)
                tw.tick()
                nh, nb = _same_tick(e, tw, what)
                role, _, voters = plan[m]
                if m == 0:
                    want = M.tick_array(oracle, role, el[m], voters, me, ET, HB, SEED, t)
                else:  # the switch is off, or there are no masks: Tick reads no mask
                    want = oracle.tick(role, el[m], ET, HB, SEED, t)
                act, got_el, got_role = e.read_tick()
                assert np.array_equal(got_el, want[0]) and np.array_equal(act, want[1]) and (nh, nb) == (want[2], want[3]), what
                assert np.array_equal(got_role, role), what
                el[m] = want[0]
                hups, beats = hups + nh, beats + nb
            unswitched[0].tick()
            ua, ue, _ = unswitched[0].read_tick()
            a0, e0, _ = es[0].read_tick()
            differs_act, differs_el = differs_act or bool((ua != a0).any()), differs_el or bool((ue != e0).any())
        # the case has teeth: timers fired, and promotable() changed member 0's actions and timers
        assert hups > 50 and beats > 0 and differs_act and differs_el
    _close(es + twins + unswitched)


def test_set_tick_follows_masks_switch_and_own_ticks(gpu_engine_cls, oracle):
    """the set's tick table goes stale when a member's masks or switch change, or a member ticks on its own: every dispatch still
    equals the twins ticked alone; and a set in which nobody asks promotable() launches the plain dispatch"""
    n, me = 5, 2
    plan = _tick_plan(n, me)
    es, twins = _tick_engines(n, me, plan), _tick_engines(n, me, plan)

    def both(f):
        for pair in zip(es, twins):
            f(*pair)

    with SweepSet(es, voters=True) as s:
        def tick_and_compare(what):
            s.tick()
            s.wait()
            for m, (e, tw) in enumerate(zip(es, twins)):
                tw.tick()
                _same_tick(e, tw, (what, m))

        for t in range(3):
            tick_and_compare(("start", t))
        es[1].tick(), twins[1].tick()  # a member ticked on its own: it is one tick ahead of the others from here on
        tick_and_compare("after a member's own tick")
        for x in (es[1], twins[1]):  # the second masked member opts in
            x._chk(x._lib.raftq_tick_set_voters(x._h, 1))
        tick_and_compare("after the switch went on")
        other = _tick_plan(n, 0)[0][2]
        for x in (es[0], twins[0]):  # other masks, in another array or the same: the values are what counts
            x.load_voters(None)
            x.load_voters(other)
        for x in (es[2], twins[2]):  # masks arrive on the member that had none, with the switch
            x.load_voters(plan[2][2])
            x._chk(x._lib.raftq_tick_set_voters(x._h, 1))
        for t in range(3):
            tick_and_compare(("after masks changed", t))
        for x in es + twins:  # nobody asks any more: the plain dispatch, then the masked one again
            x._chk(x._lib.raftq_tick_set_voters(x._h, 0))
        for t in range(2):
            tick_and_compare(("switches off", t))
        for x in (es[0], twins[0]):
            x._chk(x._lib.raftq_tick_set_voters(x._h, 1))
        for t in range(8):
            tick_and_compare(("switch on again", t))
    _close(es + twins)


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


def test_failed_calls_apply_nothing(gpu_engine_cls, oracle):
    n, me = 5, 1
    plan = _tick_plan(n, me)
    # member 0 holds masks and the switch but no self slot (a plain handle: neither raftq_set_self nor raftq_load_node)
    es, twins = _tick_engines(n, me, plan, self0=False), _tick_engines(n, me, plan, switch0=False)
    with SweepSet(es, voters=True) as s:
        rc, msg = _code(s.tick)
        assert rc == RAFTQ_ESTATE and "raftq_set_tick" in msg and "promotable()" in msg
        # nobody ticked: with the switch off again every member ticks in step with a twin that never saw the failed call
        es[0]._chk(es[0]._lib.raftq_tick_set_voters(es[0]._h, 0))
        for t in range(12):
            s.tick()
            s.wait()
            for m, (e, tw) in enumerate(zip(es, twins)):
                tw.tick()
                _same_tick(e, tw, ("after the refused tick", t, m))
    _close(es + twins)
    # a masked set sweep with RAFTQ_SWEEP_LDS: RAFTQ_EINVAL, committed / outcome as they were
    sts = _states(n, G0, 18500)
    es = _load(gpu_engine_cls, sts)
    with SweepSet(es, voters=True) as s:
        s.sweep(SWEEP_VOTES)
        before = [(e.read_committed(), e.read_outcome()) for e in es]
        assert _code(s.sweep_async, SWEEP_COMMIT | SWEEP_LDS)[0] == RAFTQ_EINVAL
        assert _code(s.sweep_async, SWEEP_COMMIT | SWEEP_VOTES | SWEEP_LDS)[0] == RAFTQ_EINVAL
        s.wait()
        for e, (c, o), st in zip(es, before, sts):
            assert np.array_equal(e.read_committed(), c) and np.array_equal(c, st.committed) and np.array_equal(e.read_outcome(), o)
        per, tot = s.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT)  # ... and the set goes on working
        assert per[0].n_changed == R.commit_advance(sts[0].match, sts[0].committed, sts[0].voters)[1]
    _close(es)


def test_the_default_restated(gpu_engine_cls):
    """raftq_set_create still refuses a masked handle, and a member of a plain set still refuses raftq_load_voters"""
    n = 5
    st = State(n, G0, 18600)
    with st.load(gpu_engine_cls(G0, n)) as a, st.load(gpu_engine_cls(G0, n), voters=False) as b, st.load(gpu_engine_cls(G0, n)) as c:
        rc, msg = _code(SweepSet, [a, b])
        assert rc == RAFTQ_ESTATE and "raftq_set_create:" in msg and "voter masks" in msg
        with SweepSet([b]) as s:
            rc, msg = _code(b.load_voters, st.voters)
            assert rc == RAFTQ_ESTATE and "sweep set" in msg
            assert _code(b.apply_voter_deltas, b.pack_voter_deltas([0], [1], [0]))[0] == RAFTQ_ESTATE
            assert _code(b.clone_state_from, a)[0] == RAFTQ_ESTATE
        # the new constructor shares the other refusals
        with SweepSet([a, b], voters=True) as s:
            assert _code(SweepSet, [a], voters=True)[0] == RAFTQ_ESTATE  # already a member
            assert _code(SweepSet, [c, c], voters=True)[0] == RAFTQ_EINVAL  # duplicate
            assert _code(a.set_stream, 0)[0] == RAFTQ_ESTATE
            assert a.get_stream() == s.get_stream() == b.get_stream()
        assert _code(SweepSet, [], voters=True)[0] == RAFTQ_EINVAL
        assert a.sweep(SWEEP_COMMIT | SWEEP_NO_ADOPT).n_changed == R.commit_advance(st.match, st.committed, st.voters)[1]
