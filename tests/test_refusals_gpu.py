"""GPU: a call that fails has applied nothing -- the promise of include/raftq.h (the validated ingest, the batching turn),
include/raftq_step.h (malformed Step batches) and include/raftq_wire.h (raftq_propose_frames), held over the WHOLE handle.

Every case: snapshot(e) -- every key of read_node(), read_match(), read_votes(), read_voters(), the three arrays of read_tick(),
read_committed(), narrow(), self_max() -- is taken before the call and after it and must be equal byte for byte; the call returns
its documented code with a text; canaries on the caller's output arrays stand (where a header calls an output unspecified after a
refusal: behind its capacity); and then the next calls are whole (tests/_refusals.py::probe): the refused batch without its bad
record, a list-walk Step batch over the refusal's groups, a Tick with its lists, vote deltas on the refusal's slots, an adopted
gated sweep with its changed list, a raftq_propose_frames and a raftq_step_frames_respond -- on the handle, held to the references
(oracle.pyoracle, oracle.pywire, tests/ref_step_voters.py, ref_tick_members.py, ref_bcast_members.py, ref_voters.py), and on a twin
that was loaded identically and never saw a refusal, held to the handle: what a refusal leaves in state that cannot be read back
(list words, vote claims, stamps, the tick number, the in-flight count) shows there.

Device verdicts are taken per wave and handed from kernel to kernel through a word, so their batches have 513 records -- two
workgroups and a lone lane -- with the bad record at 0, 63, 64, 255, 256 and 512 in turn, good records in every wave, and a good
record for the bad one's group (or slot) in another workgroup.  Before anything is compared the reference side asserts that the
good records alone do change the state."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from raftsql_amd import _lib
from raftsql_amd import step as S
from raftsql_amd._lib import CYCLE_SEGMENTED, SWEEP_CHANGED, SWEEP_COMMIT
from raftsql_amd.engine import RaftqError
from tests import _refusals as F
from tests import ref_step_voters as V
from tests._refusals import CANARY, NREC, POSITIONS, SHAPES, ProposeArgs, Ref, probe, same_snapshot, snapshot

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = _lib.RAFTQ_EINVAL, _lib.RAFTQ_ESTATE
G_SWEEP, G_PLAIN = 4099, 2500  # the ragged shape of tests/test_narrow_gpu.py where a sweep is part of the case; 2,500 elsewhere


def _refused(e, call, code, what, words=()):
    """checks 1 to 3 of a case: snapshot, the documented code with a text, the same snapshot"""
    before = snapshot(e)
    with pytest.raises(RaftqError) as ei:
        call()
    text = str(ei.value)
    assert ei.value.code == code and text.split(":", 1)[-1].strip(), (what, text)
    same_snapshot(before, snapshot(e), what)
    for w in words:
        assert w in text, (what, text)
    return text


def _insert(a, i, rec):
    return np.concatenate([a[:i], rec, a[i:]])


def _elsewhere(i):
    """a good record's index in another workgroup than the bad record's"""
    return (i + 256) % (NREC - 1)


# ---- 1. the validated ingest: raftq_apply_deltas, raftq_apply_vote_deltas, raftq_cycle, raftq_cycle_packed -----------------------
@functools.lru_cache(maxsize=None)
def _ingest_good(N, me):
    """512 match deltas (in 512 groups the slot furthest behind acknowledges the leader's tail) and 512 vote deltas (in 512
    groups a slot with nothing recorded, where there is one, answers) -- and the assertion that they do change the state"""
    G = G_SWEEP
    s = F.base_state(G, N, me, 21000 + N)
    rng = np.random.default_rng(21100 + N)
    g = rng.choice(G, NREC - 1, replace=False).astype(np.uint64)
    gi = g.astype(np.int64)
    rows = s.match[:, gi].astype(np.float64)
    rows[me] = np.inf
    p = rows.argmin(axis=0).astype(np.uint32)
    m = s.match[me, gi].copy()
    vg = rng.choice(G, NREC - 1, replace=False).astype(np.uint64)
    vi = vg.astype(np.int64)
    free = s.votes[:, vi] == 0
    free[me] = False
    vp = np.where(free.any(axis=0), free.argmax(axis=0), (me + 1) % N).astype(np.uint32)
    vv = (1 + (vg & np.uint64(1))).astype(np.uint8)
    # the good records alone change the state: Match words raised, votes recorded, commit indices moved by them
    match1 = pyoracle.apply_deltas(s.match, g, p, m)
    votes1 = pyoracle.apply_vote_deltas(s.votes, vg, vp, vv)
    assert (match1 > s.match).sum() > 100 and ((s.votes == 0) & (votes1 != 0)).sum() > 50
    assert (pyoracle.commit_advance(match1, s.committed)[0] != pyoracle.commit_advance(s.match, s.committed)[0]).sum() > 20
    return g, p, m, vg, vp, vv


_RANGE_KINDS = (("group", "G"), ("group", "far"), ("peer", "N"), ("peer", 255))
_VOTE_KINDS = _RANGE_KINDS + (("vote", 0), ("vote", 3))


def _broken(rec, kind, G, N, packed=False):
    field, v = kind
    v = {"G": G, "far": 0xFFFFFFFF if packed else 1 << 63, "N": N}.get(v, v)
    rec = rec.copy()
    rec[field] = v
    return rec


def _ingest_case(e_cls, N, me, variant, pos, k):
    """-> (refuse(e), again(x), again_want(R), touched groups)"""
    G = G_SWEEP
    g, p, m, vg, vp, vv = _ingest_good(N, me)
    D, D16, VD = e_cls.pack_deltas(g, p, m), e_cls.pack_deltas16(g, p, m), e_cls.pack_vote_deltas(vg, vp, vv)
    j = _elsewhere(pos)
    touched = np.concatenate([g, vg]).astype(np.int64)

    def moved_by_cycle(R, votes=True):
        s = R.s
        s.match[:] = pyoracle.apply_deltas(s.match, g, p, m)
        if votes:
            s.votes[:] = pyoracle.apply_vote_deltas(s.votes, vg, vp, vv)
        want, _ = pyoracle.commit_advance(s.match, s.committed)
        old = s.committed.copy()
        s.committed[:] = want
        at = np.flatnonzero(want != old)
        return at, old[at], want[at]

    if variant == "apply_deltas":
        bad = _insert(D, pos, _broken(D[j:j + 1], _RANGE_KINDS[k % 4], G, N))

        def refuse(e):
            e.apply_deltas(bad["group"], bad["peer"], bad["match"])

        def again(x):
            x.apply_deltas(g, p, m)
            return dict(match=x.read_match())

        def again_want(R):
            R.s.match[:] = pyoracle.apply_deltas(R.s.match, g, p, m)
            return dict(match=R.s.match.copy())
    elif variant == "apply_vote_deltas":
        bad = _insert(VD, pos, _broken(VD[j:j + 1], _VOTE_KINDS[k % 6], G, N))

        def refuse(e):
            e.apply_vote_deltas(bad["group"], bad["peer"], bad["vote"])

        def again(x):
            x.apply_vote_deltas(vg, vp, vv)
            return dict(votes=x.read_votes())

        def again_want(R):
            R.s.votes[:] = pyoracle.apply_vote_deltas(R.s.votes, vg, vp, vv)
            return dict(votes=R.s.votes.copy())
    elif variant in ("cycle, a bad match delta", "cycle, a bad vote delta"):
        if variant.endswith("match delta"):
            bd, bv = _insert(D, pos, _broken(D[j:j + 1], _RANGE_KINDS[k % 4], G, N)), VD
        else:
            bd, bv = D, _insert(VD, pos, _broken(VD[j:j + 1], _VOTE_KINDS[k % 6], G, N))
        fl = SWEEP_COMMIT | SWEEP_CHANGED

        def refuse(e):
            out = np.frombuffer(bytearray([CANARY]) * (G * e._ADV_DT.itemsize), e._ADV_DT)
            try:
                e.cycle(fl, bd, bv, out=out)
            finally:
                assert (out.view(np.uint8) == CANARY).all(), "a refused turn wrote its advance list"

        def again(x):
            adv, total, cnt = x.cycle(fl, D, VD)
            return dict(group=adv["group"].copy(), old=adv["old_commit"].copy(), new=adv["new_commit"].copy(), total=total, n_changed=cnt.n_changed)

        def again_want(R):
            at, old, new = moved_by_cycle(R)
            return dict(group=at.astype(np.uint64), old=old, new=new, total=len(at), n_changed=len(at))
    else:
        segmented = variant.startswith("cycle_packed segmented")
        if variant.endswith("match delta"):
            bd, bv = _insert(D16, pos, _broken(D16[j:j + 1], _RANGE_KINDS[k % 4], G, N, packed=True)), VD
        else:
            bd, bv = D16, _insert(VD, pos, _broken(VD[j:j + 1], _VOTE_KINDS[k % 6], G, N))
        fl = SWEEP_COMMIT | (CYCLE_SEGMENTED if segmented else SWEEP_CHANGED)

        def turn(x, d, v):
            if not segmented:
                adv, total, cnt = x.cycle_packed(fl, d, v)
                return dict(group=adv["group"].astype(np.uint64), new=adv["new_commit"].copy(), total=total)
            _, total, _ = x.cycle_packed(fl, d, v, cap=G, inplace=True, want_counts=False)
            adv = x.advance_list_from_segments()
            return dict(group=adv["group"].astype(np.uint64), new=adv["new_commit"].copy(), total=total)

        def refuse(e):
            turn(e, bd, bv)

        def again(x):
            return turn(x, D16, VD)

        def again_want(R):
            at, _, new = moved_by_cycle(R)
            return dict(group=at.astype(np.uint64), new=new, total=len(at))
    return refuse, again, again_want, touched


INGEST_VARIANTS = ("apply_deltas", "apply_vote_deltas", "cycle, a bad match delta", "cycle, a bad vote delta",
                   "cycle_packed, a bad match delta", "cycle_packed segmented, a bad vote delta")


@pytest.mark.parametrize("variant", INGEST_VARIANTS)
@pytest.mark.parametrize("N,me", SHAPES)
def test_validated_ingest_applies_nothing(gpu_engine_cls, oracle, N, me, variant):
    """group = G, group = 2^63 (2^32 - 1 in the packed record), peer = N, peer = 255, vote bytes 0 and 3, dealt over the six
    positions; turn flags with SWEEP_CHANGED and with CYCLE_SEGMENTED.  Both device words are set on entry and still are after."""
    base = F.base_state(G_SWEEP, N, me, 21000 + N)
    for k, pos in enumerate(POSITIONS):
        what = f"{variant}, bad record {pos}, N={N}"
        refuse, again, again_want, touched = _ingest_case(gpu_engine_cls, N, me, variant, pos, k + INGEST_VARIANTS.index(variant))
        with F.engine(base) as e, F.engine(base) as t:
            assert e.narrow() and e.self_max() == me, "the self-max word and the narrow word are meant to be set on entry"
            _refused(e, lambda: refuse(e), EINVAL, what)
            assert e.narrow() and e.self_max() == me
            probe(e, t, Ref(base), touched, 21200 + pos, again, again_want, what)


@pytest.mark.parametrize("N,me", SHAPES)
def test_refused_turn_leaves_the_rows_and_the_mirror_to_every_sweep(gpu_engine_cls, oracle, N, me):
    """behind a refused turn every dispatch tests/test_narrow_gpu.py::_check runs -- plain and gated, the set's grid and its
    persistent walk, NO_ADOPT -- equals the oracle over the UNCHANGED rows: the mirror's offsets are untouched as well"""
    from tests.test_narrow_gpu import _check

    base = F.base_state(G_SWEEP, N, me, 21000 + N)
    refuse, _, _, _ = _ingest_case(gpu_engine_cls, N, me, "cycle, a bad match delta", 256, 2)
    with F.engine(base) as e:
        assert e.narrow() and e.self_max() == me
        _refused(e, lambda: refuse(e), EINVAL, "cycle")
        _check(oracle, [e], [[base.match.copy(), base.committed.copy(), base.first_idx.copy(), base.votes.copy()]])
        assert e.narrow() and e.self_max() == me


# ---- 2. malformed Step batches: raftq_step_batch, raftq_step_submit / _collect, raftq_step_submit_packed ---------------------------
def _start(N, me, masked, seed):
    if masked:
        voters, s = F.base_masks(G_PLAIN, N, me, seed)
        return s, voters
    return F.base_state(G_PLAIN, N, me, seed), None


@functools.lru_cache(maxsize=None)
def _step_good(N, me, masked):
    s, voters = _start(N, me, masked, 22000 + N)
    rng = np.random.default_rng(22100 + N)
    g = rng.choice(G_PLAIN, NREC - 1, replace=False)
    role = s.role[g]
    typ = np.where(role == S.ROLE_LEADER, S.MSG_APP_RESP, np.where(role == S.ROLE_CANDIDATE, S.MSG_VOTE_RESP, S.MSG_HEARTBEAT))
    rows = s.match[:, g].astype(np.float64)
    rows[me] = np.inf
    free = s.votes[:, g] == 0
    free[me] = False
    frm = np.where(role == S.ROLE_CANDIDATE, np.where(free.any(axis=0), free.argmax(axis=0), (me + 1) % N), rows.argmin(axis=0))
    good = S.pack_msgs(g.astype(np.uint64), typ, term=s.term[g], frm=frm, index=s.last_index[g], commit=s.last_index[g])
    # the good records alone change the state: Match words raised, votes recorded, commit indices moved
    R = Ref(s, voters)
    R.step(good)
    # (a candidate that wins clears its votes again: few recorded votes are left standing at the end of the batch)
    assert (R.s.match > s.match).sum() > 50 and ((s.votes == 0) & (R.s.votes != 0)).sum() > 0 and (R.s.committed != s.committed).sum() > 20
    assert (R.s.role != s.role).sum() > 0
    return good


_STEP_KINDS = (("group", "G"), ("from", "N"), ("type", 7), ("group", "far"))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-voters"])
@pytest.mark.parametrize("form", ["step_batch", "step_submit", "step_submit_packed"])
@pytest.mark.parametrize("N,me", SHAPES)
def test_malformed_step_batch_applies_nothing(gpu_engine_cls, oracle, N, me, form, masked):
    """group >= G, from >= N, a type Step does not take.  A refused submit does not count as a batch in flight: the probe's batches
    go through.  raftq_step_batch's `out` keeps its canaries."""
    s, voters = _start(N, me, masked, 22000 + N)
    good = _step_good(N, me, masked)
    packed = form == "step_submit_packed"
    for k, pos in enumerate(POSITIONS):
        kind = _STEP_KINDS[(k + len(form)) % 4]
        what = f"{form}, bad record {pos} ({kind[0]}), N={N}"
        bad = _insert(good, pos, _broken(good[_elsewhere(pos):_elsewhere(pos) + 1], kind, G_PLAIN, N, packed=packed))

        def run(x, m):
            if form == "step_batch":
                out = np.frombuffer(bytearray([CANARY]) * (len(m) * 64), S.OUT_DT)
                rc = x._lib.raftq_step_batch(x._h, m.ctypes.data, len(m), out.ctypes.data, C.byref(_lib.StepCounts()))
                if rc != 0:
                    assert (out.view(np.uint8) == CANARY).all(), "a refused batch wrote result records"
                x._chk(rc)
                return dict(outs=out)
            if packed:
                x.step_submit_packed(S.pack_msgs40(m))
            else:
                x.step_submit(m)
            return dict(outs=x.step_collect()[0])

        with F.engine(s, voters) as e, F.engine(s, voters) as t:
            _refused(e, lambda: run(e, bad), EINVAL, what, ["malformed"])
            probe(e, t, Ref(s, voters), good["group"], 22200 + pos, lambda x: run(x, good), lambda R: dict(outs=R.step(good)), what)


# ---- 2b. the frame forms: raftq_step_frames, raftq_step_frames_packed, raftq_step_frames_respond --------------------------------
# include/raftq_wire.h gives these three NO device verdict: a frame that names a group >= G or a sender >= N, is of a kind a peer
# never sends, is addressed to another slot or did not parse is RAFTQ_MSGF_SKIP -> RAFTQ_OUT_SKIPPED ("a node has to survive
# whatever bytes a peer throws at it"), and the rest of the batch is stepped.  So the position table holds them to THAT: the bad
# frame is skipped wherever it sits and every good frame is applied.  What the header does document as refusals of these forms --
# a bad `form`, an array that is not page-locked, a cap below the bound, a batch in flight, masks without the switch -- are host
# verdicts and sit in section 4.
def _frame_calls(e, fs, foff, at=None):
    """-> {form: call() -> (records as raftq_wire_decode would give them, results, respond bytes | None)}"""
    from raftsql_amd import wire as W_
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests.test_respond_gpu import _call

    n = len(foff) - 1
    ps, po = pinned_copy(np.ascontiguousarray(fs)), pinned_copy(np.ascontiguousarray(foff, np.uint64))

    def frames():
        gm, _, go, _ = e.step_frames(ps, po, pinned_empty(n, W_.WIRE_MSG_DT), pinned_empty(8, W_.WIRE_ENT_DT))
        return gm.copy(), go, None

    def packed(form=W_.FORM_40, stream=ps):
        nar, wide, _, go, _, _ = e.step_frames_packed(stream, po, form, pinned_empty(n, W_._FORM_DT[W_.FORM_40]), pinned_empty(n, W_.WIRE_MSG_DT),
                                                      pinned_empty(8, W_.WIRE_ENT_DT))
        return W_.expand_packed(nar, wide, e.self_peer, W_.FORM_40), go, None

    def respond():
        gm, _, go, got_s, _, got_po, _, rc = _call(e, fs, foff, 8, at)
        return gm.copy(), go, (bytes(got_s), np.asarray(got_po).copy(), int(rc.n_msgs))

    return dict(step_frames=frames, step_frames_packed=packed, step_frames_respond=respond)


_FRAME_KINDS = (("group", "G"), ("from", "N"), ("type", 7), ("to", "other"))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-voters"])
@pytest.mark.parametrize("form", ["step_frames", "step_frames_packed", "step_frames_respond"])
@pytest.mark.parametrize("N,me", SHAPES)
def test_frame_forms_skip_a_bad_frame_and_apply_the_rest(gpu_engine_cls, oracle, N, me, form, masked):
    """the 513-frame position table for the forms whose documented answer to group >= G, from >= N, an unknown type or another
    addressee is a skipped frame, not a refused batch: records, results, responses and the state afterwards are the references'"""
    from oracle import pywire as W
    from tests import _stepgen
    from tests import ref_bcast_members as B

    s, voters = _start(N, me, masked, 22000 + N)
    good = _step_good(N, me, masked)
    wm = np.zeros(len(good), W.WIRE_MSG_DT)
    for f in ("group", "term", "log_term", "index", "commit", "reject_hint", "from", "type", "reject"):
        wm[f] = good[f]
    wm["to"] = me
    for k, pos in enumerate(POSITIONS):
        kind = _FRAME_KINDS[(k + len(form)) % 4]
        what = f"{form}, bad frame {pos} ({kind[0]}), N={N}"
        bad = wm[_elsewhere(pos):_elsewhere(pos) + 1].copy()
        bad[kind[0]] = {"G": G_PLAIN, "N": N, "other": (me + 1) % N}.get(kind[1], kind[1])
        fs, foff = W.wire_encode(_insert(wm, pos, bad))
        R = Ref(s, voters)
        at = B.leaders_bitmap(np.random.default_rng(22300 + pos), R.s, 1.0) if form == "step_frames_respond" else None
        want_m, _, want_o, want_w, want_po, want_ans, _ = B.respond_want(R.s, R.masks, fs, foff, at)
        assert want_o["type"][pos] == S.OUT_SKIPPED and (np.delete(want_o["type"], pos) != S.OUT_SKIPPED).all()
        assert (R.s.match > s.match).sum() > 50 and (R.s.committed != s.committed).sum() > 20  # the good frames do change the state
        with F.engine(s, voters) as e:
            gm, go, resp = _frame_calls(e, np.asarray(fs), foff, at)[form]()
            assert gm.tobytes() == want_m.tobytes(), f"{what}: records"
            go = go.copy()
            if resp is not None:
                assert np.array_equal((go["flags"] & B.ANSWERED) != 0, want_ans), f"{what}: answered flags"
                go["flags"] &= np.uint8(~B.ANSWERED & 0xFF)
                want_s = W.wire_encode(want_w)[0] if len(want_w) else np.zeros(0, np.uint8)
                assert resp[0] == bytes(want_s) and np.array_equal(resp[1], want_po) and resp[2] == len(want_w), f"{what}: responses"
            assert go.tobytes() == want_o.tobytes(), f"{what}: results"
            _stepgen.assert_same_state(e, R.s)


# ---- 3. raftq_propose_frames -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _propose_good(N, me, masked, n_host):
    s, voters = _start(N, me, masked, 23000 + N)
    rng = np.random.default_rng(23100 + N + n_host)
    led = np.flatnonzero(s.role == S.ROLE_LEADER)
    groups = rng.permutation(led)[:NREC]
    batch = F.propose_batch(s, voters, groups, rng, n_host)
    # the good records alone change the state: the tail, its term and the leader's own Match move
    R = Ref(s, voters)
    F.propose_want(R, *batch)
    gi = groups.astype(np.int64)
    assert (R.s.last_index[gi] == s.last_index[gi] + 1).all() and (R.s.match[me, gi] > s.match[me, gi]).all()
    return batch


def _room(batch, N):
    props, pe, pool, hm, he = batch
    return len(pool) + 128 * (len(hm) + len(props) * (N - 1)) + 4096


_REASONS = (("payload", "an entry's payload lies outside the pool"), ("group", "its group is out of range"), ("count", "it carries no entries"),
            ("range", "its entries lie outside prop_ents[]"), ("follower", "this node does not lead its group"), ("twice", "its group is named twice"),
            ("no member", "this node is no member of its group"), ("commits", "its append would move the commit index"))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-members"])
@pytest.mark.parametrize("N,me", SHAPES)
def test_refused_proposals_append_nothing(gpu_engine_cls, oracle, N, me, masked):
    """the six record reasons unmasked, all eight with masks and raftq_bcast_set_voters on, dealt over the six positions"""
    s0, voters0 = _start(N, me, masked, 23000 + N)
    props, pe, pool, hm, he = _propose_good(N, me, masked, 40)
    reasons = _REASONS if masked else _REASONS[:6]
    for k, (reason, words) in enumerate(reasons):
        pos = POSITIONS[(k + N) % len(POSITIONS)]
        what = f"{reason}, bad record {pos}, N={N}"
        s, voters = V.copy_state(s0), None if voters0 is None else voters0.copy()
        bp, be = props.copy(), pe.copy()
        g = int(props["group"][pos])
        if reason == "payload":
            be["data_off"][pos], be["data_len"][pos] = len(pool), 8
        elif reason == "group":
            bp["group"][pos] = G_PLAIN
        elif reason == "count":
            bp["n_ents"][pos] = 0
        elif reason == "range":
            bp["ent_first"][pos] = len(pe)
        elif reason == "follower":
            s.role[g] = S.ROLE_FOLLOWER
        elif reason == "twice":
            bp["group"][pos] = props["group"][_elsewhere(pos)]
        elif reason == "no member":
            voters[g] &= ~np.uint16(1 << me)
        else:
            voters[g] = 1 << me
        rest = np.delete(props, pos)  # the refused batch with its bad record taken out (the entries stay where they are)
        bad = ProposeArgs(bp, be, pool, hm, he, N, _room((props, pe, pool, hm, he), N))
        good = ProposeArgs(rest, pe, pool, hm, he, N, bad.room)

        def refuse(e):
            rc, c = bad.call(e)
            assert rc == 0 or (c.n_msgs, c.bytes) == (0, 0), what
            e._chk(rc)

        with F.engine(s, voters) as e, F.engine(s, voters) as t:
            named = [] if reason == "twice" else [f"record {pos}:"]  # (of a group named twice either record may be the second to arrive)
            _refused(e, lambda: refuse(e), EINVAL, what, named + [words, "nothing was appended"])
            probe(e, t, Ref(s, voters), props["group"], 23200 + pos, good.whole,
                  lambda R: F.propose_outputs(F.propose_want(R, rest, pe, pool, hm, he)), what)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-members"])
@pytest.mark.parametrize("N,me", SHAPES)
def test_proposals_with_an_out_that_is_too_small_append_nothing(gpu_engine_cls, oracle, N, me, masked):
    """cap one byte short, short by exactly the last frame, and 1: the call fails, counts->bytes is the size needed, nothing has
    moved; the same call with cap = counts->bytes exactly succeeds, the oracle's bytes, and the tail moves ONCE"""
    s, voters = _start(N, me, masked, 23000 + N)
    batch = _propose_good(N, me, masked, 40)
    want = F.propose_want(Ref(s, voters), *batch)
    needed = len(want[0])
    sizes = np.diff(want[1].astype(np.int64))
    last = int(sizes[sizes > 0][-1])
    a = ProposeArgs(*batch, N, needed)  # (64 bytes of canaries behind `needed`)
    with F.engine(s, voters) as e, F.engine(s, voters) as t:
        for cap in (needed - 1, needed - last, 1):
            what = f"cap {cap} of {needed}, N={N}"

            def refuse():
                rc, c = a.call(e, cap)
                assert rc == 0 or c.bytes == needed, f"{what}: counts->bytes is {c.bytes}"
                e._chk(rc)

            _refused(e, refuse, EINVAL, what, ["too small", "nothing was appended"])
        probe(e, t, Ref(s, voters), batch[0]["group"], 23300, a.whole, lambda R: F.propose_outputs(F.propose_want(R, *batch)), f"cap == needed, N={N}")


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-members"])
@pytest.mark.parametrize("N,me", SHAPES)
def test_proposals_behind_a_queued_message_the_marshal_refuses_append_nothing(gpu_engine_cls, oracle, N, me, masked):
    """to = 255, an entry range outside ents[], a payload outside the pool; first and last in msgs[], which spans two encoder
    tiles; with the message repaired the call is whole"""
    s, voters = _start(N, me, masked, 23000 + N)
    props, pe, pool, hm, he = batch = _propose_good(N, me, masked, 300)
    assert len(hm) > 256 and len(he) > 0
    room = _room(batch, N)
    with F.engine(s, voters) as e, F.engine(s, voters) as t:
        for at in (0, len(hm) - 1):
            for kind in ("to", "range", "payload"):
                what = f"queued message {at}: {kind}, N={N}"
                bm, bh = hm.copy(), he.copy()
                if kind == "to":
                    bm["to"][at] = 255
                elif kind == "range":
                    bm["ent_first"][at], bm["n_ents"][at] = len(he) + len(pe), 1
                else:
                    bm["ent_first"][at], bm["n_ents"][at] = len(he) - 1, 1
                    bh["data_off"][-1], bh["data_len"][-1] = len(pool), 8
                bad = ProposeArgs(props, pe, pool, bm, bh, N, room)
                _refused(e, lambda: e._chk(bad.call(e)[0]), EINVAL, what, ["queued message", "nothing was appended"])
        good = ProposeArgs(*batch, N, room)
        probe(e, t, Ref(s, voters), props["group"], 23400, good.whole, lambda R: F.propose_outputs(F.propose_want(R, *batch)), f"repaired, N={N}")


# ---- 4. host verdicts (N = 3): one position each, chained on one handle, the probe behind every one ------------------------------
def _tick_bufs(e, n, elect=False):
    from raftsql_amd.engine import pinned_empty

    out = pinned_empty(e.respond_cap(n) + 64, np.uint8)
    off = pinned_empty(n * (e.n_peers - 1) + 1, np.uint64)
    po = pinned_empty((2 if elect else 1) * (e.n_peers + 1), np.uint64)
    out[:] = CANARY
    return out, off, po


def test_host_verdicts_apply_nothing(gpu_engine_cls, oracle):
    """raftq_apply_term_deltas, raftq_campaign, raftq_apply_log_deltas with a group >= G; raftq_step_frames_respond, raftq_tick_frames
    and raftq_tick_elect_frames with cap one below their worst case (the two Ticks "have not ticked": the probe's Tick produces
    the lists of the reference for the same tick number); raftq_load_voters on a member of a set"""
    from raftsql_amd import wire as W_
    from raftsql_amd.engine import SweepSet, pinned_copy, pinned_empty
    from tests.test_respond_gpu import _call
    from tests.test_wire_gpu import _node_frames

    N, me, G = 3, 1, G_PLAIN
    s = F.base_state(G, N, me, 24000)
    rng = np.random.default_rng(24100)
    far = np.array([5, G], np.uint64)
    fs, foff = _node_frames(rng, 120, s, me)
    n = len(foff) - 1
    with F.engine(s) as e, F.engine(s) as t, F.engine(s) as other:
        R = Ref(s)
        out, off, po = _tick_bufs(e, 64)
        out2, off2, po2 = _tick_bufs(e, 128, elect=True)
        camp = pinned_empty(64, S.OUT_S_DT)
        fc = _frame_calls(e, np.asarray(fs), foff)
        pfoff, pmsgs, pents = pinned_copy(np.ascontiguousarray(foff, np.uint64)), pinned_empty(n, W_.WIRE_MSG_DT), pinned_empty(8, W_.WIRE_ENT_DT)

        def in_a_set():
            with SweepSet([e, other]):
                e.load_voters(V.full_masks(N, G))

        cases = [
            ("raftq_apply_term_deltas", lambda: e.apply_term_deltas(far, np.array([3, 3], np.uint64), np.array([1, 1], np.uint64)), EINVAL),
            ("raftq_campaign, a group", lambda: e.campaign(far, me), EINVAL),
            ("raftq_campaign, the slot", lambda: e.campaign(far[:1], N), EINVAL),
            ("raftq_apply_log_deltas", lambda: e.apply_log_deltas(far, 9, 1), EINVAL),
            ("raftq_step_frames_respond", lambda: _call(e, fs, foff, 8 * n, None, cap=e.respond_cap(n) - 1), EINVAL),
            ("raftq_step_frames, a pageable array", lambda: e.step_frames(np.asarray(fs).copy(), pfoff, pmsgs, pents), EINVAL),
            ("raftq_step_frames_packed, a form that is none", lambda: fc["step_frames_packed"](form=17), EINVAL),
            ("raftq_step_frames_packed, a pageable array", lambda: fc["step_frames_packed"](stream=np.asarray(fs).copy()), EINVAL),
            ("raftq_tick_frames", lambda: e.tick_frames(out, off, po, 64, cap=e.respond_cap(64) - 1), EINVAL),
            ("raftq_tick_elect_frames", lambda: e.tick_elect_frames(camp, out2, off2, po2, 64, 64, cap=e.respond_cap(128) - 1), EINVAL),
            ("raftq_load_voters on a member of a set", in_a_set, ESTATE),
        ]
        for k, (what, call, code) in enumerate(cases):
            text = _refused(e, call, code, what)
            if "tick" in what:
                assert "has not ticked" in text, text
            assert (out == CANARY).all() and (out2 == CANARY).all(), what
            probe(e, t, R, np.arange(k * 97, k * 97 + 400), 24200 + k, what=what)


def test_host_verdicts_over_voters_apply_nothing(gpu_engine_cls, oracle):
    """raftq_apply_voter_deltas (group >= G, a bit >= N), raftq_load_voters (a bit >= N), and the three switch setters with a value
    that is neither 0 nor 1: the masks and the switches keep their values -- the probe's masked calls go through"""
    N, me, G = 3, 1, G_PLAIN
    voters, s = F.base_masks(G, N, me, 24000)
    with F.engine(s, voters) as e, F.engine(s, voters) as t:
        R = Ref(s, voters)
        wide = voters.copy()
        wide[9] |= 1 << N
        cases = [
            ("raftq_apply_voter_deltas, a group", lambda: e.apply_voter_deltas(e.pack_voter_deltas(np.array([4, G], np.uint64), [3, 3])), EINVAL),
            ("raftq_apply_voter_deltas, a bit", lambda: e.apply_voter_deltas(e.pack_voter_deltas(np.array([4, 6], np.uint64), [3, 1 << N])), EINVAL),
            ("raftq_load_voters, a bit", lambda: e.load_voters(wide), EINVAL),
            ("raftq_step_set_voters(2)", lambda: e.set_step_voters(2), EINVAL),
            ("raftq_tick_set_voters(2)", lambda: e.set_tick_voters(2), EINVAL),
            ("raftq_bcast_set_voters(2)", lambda: e.set_bcast_voters(2), EINVAL),
        ]
        for k, (what, call, code) in enumerate(cases):
            _refused(e, call, code, what)
            probe(e, t, R, np.arange(k * 131, k * 131 + 400), 24300 + k, what=what)


def test_masks_without_the_switch_a_call_needs(gpu_engine_cls, oracle):
    """masks loaded, no switch on: Step, the tail reports, both device-built Ticks, the proposals and the responses are RAFTQ_ESTATE
    ("voter masks" in the text) and apply nothing; with the switches on the handle is whole"""
    from raftsql_amd.engine import pinned_empty
    from tests.test_respond_gpu import _call
    from tests.test_wire_gpu import _node_frames

    N, me, G = 3, 1, G_PLAIN
    voters, s = F.base_masks(G, N, me, 24000)
    rng = np.random.default_rng(24400)
    m = F.walk_batch(s, np.arange(0, 300), rng)
    led = np.flatnonzero(s.role == S.ROLE_LEADER)[:64]
    batch = F.propose_batch(s, voters, led, rng, 10)
    a = ProposeArgs(*batch, N, _room(batch, N))
    fs, foff = _node_frames(rng, 120, s, me)
    n = len(foff) - 1
    with F.engine(s, voters, switches=False) as e, F.engine(s, voters, switches=False) as t:
        out, off, po = _tick_bufs(e, 64)
        out2, off2, po2 = _tick_bufs(e, 128, elect=True)
        camp = pinned_empty(64, S.OUT_S_DT)
        fc = _frame_calls(e, np.asarray(fs), foff)
        cases = [
            ("raftq_step_batch", lambda: e.step_batch(m)),
            ("raftq_step_submit", lambda: e.step_submit(m)),
            ("raftq_step_submit_packed", lambda: e.step_submit_packed(S.pack_msgs40(m))),
            ("raftq_step_frames", fc["step_frames"]),
            ("raftq_step_frames_packed", fc["step_frames_packed"]),
            ("raftq_apply_log_deltas", lambda: e.apply_log_deltas(led.astype(np.uint64), s.last_index[led], s.last_term[led])),
            ("raftq_tick_frames", lambda: e.tick_frames(out, off, po, 64)),
            ("raftq_tick_elect_frames", lambda: e.tick_elect_frames(camp, out2, off2, po2, 64, 64)),
            ("raftq_propose_frames", lambda: e._chk(a.call(e)[0])),
            ("raftq_step_frames_respond", lambda: _call(e, fs, foff, 8 * n, None)),
        ]
        for what, call in cases:
            _refused(e, call, ESTATE, what, ["voter masks"])
            assert (out == CANARY).all() and (out2 == CANARY).all(), what
        for x in (e, t):
            x.set_step_voters(True)
            x.set_tick_voters(True)
            x.set_bcast_voters(True)
        probe(e, t, Ref(s, voters), np.arange(0, 400), 24500, what="the switches on")


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "over-voters"])
def test_calls_refused_while_a_step_batch_is_in_flight(gpu_engine_cls, oracle, masked):
    """every call that names it returns RAFTQ_ESTATE while a batch is in flight -- the sweeps, Tick in all its forms, the deltas, the
    tail reports, every raftq_load_* and raftq_read_*, the setters, raftq_step_batch and the frame forms, the device-built rounds
    (the read-backs too, so the snapshot is the twin's: it submitted the same batch and made none of the calls); the batch collects
    whole; a refused setter leaves its switch, the message flags and the result format where they were"""
    from raftsql_amd.engine import pinned_empty
    from tests.test_respond_gpu import _call
    from tests.test_wire_gpu import _node_frames

    N, me, G = 3, 1, G_PLAIN
    s, voters = _start(N, me, masked, 24000)
    rng = np.random.default_rng(24600)
    m = F.walk_batch(s, np.arange(100, 400), rng)
    led = np.flatnonzero(s.role == S.ROLE_LEADER)[-64:]
    batch = F.propose_batch(s, voters, led, rng, 10)
    a = ProposeArgs(*batch, N, _room(batch, N))
    fs, foff = _node_frames(rng, 120, s, me)
    n = len(foff) - 1
    g2 = np.array([7, 8], np.uint64)
    with F.engine(s, voters) as e, F.engine(s, voters) as t:
        R = Ref(s, voters)
        out, off, po = _tick_bufs(e, 64)
        out2, off2, po2 = _tick_bufs(e, 128, elect=True)
        camp = pinned_empty(64, S.OUT_S_DT)
        fc = _frame_calls(e, np.asarray(fs), foff)
        for x in (e, t):
            x.step_submit(m)
        cases = [
            ("raftq_step_async", lambda: e.sweep(SWEEP_COMMIT)),
            ("raftq_tick", lambda: e.tick()),
            ("raftq_tick_collect_lists", lambda: e.tick_collect_lists()),
            ("raftq_apply_deltas", lambda: e.apply_deltas(g2, np.array([0, 0], np.uint32), s.match[me, 7:9])),
            ("raftq_apply_vote_deltas", lambda: e.apply_vote_deltas(g2, np.array([0, 0], np.uint32), np.array([1, 2], np.uint8))),
            ("raftq_cycle", lambda: e.cycle(SWEEP_COMMIT, e.pack_deltas(g2, np.array([0, 0], np.uint32), s.match[me, 7:9]))),
            ("raftq_apply_log_deltas", lambda: e.apply_log_deltas(g2, s.last_index[7:9], s.last_term[7:9])),
            ("raftq_read_match", lambda: e.read_match()),
            ("raftq_load_roles", lambda: e.load_roles(s.role, s.elapsed)),
            ("raftq_step_set_voters", lambda: e.set_step_voters(not masked)),
            ("raftq_tick_set_voters", lambda: e.set_tick_voters(not masked)),
            ("raftq_bcast_set_voters", lambda: e.set_bcast_voters(not masked)),
            ("raftq_propose_frames", lambda: e._chk(a.call(e)[0])),
            ("raftq_step_frames_respond", lambda: _call(e, fs, foff, 8 * n, None)),
            ("raftq_tick_frames", lambda: e.tick_frames(out, off, po, 64)),
            ("raftq_tick_elect_frames", lambda: e.tick_elect_frames(camp, out2, off2, po2, 64, 64)),
            ("raftq_step_frames", fc["step_frames"]),
            ("raftq_step_frames_packed", fc["step_frames_packed"]),
            ("raftq_step_batch", lambda: e.step_batch(m)),
            ("raftq_step_set_msg_flags", lambda: e._chk(e._lib.raftq_step_set_msg_flags(e._h, 0))),
            ("raftq_step_set_compact", lambda: e.set_compact(1)),
            ("raftq_tick_collect", lambda: e.tick_collect()),
            ("raftq_collect_changed", lambda: e.collect_changed()),
            ("raftq_campaign", lambda: e.campaign(g2, me)),
            ("raftq_apply_term_deltas", lambda: e.apply_term_deltas(g2, s.term[7:9], s.first_idx[7:9])),
            ("raftq_apply_voter_deltas", lambda: e.apply_voter_deltas(e.pack_voter_deltas(g2, [3, 3]))),
            ("raftq_stage", lambda: e.stage(2, 0)),
            ("raftq_stage_packed", lambda: e.stage_packed(2, 0)),
            ("raftq_load_match", lambda: e.load_match(s.match, s.committed)),
            ("raftq_load_votes", lambda: e.load_votes(s.votes)),
            ("raftq_load_terms", lambda: e.load_terms(s.term, s.first_idx)),
            ("raftq_load_node", lambda: e.load_node(s.term, s.vote, s.lead, s.last_index, s.last_term)),
            ("raftq_load_voters", lambda: e.load_voters(V.full_masks(N, G))),
            ("raftq_read_node", lambda: e.read_node()),
            ("raftq_read_votes", lambda: e.read_votes()),
            ("raftq_read_committed", lambda: e.read_committed()),
            ("raftq_read_outcome", lambda: e.read_outcome()),
            ("raftq_read_tick", lambda: e.read_tick()),
            ("raftq_read_voters", lambda: e.read_voters()),
            ("raftq_narrow", lambda: e.narrow()),
            ("raftq_narrow_rebuild", lambda: e.narrow_rebuild()),
            ("raftq_self_max", lambda: e.self_max()),
        ]
        for what, call in cases:
            with pytest.raises(RaftqError) as ei:
                call()
            assert ei.value.code == ESTATE and str(ei.value).split(":", 1)[-1].strip(), (what, str(ei.value))
            assert (out == CANARY).all() and (out2 == CANARY).all(), what
        want = R.step(m)
        got = e.step_collect()[0]
        assert got.tobytes() == want.tobytes() and t.step_collect()[0].tobytes() == got.tobytes()
        same_snapshot(snapshot(e), snapshot(t), "behind the calls refused in flight")
        probe(e, t, R, np.arange(100, 500), 24700, what="behind the calls refused in flight")
