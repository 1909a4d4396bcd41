"""Shared parts of tests/test_refusals_gpu.py: the start state, the full snapshot of a handle, the reference that moves with the
calls, and the probe sequence that runs on a handle behind a refusal and on a twin that never saw one.

The state comes from synth.make_groups (so that the self-max word and the narrow word are both set when it is loaded), with the
row maximum moved to the handle's own slot and roles dealt by group number: g % 4 in (0, 1) led here, 2 a follower, 3 a
candidate.  Every input of every call in here is in range unless a test breaks it on purpose."""
import functools

import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from raftsql_amd import step as S
from raftsql_amd import synth
from raftsql_amd._lib import SWEEP_CHANGED, SWEEP_COMMIT, SWEEP_GATED
from tests import _stepgen, _wiregen
from tests import ref_bcast_members as B
from tests import ref_step_voters as V
from tests import ref_tick_members as T
from tests import ref_voters as RV

ET, HB, SEED = 10, 1, 0x5EED
NREC = 513                          # two workgroups of 256 and a lone lane
POSITIONS = (0, 63, 64, 255, 256, 512)  # first lane, a wave's last and the next one's first, a workgroup's last and the next one's first, the lone lane
SHAPES = [(3, 1), (5, 0), (9, 8)]   # self-row skip body and 16-bit vote words; narrow body; 32-bit vote words and the last slot
CANARY = 0xA5
CANARY64 = np.uint64(0xA5A5A5A5A5A5A5A5)


@functools.lru_cache(maxsize=None)
def base_state(G, N, me, seed):
    """computed once per shape and never changed: callers take V.copy_state() of it"""
    st = synth.make_groups(G, N, seed=seed, with_terms=True)
    rng = np.random.default_rng(seed)
    s = pyoracle.NodeState(G, N, me)
    m, v = st.match.copy(), st.votes.copy()
    m[[0, me]] = m[[me, 0]]  # (make_groups puts the row maximum into slot 0)
    v[[0, me]] = v[[me, 0]]
    s.match[:], s.votes[:], s.committed[:] = m, v, st.committed
    s.term[:] = np.maximum(st.cur_term, 1)
    s.last_index[:] = m[me]
    s.last_term[:] = s.term
    s.first_idx[:] = st.first_idx_cur_term
    kind = np.arange(G) % 4
    s.role[:] = np.where(kind <= 1, S.ROLE_LEADER, np.where(kind == 2, S.ROLE_FOLLOWER, S.ROLE_CANDIDATE))
    lead, cand = s.role == S.ROLE_LEADER, s.role == S.ROLE_CANDIDATE
    s.vote[:] = np.where(lead | cand, me + 1, 0)
    s.lead[:] = np.where(lead, me + 1, 0)
    s.votes[me, cand] = 1
    s.elapsed[:] = np.where(lead, 0, rng.integers(0, ET, G))
    return s


@functools.lru_cache(maxsize=None)
def base_masks(G, N, me, seed):
    """ref_bcast_members.masks() in which self and one other slot vote in every led group -> (voters, the state with the led
    groups' commit index settled over those voters: an append then moves no commit index)"""
    s = V.copy_state(base_state(G, N, me, seed))
    rng = np.random.default_rng(seed + 1)
    led = np.flatnonzero(s.role == S.ROLE_LEADER)
    voters = B.propose_masks(rng, N, G, me, led)
    want, _ = RV.commit_advance(s.match, s.committed, voters, gated=True, first_idx=s.first_idx)
    s.committed[led] = want[led]
    return voters, s


def engine(s, voters=None, switches=True):
    from raftsql_amd.wire import WireEngine

    e = WireEngine(s.G, s.N, s.self_peer)
    e.set_timers(ET, HB, SEED)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        if switches:
            e.set_step_voters(True)
            e.set_tick_voters(True)
            e.set_bcast_voters(True)
    return e


def snapshot(e):
    """everything of a handle that can be read back, as bytes"""
    d = dict(e.read_node())
    d["match"], d["votes"], d["voters"] = e.read_match(), e.read_votes(), e.read_voters()
    d["tick_action"], d["tick_elapsed"], d["tick_role"] = e.read_tick()
    d["read_committed"] = e.read_committed()
    d["narrow"], d["self_max"] = np.array([int(e.narrow())]), np.array([e.self_max()])
    return {k: np.ascontiguousarray(a).tobytes() for k, a in d.items()}


def same_snapshot(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


class Ref:
    """the reference side of a handle: an oracle NodeState, the masks (None: none loaded) and the tick number"""

    def __init__(self, s, voters=None):
        self.s, self.voters, self.tick_no = V.copy_state(s), voters, 0

    @property
    def masks(self):
        return V.full_masks(self.s.N, self.s.G) if self.voters is None else self.voters

    def step(self, m):
        return self.s.step_batch(m) if self.voters is None else V.step_batch(self.s, self.voters, m)

    def tick(self):
        s = self.s
        if self.voters is None:
            el, act, nh, nb = pyoracle.tick(s.role, s.elapsed, ET, HB, SEED, self.tick_no)
        else:
            el, act, nh, nb = T.tick_array(pyoracle, s.role, s.elapsed, self.voters, s.self_peer, ET, HB, SEED, self.tick_no)
        s.elapsed[:] = el
        self.tick_no += 1
        return el, act, nh, nb

    def sweep_gated(self):
        s = self.s
        if self.voters is None:
            want, n = pyoracle.commit_advance(s.match, s.committed, True, s.first_idx)
        else:
            want, n = RV.commit_advance(s.match, s.committed, self.voters, gated=True, first_idx=s.first_idx)
        old = s.committed.copy()
        s.committed[:] = want
        return old, want, n


def same_outputs(got, want, what):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            g, w = np.ascontiguousarray(g).tobytes(), np.ascontiguousarray(w).tobytes()
        assert g == w, f"{what}: {k}"


def other_peers(N, me):
    return [p for p in range(N) if p != me]


def walk_batch(s, groups, rng):
    """a Step batch for the list walk: two messages for each of `groups` by what the group is now -- acknowledgements of the tail
    for a led group, vote responses for a candidate, heartbeats that carry the tail as the commit index for a follower"""
    g = np.asarray(groups, np.int64)
    N, me = s.N, s.self_peer
    typ = np.where(s.role[g] == S.ROLE_LEADER, S.MSG_APP_RESP, np.where(s.role[g] == S.ROLE_CANDIDATE, S.MSG_VOTE_RESP, S.MSG_HEARTBEAT))
    parts = []
    for k in range(2):
        frm = np.array(other_peers(N, me))[(g + k) % (N - 1)]
        m = S.pack_msgs(g.astype(np.uint64), typ, term=s.term[g], frm=frm, index=s.last_index[g], commit=s.last_index[g],
                        reject=(rng.random(len(g)) < 0.2) & (typ == S.MSG_VOTE_RESP))
        parts.append(m)
    return np.concatenate(parts)


def propose_batch(s, voters, groups, rng, n_host):
    """one entry per group of `groups` (led here, sound over `voters`) behind n_host queued messages -> (props, prop_ents, pool, hm, he)"""
    from raftsql_amd.wire import PROP_DT, PROP_ENT_DT

    n = len(groups)
    props, pe = np.zeros(n, PROP_DT), np.zeros(n, PROP_ENT_DT)
    props["group"], props["n_ents"], props["ent_first"] = groups, 1, np.arange(n)
    pe["data_len"] = rng.integers(0, 90, n)
    hm, he, hpool = _wiregen.random_msgs(rng, n_host, big_every=0, ent_frac=0.2) if n_host else (np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT), b"")
    hpool = np.frombuffer(bytes(hpool), np.uint8)
    pe["data_off"] = len(hpool) + np.cumsum(pe["data_len"]) - pe["data_len"]
    pool = np.concatenate([hpool, rng.integers(0, 256, int(pe["data_len"].sum()) + 1, dtype=np.uint8)])
    assert (s.role[np.asarray(groups, np.int64)] == S.ROLE_LEADER).all()
    if voters is not None:
        assert not B.propose_verdict(s, voters, props).any(), "the proposals are meant to be sound"
    return props, pe, pool, hm, he


def propose_want(R, props, pe, pool, hm, he):
    """R moves (appendEntry) -> (stream, frame_off, frames that have bytes, entry headers)"""
    from tests.test_wire_gpu import _propose_expect

    s = R.s
    if R.voters is None:  # the oracle's encoder over _propose_expect's messages
        d = dict(term=s.term, last=s.last_index, last_term=s.last_term, committed=s.committed)
        want_m, want_e, _, _ = _propose_expect(d, s.N, s.self_peer, props, pe, hm, he)
        want, want_off = W.wire_encode(want_m, want_e, pool)
        B.propose_expect(s, R.masks, props, pe, hm, he)
        return np.asarray(want), np.asarray(want_off, np.uint64), len(want_m), len(want_e)
    msgs, keep, ents = B.propose_expect(s, R.voters, props, pe, hm, he)
    want, want_off = B.encode_positional(msgs, keep, ents, pool)
    return np.asarray(want), np.asarray(want_off, np.uint64), int(keep.sum()), len(ents)


class ProposeArgs:
    """page-locked arrays of one raftq_propose_frames call; `out` and `off` carry canaries behind `cap` / the offsets"""

    def __init__(self, props, pe, pool, hm, he, n_peers, room):
        from raftsql_amd.engine import pinned_copy, pinned_empty

        self.props, self.pe, self.pool, self.hm, self.he = (pinned_copy(np.ascontiguousarray(a)) if len(a) else a for a in (props, pe, pool, hm, he))
        self.n_slots = len(hm) + len(props) * (n_peers - 1)
        self.out = pinned_empty(room + 64, np.uint8)
        self.off = pinned_empty(self.n_slots + 1 + 8, np.uint64)
        self.room = room

    def call(self, e, cap=None):
        """-> (rc, counts); `out` is unspecified after a refusal, so are the n_slots + 1 offsets: canaries everywhere else"""
        import ctypes as C

        from raftsql_amd import _lib

        cap = self.room if cap is None else cap
        self.cap = cap
        self.out[:] = CANARY
        self.off[:] = CANARY64
        c = _lib.WireCounts()
        p = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
        rc = e._lib.raftq_propose_frames(e._h, p(self.props), len(self.props), p(self.pe), len(self.pe), p(self.hm), len(self.hm), p(self.he), len(self.he),
                                         p(self.pool), len(self.pool), self.out.ctypes.data, cap, self.off.ctypes.data, C.byref(c))
        assert (self.out[cap:] == CANARY).all(), "bytes at or behind out[cap] were written"
        assert (self.off[self.n_slots + 1:] == CANARY64).all(), "words behind frame_off's end were written"
        return rc, c

    def whole(self, e):
        rc, c = self.call(e)
        e._chk(rc)
        n = int(c.bytes)
        return dict(stream=self.out[:n].copy(), off=self.off[: self.n_slots + 1].copy(), n_msgs=int(c.n_msgs), n_ents=int(c.n_ents), bytes=n)


def propose_outputs(want):
    stream, off, frames, n_e = want
    return dict(stream=stream, off=off, n_msgs=frames, n_ents=n_e, bytes=len(stream))


def probe(e, t, R, touched, seed, again=None, again_want=None, what=""):
    """The next calls are whole: the same sequence on the handle `e` (which saw a refusal) and on its twin `t` (which did not),
    `e` held to the references through R, `t` held to `e`.  again(x) -> dict of outputs, again_want(R) -> the same dict from the
    references (R moves): the refused batch with its bad record taken out, through the same call."""
    from tests.test_respond_gpu import _call

    s, N, me, G = R.s, R.s.N, R.s.self_peer, R.s.G
    rng = np.random.default_rng(seed)
    touched = np.unique(np.asarray(touched, np.int64))
    touched = touched[touched < G]
    assert len(touched) >= 64
    # 1. the refused batch without its bad record
    if again is not None:
        want = again_want(R)
        got = again(e)
        same_outputs(got, want, f"{what}: the batch without its bad record")
        same_outputs(again(t), got, f"{what}: the twin's batch")
    # 2. a list-walk Step batch over the refusal's groups: a list word left marked would be walked into
    m = walk_batch(s, touched[:300], rng)
    want_o = R.step(m)
    got_o, _ = e.step_batch(m)
    assert got_o.tobytes() == want_o.tobytes(), f"{what}: Step results behind the refusal"
    assert t.step_batch(m)[0].tobytes() == got_o.tobytes(), f"{what}: the twin's Step results"
    # 3. one Tick with its lists: the tick number has not moved
    el, act, rh, rb = R.tick()
    for x in (e, t):
        hups, nh, beats, nb = x.tick_collect_lists()
        assert (nh, nb) == (rh, rb), f"{what}: tick counts"
        assert np.array_equal(hups, np.flatnonzero(act == 1).astype(np.uint32)) and np.array_equal(beats, np.flatnonzero(act == 2).astype(np.uint32)), f"{what}: tick lists"
        got_act, got_el, got_role = x.read_tick()
        assert np.array_equal(got_act, act) and np.array_equal(got_el, el) and np.array_equal(got_role, s.role), f"{what}: tick arrays"
    # 4. vote deltas on the refusal's slots: a claim left behind would swallow them
    vg = touched[:300].astype(np.uint64)
    vp = np.array(other_peers(N, me), np.uint32)[(vg.astype(np.int64) + 1) % (N - 1)]
    vv = (1 + (vg & np.uint64(1))).astype(np.uint8)
    s.votes[:] = pyoracle.apply_vote_deltas(s.votes, vg, vp, vv)
    for x in (e, t):
        x.apply_vote_deltas(vg, vp, vv)
        assert np.array_equal(x.read_votes(), s.votes), f"{what}: votes behind the vote deltas"
    # 5. an adopted gated sweep with its changed list: the commit buffer that is current, the mirror
    old, want_c, n_changed = R.sweep_gated()
    moved = np.flatnonzero(want_c != old)
    for x in (e, t):
        c = x.sweep(SWEEP_COMMIT | SWEEP_GATED | SWEEP_CHANGED)
        assert np.array_equal(x.read_committed(), want_c), f"{what}: commit indices behind the sweep"
        adv, n_adv = x.collect_changed()
        assert c.n_changed == n_changed == n_adv == len(moved), f"{what}: the sweep's counts"
        assert np.array_equal(adv["group"], moved.astype(np.uint64)) and np.array_equal(adv["old_commit"], old[moved]) and np.array_equal(adv["new_commit"], want_c[moved]), what
    # 6. one valid raftq_propose_frames and one raftq_step_frames_respond
    led = touched[s.role[touched] == S.ROLE_LEADER]
    led = led[B.propose_verdict(s, R.masks, _props_of(led)) == 0][:40]
    assert len(led) >= 8, f"{what}: the probe found no led group to propose in"
    props, pe, pool, hm, he = propose_batch(s, R.masks, led, rng, 30)
    a = ProposeArgs(props, pe, pool, hm, he, N, len(pool) + 128 * (len(hm) + len(props) * (N - 1)) + 4096)
    want = propose_outputs(propose_want(R, props, pe, pool, hm, he))
    got = a.whole(e)
    same_outputs(got, want, f"{what}: proposals behind the refusal")
    same_outputs(a.whole(t), got, f"{what}: the twin's proposals")
    from tests.test_wire_gpu import _node_frames

    fs, foff = _node_frames(rng, 150, s, me)
    at = B.leaders_bitmap(rng, s, 1.0)
    want_m, we, want_o, want_w, want_po, want_ans, _ = B.respond_want(s, R.masks, fs, foff, at)
    want_s = W.wire_encode(want_w)[0] if len(want_w) else np.zeros(0, np.uint8)
    got = None
    for x in (e, t):
        gm, ge, go, got_s, got_off, got_po, cnt, rc = _call(x, fs, foff, len(we), at)
        mine = (gm.tobytes(), ge.tobytes(), go.tobytes(), bytes(got_s), np.asarray(got_off).tobytes(), np.asarray(got_po).tobytes(), int(rc.n_msgs), int(rc.bytes))
        if got is None:
            got = mine
            assert gm.tobytes() == want_m.tobytes() and ge.tobytes() == we.tobytes(), f"{what}: records behind the refusal"
            assert np.array_equal((go["flags"] & B.ANSWERED) != 0, want_ans), f"{what}: answered flags"
            plain = go.copy()
            plain["flags"] &= np.uint8(~B.ANSWERED & 0xFF)
            assert plain.tobytes() == want_o.tobytes(), f"{what}: results of the respond call"
            assert np.array_equal(got_po, want_po) and rc.n_msgs == len(want_w) and bytes(got_s) == bytes(want_s), f"{what}: responses"
        else:
            assert mine == got, f"{what}: the twin's respond call"
    # and both handles stand where the references stand
    _stepgen.assert_same_state(e, s)
    same_snapshot(snapshot(e), snapshot(t), f"{what}: handle against its twin behind the probe")


def _props_of(groups):
    from raftsql_amd.wire import PROP_DT

    p = np.zeros(len(groups), PROP_DT)
    p["group"], p["n_ents"] = groups, 1
    return p
