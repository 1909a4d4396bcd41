"""Generators for the Step family at 64-bit terms and indices (tests/test_widegen.py, tests/test_step_wide_gpu.py).

tests/_stepgen.py and tests/test_wire_gpu.py draw terms below 9 and indices below 1,000, and do their "value +- delta" through
int64, which wraps from 2^63 up.  Here a state of theirs is LIFTED into one of three bands and the traffic around it is drawn in
uint64 alone, saturating at 0 and at 2^64 - 1:

  b32   every group's tail within +-6 of 2^32, its term within +-3: a 32-bit temporary or mirror loses the carry
  b63   the same around 2^63: a signed compare orders the two sides the wrong way round
  top   [2^64 - 2^12, 2^64 - 2^11): bit 63 set in every operand, every varint ten bytes long

A 0 that means "none" (an empty log's tail, a Match nobody reported, first_idx / committed 0) stays 0, so a group may hold 0 and
2^32 + k side by side.  No helper returns a value, or implies an index + n_ents, at or above 2^64 - 2^10 (LIMIT): the exact top
and wrap-around belong to the Tick suites.  TEST INFRASTRUCTURE: nothing in the product imports it."""
import functools

import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from tests import _stepgen
from tests import ref_step_voters as V

U = np.uint64
MAX = U(2**64 - 1)
LIMIT = 2**64 - 2**10
BANDS = {"b32": 2**32, "b63": 2**63, "top": None}  # the boundary B; "top" is a range instead
TOP_LO, TOP_HI = 2**64 - 2**12, 2**64 - 2**11
BAND_NAMES = tuple(BANDS)
PROP_MAX_ENTS = 1024  # kPropMaxEnts: the most entries raftq_propose_frames takes in one record


# ---- uint64 arithmetic ---------------------------------------------------------------------------------------------------------
def _u(x):
    return np.asarray(x).astype(U)


def sat_add(v, k):
    v, k = _u(v), _u(k)
    return np.where(v > MAX - k, MAX, v + k)


def sat_sub(v, k):
    v, k = _u(v), _u(k)
    return np.where(v < k, U(0), v - k)


def around(rng, v, lo, hi, n):
    """v + a uniform draw from [lo, hi) (lo <= 0 < hi), saturating: up by [0, hi - lo), then down by -lo"""
    return sat_sub(sat_add(v, rng.integers(0, hi - lo, n, dtype=U)), U(-lo))


def pick(rng, v, deltas, n):
    """v + a uniform pick from `deltas` (small, some negative), saturating"""
    lo = min(deltas)
    return sat_sub(sat_add(v, rng.choice(np.array([d - lo for d in deltas], U), n)), U(-lo))


def guard(*arrays):
    for a in arrays:
        a = np.asarray(a)
        assert a.dtype == U and (a.size == 0 or int(a.max()) < LIMIT), "a value at or above 2^64 - 2^10"


def _draw(rng, band, n, radius):
    """n targets: uniform in [B - radius, B + radius], or in the top band"""
    if band == "top":
        return U(TOP_LO) + rng.integers(0, TOP_HI - TOP_LO, n, dtype=U)
    return U(BANDS[band] - radius) + rng.integers(0, 2 * radius + 1, n, dtype=U)


# ---- the state ---------------------------------------------------------------------------------------------------------------------
def _invariants(s):
    assert (s.committed <= s.last_index).all() and (s.match[s.self_peer] == s.last_index).all() and (s.last_term <= s.term).all()


def shift(s, tbase, ibase):
    """a copy of s with every non-zero term moved by tbase[g] and every non-zero index by ibase[g]"""
    n = V.copy_state(s)
    tb, ib = np.broadcast_to(_u(tbase), (s.G,)), np.broadcast_to(_u(ibase), (s.G,))
    for k in ("term", "last_term"):
        getattr(n, k)[:] = np.where(getattr(s, k) != 0, getattr(s, k) + tb, U(0))
    for k in ("last_index", "committed", "first_idx"):
        getattr(n, k)[:] = np.where(getattr(s, k) != 0, getattr(s, k) + ib, U(0))
    n.match[:] = np.where(s.match != 0, s.match + ib[None, :], U(0))
    return n


def lift(state, band, rng):
    """-> a new NodeState: group g's indices moved so that last_index[g] lands uniformly in [B - 6, B + 6] (in the band, for
    "top"), its terms so that term[g] lands in [B - 3, B + 3]; a 0 stays 0"""
    _invariants(state)
    assert int(state.last_index.max()) < 2**11 and int(state.term.max()) < 2**11, "lift takes a small state"
    tbase = _draw(rng, band, state.G, 3) - state.term
    ibase = _draw(rng, band, state.G, 6) - state.last_index
    n = shift(state, tbase, ibase)
    _invariants(n)
    guard(n.term, n.last_term, n.last_index, n.committed, n.first_idx, n.match)
    return n


def below_boundary(band, v):
    """which of v lie below the band's boundary (b32, b63)"""
    return np.asarray(v) < U(BANDS[band])


# ---- Step's records --------------------------------------------------------------------------------------------------------------
def wide_batch(rng, s, n, hot_groups=None):
    """tests/_stepgen.random_batch, draw for draw, in saturating uint64"""
    G, N = s.G, s.N
    g = rng.integers(0, G, n) if hot_groups is None else rng.choice(hot_groups, n)
    t = rng.choice(_stepgen.TYPES, n, p=_stepgen.TYPE_P)
    m = np.zeros(n, dtype=pyoracle.STEP_MSG_DT)
    m["group"], m["type"] = g, t
    local = (t == 0) | (t == 1)
    term = np.maximum(U(1), pick(rng, s.term[g], [-1, 0, 0, 0, 0, 1, 2], n))
    m["term"] = np.where(local, U(0), term)
    m["from"] = rng.integers(0, N, n)
    li = s.last_index[g]
    m["index"] = around(rng, li, -3, 4, n)
    m["log_term"] = around(rng, s.last_term[g], -1, 2, n)
    m["commit"] = around(rng, li, -4, 3, n)
    m["reject"] = rng.random(n) < 0.3
    m["reject_hint"] = m["index"]
    says = (t == 3) & (rng.random(n) < 0.5)
    tail = says & (rng.random(n) < 0.5)
    m["index"] = np.where(tail, li, m["index"])
    m["log_term"] = np.where(tail, s.last_term[g], m["log_term"])
    bars = (t == 3) & (rng.random(n) < 0.35)
    m["_pad"][:, 1] = np.where(says, 0x80, 0) | np.where(bars, 0x40, 0)
    k = rng.integers(0, 4, n, dtype=U)
    m["_resv"] = np.where(says, k | (rng.integers(0, 2**31, n, dtype=U) << U(32)), U(0))  # high half: ignored
    last_ent = np.maximum(m["log_term"], sat_sub(m["term"], (rng.random(n) < 0.5).astype(U)))
    m["reject_hint"] = np.where(says, last_ent, m["reject_hint"])
    guard(m["term"], m["index"], m["log_term"], m["commit"], m["reject_hint"], m["index"] + np.where(says, k, U(0)))
    return m


# ---- frames in -------------------------------------------------------------------------------------------------------------------
def wide_node_frames(rng, n, st, self_peer):
    """tests/test_wire_gpu._node_frames, draw for draw, in saturating uint64 -> (stream, frame_off)"""
    G, N = st.G, st.N
    m = np.zeros(n, W.WIRE_MSG_DT)
    g = rng.integers(0, G, n)
    m["group"] = g
    m["type"] = rng.choice([2, 3, 4, 5, 6, 8, 9], n, p=[0.08, 0.30, 0.30, 0.06, 0.06, 0.10, 0.10])
    m["term"] = np.maximum(U(1), pick(rng, st.term[g], [-1, 0, 0, 0, 0, 1], n))
    m["from"] = (self_peer + 1 + rng.integers(0, N - 1, n)) % N
    m["to"] = self_peer
    li = st.last_index[g]
    m["index"] = around(rng, li, -2, 3, n)
    m["log_term"] = around(rng, st.last_term[g], -1, 2, n)
    m["commit"] = around(rng, li, -3, 3, n)
    m["reject"] = rng.random(n) < 0.2
    m["reject_hint"] = m["index"]
    tail = (m["type"] == 3) & (rng.random(n) < 0.6)
    m["index"] = np.where(tail, li, m["index"])
    m["log_term"] = np.where(tail, st.last_term[g], m["log_term"])
    carries = ((m["type"] == 3) & (rng.random(n) < 0.8)) | (m["type"] == 2)
    k = np.where(carries, rng.choice([1, 1, 2, 3, 6], n), 0)  # (6: more than a decoder lane keeps)
    m["n_ents"] = k
    m["ent_first"] = np.concatenate([[0], np.cumsum(k)[:-1]])
    ne = int(k.sum())
    e = np.zeros(ne, W.WIRE_ENT_DT)
    owner = np.repeat(np.arange(n), k)
    e["term"] = np.maximum(m["log_term"][owner], sat_sub(m["term"][owner], (rng.random(ne) < 0.5).astype(U)))
    e["index"] = m["index"][owner] + U(1) + (np.arange(ne) - m["ent_first"][owner]).astype(U)
    e["data_len"] = rng.integers(0, 40, ne)
    e["data_off"] = np.concatenate([[0], np.cumsum(e["data_len"])[:-1]]) if ne else 0
    pool = rng.integers(0, 256, int(e["data_len"].sum()) + 1, dtype=np.uint8)
    guard(m["term"], m["index"], m["log_term"], m["commit"], m["reject_hint"], m["index"] + _u(k), e["term"], e["index"])
    # what a node has to shrug off
    odd = rng.random(n)
    m["to"] = np.where(odd < 0.03, (self_peer + 1) % N, m["to"])
    m["from"] = np.where((odd >= 0.03) & (odd < 0.05), N + 3, m["from"])
    m["group"] = np.where((odd >= 0.05) & (odd < 0.07), G + rng.integers(0, 1000, n), m["group"])
    m["type"] = np.where((odd >= 0.07) & (odd < 0.10), rng.choice([0, 1, 7, 10, 11, 200], n), m["type"])
    s, off = W.wire_encode(m, e, pool)
    s = s.copy()
    for i in np.nonzero((odd >= 0.10) & (odd < 0.12))[0]:  # garbage where the message's first key was
        s[int(off[i]) + 8] = 0x0B
    return s, off


def wide_lead_call(rng, st, cands, granters, n_noise, n_grants, n_acks):
    """tests/ref_respond_lead.random_call over wide_node_frames: the traffic, the missing grant of n_grants candidates, and for
    n_acks of those the granter's acknowledgement of the empty entry"""
    from tests import ref_respond_lead as L

    pick_ = np.flatnonzero(st.role[cands] == 1)[:n_grants]
    g, p = cands[pick_], granters[pick_]
    guard(st.last_index[g] + U(1))
    grants = L.frames([dict(group=int(a), type=L.MSG_VOTE_RESP, term=int(st.term[a]), **{"from": int(b)}) for a, b in zip(g, p)], st.self_peer)
    acks = L.frames([dict(group=int(a), type=L.MSG_APP_RESP, term=int(st.term[a]), index=int(st.last_index[a]) + 1, **{"from": int(b)})
                     for a, b in zip(g[:n_acks], p[:n_acks])], st.self_peer)
    return L.shuffled(rng, [wide_node_frames(rng, n_noise, st, st.self_peer), grants, acks])


# ---- proposals -------------------------------------------------------------------------------------------------------------------
def wide_propose_setup(rng, band, G, N, me, n_props, n_host_msgs, max_per_group=3):
    """tests/test_wire_gpu._propose_setup with every tail within 3 below B (anywhere in the band, for "top"), so that a record's
    entries cross B inside one MsgApp, term and last_term around B, and record 0 carrying PROP_MAX_ENTS entries
    -> (state dict, props, prop_ents, pool, host msgs, host ents)"""
    from raftsql_amd.wire import PROP_DT, PROP_ENT_DT
    from tests import _wiregen

    term = _draw(rng, band, G, 3)
    if band == "top":
        last = _draw(rng, band, G, 0)
    else:
        last = U(BANDS[band] - 3) + rng.integers(0, 3, G, dtype=U)
    last_term = np.minimum(term, _draw(rng, band, G, 3))
    committed = sat_sub(last, rng.integers(0, 1000, G, dtype=U))
    role = np.full(G, 2, np.uint8)
    groups = rng.choice(G, n_props, replace=False).astype(U)
    cnt = rng.integers(1, max_per_group + 1, n_props).astype(np.uint32)
    cnt[0] = PROP_MAX_ENTS
    props = np.zeros(n_props, PROP_DT)
    props["group"], props["n_ents"] = groups, cnt
    props["ent_first"] = np.cumsum(cnt) - cnt
    ne = int(cnt.sum())
    pe = np.zeros(ne, PROP_ENT_DT)
    pe["data_len"] = rng.integers(0, 200, ne)
    pe["data_len"][rng.random(ne) < 0.1] = 0  # (an empty statement: Entry.Data omitted)
    if n_host_msgs:
        hm, he, hpool = _wiregen.random_msgs(rng, n_host_msgs, big_every=0, ent_frac=0.2)
        for a, ks in ((hm, ("term", "log_term", "index", "commit", "reject_hint")), (he, ("term", "index"))):
            for k in ks:  # (the host's own messages pass through as they are: any width, short of the guard)
                a[k] = np.minimum(a[k], U(LIMIT - 1))
    else:
        hm, he, hpool = np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT), b""
    hpool = np.frombuffer(bytes(hpool), np.uint8) if not isinstance(hpool, np.ndarray) else hpool
    pe["data_off"] = len(hpool) + np.cumsum(pe["data_len"]) - pe["data_len"]
    pool = np.concatenate([hpool, rng.integers(0, 256, int(pe["data_len"].sum()), dtype=np.uint8)])
    new_last = last.copy()
    new_last[groups.astype(np.int64)] += cnt.astype(U)
    guard(term, last, last_term, committed, new_last)
    st = dict(term=term, last=last, last_term=last_term, committed=committed, role=role)
    return st, props, pe, pool, hm, he


# ---- the hand tables of tests/_stepgen.py, lifted ----------------------------------------------------------------------------------
def table_bases(band):
    """(term base, index base): the tables' term 5 lands on B, their tail index 10 on B, commit 7 at B - 3 (for "top": on the
    band's lower edge instead)"""
    b = TOP_LO if band == "top" else BANDS[band]
    return U(b - 5), U(b - 10)


def _nz(v, base):
    v = _u(v)
    return np.where(v != 0, v + base, U(0))


def lift_msgs(m, tb, ib):
    """a copy of hand-made Step records: term / log_term / reject_hint (the tables keep the last entry's term there) by tb, index /
    commit by ib, zeros left alone"""
    m = m.copy()
    for k in ("term", "log_term", "reject_hint"):
        m[k] = _nz(m[k], tb)
    for k in ("index", "commit"):
        m[k] = _nz(m[k], ib)
    guard(m["term"], m["log_term"], m["reject_hint"], m["index"], m["commit"], m["index"] + (m["_resv"] & U(0xFFFFFFFF)))
    return m


def lifted_tail_append_table(band):
    tb, ib = table_bases(band)
    s, m, want = _stepgen.tail_append_table()
    lw = [(typ, int(_nz(idx, ib)), int(_nz(c, ib)), int(_nz(last, ib)), int(_nz(lt, tb)), role) for typ, idx, c, last, lt, role in want]
    return shift(s, tb, ib), lift_msgs(m, tb, ib), lw


def lifted_barrier_table(band):
    tb, ib = table_bases(band)
    s, m, want, after = _stepgen.barrier_table()
    la = {"committed": [int(_nz(v, ib)) for v in after["committed"]], "last_index": [int(_nz(v, ib)) for v in after["last_index"]],
          "last_term": [int(_nz(v, tb)) for v in after["last_term"]]}
    return shift(s, tb, ib), lift_msgs(m, tb, ib), want, la


def lifted_hold_skip_table(band):
    tb, ib = table_bases(band)
    s, m, want, after = _stepgen.hold_skip_table()
    return shift(s, tb, ib), lift_msgs(m, tb, ib), want, {"committed": [int(_nz(v, ib)) for v in after["committed"]]}


def alias_table(band):
    """By hand: values exactly 2^32 apart are different values (an equality taken on the low words says otherwise).  T, L = the
    tables' term 5 and tail index 10 in the band; `far(v)` is v + 2^32, or v - 2^32 where that would pass the guard ("top").
    Groups 0 and 1 follow at term T, tail (L, T - 1), commit L - 3; group 2 is led at T, tail (L, T), commit L - 2, the followers'
    Match L - 2 and L - 4.  -> (NodeState, msgs, want types (None: not held), state after)"""
    tb, ib = table_bases(band)
    T, L = int(tb) + 5, int(ib) + 10
    up = band != "top"
    far = (lambda v: v + 2**32) if up else (lambda v: v - 2**32)
    s = pyoracle.NodeState(3, 3, 1)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:] = T, L, T - 1, L - 3
    s.match[1] = L
    s.role[2], s.last_term[2], s.committed[2], s.first_idx[2], s.vote[2], s.lead[2] = 2, T, L - 2, L - 5, 2, 2
    s.match[0, 2], s.match[2, 2] = L - 2, L - 4
    rows = [
        # group, type, flags, from, index, log_term, commit, n_ents, last_ent_term -> out type
        (0, 3, 0x80, 0, far(L), T - 1, L, 1, T, 7),       # not the tail: a gap (or far below it) -- the owner's (OUT_APPEND)
        (1, 3, 0x80, 0, L, far(T - 1), L, 1, T, 7),       # the tail's index, another term: the owner's
        (2, 4, 0x00, 0, far(L - 2), 0, 0, 0, 0, None),    # an ack 2^32 from the Match on record: beyond the log (clamped to L, which
    ]                                                     # commits L) or long stale (nothing moves) -- never "the same again"
    m = np.zeros(len(rows), dtype=pyoracle.STEP_MSG_DT)
    for i, r in enumerate(rows):
        m["group"][i], m["type"][i], m["_pad"][i][1], m["from"][i] = r[0], r[1], r[2], r[3]
        m["index"][i], m["log_term"][i], m["commit"][i], m["_resv"][i], m["reject_hint"][i] = r[4], r[5], r[6], r[7], r[8]
    m["term"] = T
    guard(m["term"], m["index"], m["log_term"], m["commit"], m["reject_hint"], m["index"] + m["_resv"])
    after = {"last_index": [L, L, L], "last_term": [T - 1, T - 1, T], "committed": [L - 3, L - 3, L if up else L - 2]}
    return s, m, [r[9] for r in rows], after, [L if up else L - 2, L, L - 4]  # (the led group's Match row after)


def check_state_after(s, after):
    for k, v in after.items():
        assert [int(x) for x in getattr(s, k)] == v, k


# ---- the run tests/test_step_wide_gpu.py::test_step_wide and the pipelined forms make: computed once, never changed ------------------
STEP_SHAPES = ((3, 0), (5, 4), (9, 8))  # N = 9: the 32-bit vote words
STEP_G, STEP_N_MSGS, STEP_BATCHES, STEP_HOT = 3000, 9000, 10, 30


def step_seed(band, N, me, hold_skip):
    return 20000 + 1000 * BAND_NAMES.index(band) + 10 * N + me + 500 * bool(hold_skip)


@functools.lru_cache(maxsize=None)
def step_run(band, N, me, hold_skip=False, G=STEP_G):
    """-> (start NodeState, [per batch: (msgs, the oracle's records, (last_index, committed) before it, the state before it)],
    the state after).  Every third batch goes to STEP_HOT groups: runs of ~100 messages, hence the stall replay; with hold_skip
    every other batch carries RAFTQ_MSGF_HOLD / RAFTQ_MSGF_SKIP."""
    rng = np.random.default_rng(step_seed(band, N, me, hold_skip))
    s = lift(_stepgen.random_state(rng, G, N, me), band, rng)
    start = V.copy_state(s)
    batches = []
    for it in range(STEP_BATCHES):
        hot = rng.choice(G, STEP_HOT, replace=False) if it % 3 == 2 else None
        m = wide_batch(rng, s, STEP_N_MSGS, hot_groups=hot)
        if hold_skip and it % 2:
            m = _stepgen.with_hold_skip(rng, m)
        pre = V.copy_state(s)
        want = s.step_batch(m)
        batches.append((m, want, (pre.last_index, pre.committed), pre))
    guard(s.term, s.last_term, s.last_index, s.committed, s.first_idx, s.match)
    return start, batches, s


# ---- what the switch suites' band cases share (tests/ref_check_quorum.py, ref_pre_vote.py, ref_lead_transfer.py, ref_read_index.py) -------
MSG_U64 = ("term", "index", "log_term", "commit", "reject_hint")
STATE_U64 = ("term", "last_term", "last_index", "committed", "first_idx")
OWN_KINDS = tuple(range(12, 19))  # MsgCheckQuorum .. MsgPreVoteResp: the kinds only the *_cq_* kernels take
DECIDED = ("type", "reject", "flags", "role")


def band_edge(band):
    """the band's boundary B, or -- "top" -- its lower edge"""
    return TOP_LO if band == "top" else BANDS[band]


def band_floor(band):
    """what the largest term and index of a run in the band cannot lie below: lift() draws within 3 / 6 of B"""
    return (TOP_LO, TOP_LO) if band == "top" else (BANDS[band] - 3, BANDS[band] - 6)


def far(band, v):
    """v + 2^32, or v - 2^32 where that would pass the guard ("top"): alias_table's"""
    return v - 2**32 if band == "top" else v + 2**32


def set_term(s, groups, term):
    """groups' term := term, their last entry's term kept at or below it (a leader's: the term itself)"""
    s.term[groups] = term
    s.last_term[groups] = np.where(s.role[groups] == 2, s.term[groups], np.minimum(s.last_term[groups], s.term[groups]))


def guard_case(s, m):
    guard(*(getattr(s, k) for k in STATE_U64), s.match, *(m[k] for k in MSG_U64))


def low32(s, m):
    """-> copies of a state and a batch with every 64-bit word reduced mod 2^32: what a walk that kept 32 bits of them would read"""
    lo = U(0xFFFFFFFF)
    n = V.copy_state(s)
    for k in STATE_U64:
        getattr(n, k)[:] = getattr(s, k) & lo
    n.match[:] = s.match & lo
    m = np.array(m)
    for k in MSG_U64:
        m[k] = m[k] & lo
    return n, m


def decided_otherwise(a, b):
    """-> bool[n]: the records of two runs that differ in (type, reject, flags, role)"""
    return np.logical_or.reduce([a[k] != b[k] for k in DECIDED])


def straddles(s, m, boundary=2**63):
    """-> bool[n], from the inputs alone: m.term and the group's term, or m.index and the group's tail, on opposite sides of the
    boundary.  A 0 is "none" on either side; a heartbeat's index is a context, not a position."""
    g = m["group"].astype(np.int64)
    b = U(boundary)
    t = (m["term"] != 0) & (s.term[g] != 0) & ((m["term"] < b) != (s.term[g] < b))
    pos = ~np.isin(m["type"], (8, 9))
    i = pos & (m["index"] != 0) & (s.last_index[g] != 0) & ((m["index"] < b) != (s.last_index[g] < b))
    return t | i


def check_narrow_reading(m, want, want32, own_kinds, what=""):
    """a b32 case: the reference over the same start and batch reduced mod 2^32 (want32) decides at least one record in ten
    otherwise, eight of them of the switch's own kinds -> (share, own)"""
    d = decided_otherwise(want, want32)
    share, own = float(d.mean()), int((d & np.isin(m["type"], own_kinds)).sum())
    assert share >= 0.10 and own >= 8, (what, share, own)
    return share, own


def check_straddles(s, m, own_kinds, plant, what=""):
    """a b63 case, from the inputs alone: one record in twenty compares across 2^63, `plant` of them of the switch's own kinds"""
    st = straddles(s, m)
    share, own = float(st.mean()), int((st & np.isin(m["type"], own_kinds)).sum())
    assert share >= 0.05 and own >= plant, (what, share, own)
    return share, own


def check_in_band(band, want, what=""):
    """the case is where it says: the largest term and index of its results are at or above the band's lower edge"""
    t, i = band_floor(band)
    assert int(want["term"].max()) >= t and int(max(want["index"].max(), want["last_index"].max())) >= i, what
