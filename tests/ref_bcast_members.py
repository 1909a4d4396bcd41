"""The reference of the two device-built broadcasts over each group's own members (raftq_bcast_set_voters, include/raftq_wire.h):
raftq_step_frames_respond's commit broadcast and raftq_propose_frames' bcastAppend, both ranging over r.prs.

Two restatements, built from what the suite already trusts:
  * the respond table of tests/test_respond_gpu.py::expected with ONE line changed -- a broadcast goes to slot p only if
    voters[g] >> p & 1 -- run over tests/ref_step_voters.step_batch's results;
  * tests/test_wire_gpu.py::_propose_expect made positional -- every slot's record, and which of them are sent -- together with
    the verdict of the two new refusals: 7, this node is no member of its group; 8, the append would move the commit index, read
    off ref_step_voters.VRaft.maybe_commit after Match[self] was raised to lastIndex + n_ents.
TEST INFRASTRUCTURE: nothing in the product imports it."""
import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from tests import ref_raft_py as R
from tests import ref_step_voters as V

ANSWERED = 0x10
MSG_APP, MSG_APP_RESP, MSG_VOTE_RESP, MSG_HB_RESP = 3, 4, 6, 9
PROP_NO_MEMBER, PROP_COMMITS = 7, 8
WHY = {PROP_NO_MEMBER: "no member of its group", PROP_COMMITS: "would move the commit index"}


# ---- raftq_step_frames_respond ---------------------------------------------------------------------------------------------
def expected(rec, outs, last_term0, at_tail, N, me, voters):
    """tests/test_respond_gpu.py::expected over members.  -> (wire records, peer-major; peer_off; answered mask; the recipients
    of every commit broadcast, in result order, as a list of tuples)"""
    from raftsql_amd import step as S

    n = len(rec)
    per_peer = [[] for _ in range(N)]
    answered = np.zeros(n, bool)
    bcasts = []
    st = {}  # group -> [at-tail bit, host owns the rest, lastTerm]
    for i in range(n):
        o, m = outs[i], rec[i]
        t = int(o["type"])
        if t == S.OUT_SKIPPED:
            continue
        g = int(m["group"])
        if g not in st:
            bit = at_tail is not None and (int(at_tail[g >> 6]) >> (g & 63)) & 1
            st[g] = [bool(bit), False, int(last_term0[g])]
        s = st[g]
        if t == S.OUT_APPENDED and int(m["_resv"]) & 0xFFFFFFFF:
            s[2] = int(m["reject_hint"])
        if t == S.OUT_BECAME_LEADER:
            s[2] = int(o["term"])
        if int(o["role"]) != S.ROLE_LEADER:
            s[0] = False
        mt, rej, idx = int(m["type"]), int(m["reject"]), int(o["index"])
        if t == S.OUT_PROGRESS:
            if mt == MSG_APP_RESP and rej and int(m["index"]) > idx:
                s[0] = False
            elif mt == MSG_HB_RESP and idx < int(o["last_index"]):
                s[0] = False
        kind, to, fields = 0, int(m["from"]), {}
        if not s[1]:
            if t == S.OUT_APPENDED:
                kind, fields = MSG_APP_RESP, {"index": idx}
            elif t == S.OUT_VOTE_RESP:
                kind, fields = MSG_VOTE_RESP, {"reject": int(o["reject"])}
            elif t == S.OUT_HEARTBEAT_RESP:
                kind = MSG_HB_RESP
            elif t == S.OUT_PROGRESS:
                if mt == MSG_APP_RESP and not rej:
                    if not s[0]:
                        s[1] = True
                    elif int(o["flags"]) & S.OUTF_COMMITTED:
                        kind, to = MSG_APP, None
                        fields = {"index": int(o["last_index"]), "log_term": s[2], "commit": int(o["commit"])}
                elif (int(m["index"]) > idx) if mt == MSG_APP_RESP else (idx < int(o["last_index"])):
                    s[1] = True
            elif t != S.OUT_NONE:
                s[1] = True
        if not kind:
            continue
        answered[i] = True
        sent = []
        for p in range(N):
            if p == me or (to is not None and p != to):
                continue
            if to is None and not (int(voters[g]) >> p) & 1:  # THE line: bcastAppend ranges over r.prs
                continue
            per_peer[p].append(dict(group=g, term=int(o["term"]), type=kind, to=p, **fields))
            sent.append(p)
        if to is None:
            bcasts.append(tuple(sent))
    recs = [r for p in range(N) for r in per_peer[p]]
    w = np.zeros(len(recs), W.WIRE_MSG_DT)
    for k, r in enumerate(recs):
        for f, v in r.items():
            w[k][f] = v
    w["from"] = me
    peer_off = np.zeros(N + 1, np.uint64)
    peer_off[1:] = np.cumsum([len(per_peer[p]) for p in range(N)])
    return w, peer_off, answered, bcasts


def bcast_counts(bcasts, N):
    """-> (broadcasts that lost a recipient, that kept all N - 1, that have none)"""
    return (sum(1 for b in bcasts if len(b) < N - 1), sum(1 for b in bcasts if len(b) == N - 1), sum(1 for b in bcasts if not b))


def masks(rng, n, g, empty=3, single=3):
    """uniform in [1, 2^N), a few groups forced empty and a few forced to one voter"""
    v = V.random_masks(rng, n, g)
    at = rng.permutation(g)[: min(g, empty + single)]
    v[at[:empty]] = 0
    v[at[empty:]] = (1 << rng.integers(0, n, len(at[empty:]))).astype(np.uint16)
    return v


def bitmap(G, groups):
    b = np.zeros((G + 63) // 64, np.uint64)
    for g in np.asarray(groups, np.int64):
        b[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
    return b


def leaders_bitmap(rng, st, frac=0.7):
    lead = np.nonzero(st.role == 2)[0]
    return bitmap(st.G, lead[rng.random(len(lead)) < frac])


def _respond_start(rng, G, N, me):
    """tests/test_respond_gpu.py's start state plus masks().  Deviation, so that every kind of broadcast occurs at every N: among
    the led groups {self} alone is planted in up to 60 (their commit broadcast has no recipient) and the full mask in up to 150
    (rare among uniform masks once N is large).  -> (NodeState, voters, the planted groups)"""
    from tests import _stepgen

    st = _stepgen.random_state(rng, G, N, self_peer=me)
    voters = masks(rng, N, G)
    led = np.flatnonzero(st.role == 2)
    led = led[rng.permutation(len(led))]
    n_alone, n_whole = min(60, len(led) // 4), min(150, len(led) // 2)
    voters[led[:n_alone]] = 1 << me
    voters[led[n_alone:n_alone + n_whole]] = (1 << N) - 1
    return st, voters, led[:n_alone + n_whole]


def _respond_call(rng, st, planted, n):
    """n frames as a node might receive them now, and an at-tail bitmap: 70 per cent of the led groups, every planted one that is
    still led"""
    from tests.test_wire_gpu import _node_frames

    s, off = _node_frames(rng, n, st, st.self_peer)
    at_tail = leaders_bitmap(rng, st)
    at_tail |= bitmap(st.G, planted[st.role[planted] == 2])
    return s, off, at_tail


def respond_input(seed, G, N, me, n):
    """one call -> (NodeState, voters, stream, frame_off, at_tail)"""
    rng = np.random.default_rng(seed)
    st, voters, planted = _respond_start(rng, G, N, me)
    return (st, voters) + _respond_call(rng, st, planted, n)


def respond_run(seed, G, N, me, sizes, tail_appends=(True,)):
    """calls of `sizes` frames in a row, the state moving with them -> (start NodeState, voters, [per call: dict(s, off, at_tail,
    tail_appends, want = respond_want's tuple, after = the state after)])"""
    rng = np.random.default_rng(seed)
    st, voters, planted = _respond_start(rng, G, N, me)
    start = V.copy_state(st)
    calls = []
    for it, n in enumerate(sizes):
        s, off, at_tail = _respond_call(rng, st, planted, n)
        ta = tail_appends[it % len(tail_appends)]
        want = respond_want(st, voters, s, off, at_tail, ta)
        calls.append(dict(s=s, off=off, at_tail=at_tail, tail_appends=ta, want=want, after=V.copy_state(st)))
    return start, voters, calls


def respond_want(st, voters, s, off, at_tail, tail_appends=True):
    """st MOVES.  -> (records as handed back, entry headers, results, wire records, peer_off, answered, bcasts)"""
    from tests.test_wire_gpu import _node_filter

    wm, we, _ = W.wire_decode(s, off)
    want_m, rec = _node_filter(wm, we, st.G, st.N, st.self_peer, tail_appends)
    last_term0 = st.last_term.copy()
    want_o = V.step_batch(st, voters, rec)
    w, po, ans, bc = expected(rec, want_o, last_term0, at_tail, st.N, st.self_peer, voters)
    return want_m, we, want_o, w, po, ans, bc


# ---- raftq_propose_frames --------------------------------------------------------------------------------------------------
def propose_state(d, N, me):
    """tests/test_wire_gpu.py::_propose_setup's state dict as a NodeState, the way _propose_engine loads it: every follower's
    Match is the commit index, self's the tail, first_idx 1, vote = lead = self"""
    G = len(d["term"])
    s = pyoracle.NodeState(G, N, me)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:], s.role[:] = d["term"], d["last"], d["last_term"], d["committed"], d["role"]
    s.vote[:] = s.lead[:] = me + 1
    s.first_idx[:] = 1
    s.match[:] = d["committed"][None, :]
    s.match[me] = d["last"]
    return s


def propose_verdict(s, voters, props):
    """-> int [n_props]: 0 = sound over members, 7 / 8 = the new refusals.  (The six old reasons are not restated: the inputs
    that use this are sound by them.)"""
    out = np.zeros(len(props), np.int64)
    for i, p in enumerate(props):
        g = int(p["group"])
        if not (int(voters[g]) >> s.self_peer) & 1:
            out[i] = PROP_NO_MEMBER
            continue
        r = V.from_node_state(s, g, voters[g])
        r.prs[r.id].maybe_update(r.last_index + int(p["n_ents"]))  # appendEntry: r.prs[r.id].maybeUpdate(lastIndex)
        if r.maybe_commit():
            out[i] = PROP_COMMITS
    return out


def propose_expect(s, voters, props, pe, hm, he):
    """_propose_expect made positional over a NodeState (s MOVES: appendEntry) -> (every slot's record: the host's, then one run
    of n_props per peer; keep [slots] bool: the host's records and the members'; the entry headers)"""
    N, me = s.N, s.self_peer
    n_props = len(props)
    msgs = np.zeros(len(hm) + n_props * (N - 1), W.WIRE_MSG_DT)
    keep = np.ones(len(msgs), bool)
    ents = np.zeros(len(he) + len(pe), W.WIRE_ENT_DT)
    msgs[: len(hm)] = hm
    ents[: len(he)] = he
    for i, p in enumerate(props):
        g, k, f = int(p["group"]), int(p["n_ents"]), int(p["ent_first"])
        for j in range(k):
            e = ents[len(he) + f + j]
            e["term"], e["index"] = s.term[g], s.last_index[g] + 1 + j
            e["data_len"], e["type"] = pe["data_len"][f + j], pe["type"][f + j]
            e["data_off"] = pe["data_off"][f + j] if pe["data_len"][f + j] else 0
            ents[len(he) + f + j] = e
        run = 0
        for to in range(N):
            if to == me:
                continue
            at = len(hm) + run * n_props + i
            m = msgs[at]
            m["group"], m["term"], m["log_term"], m["index"], m["commit"] = g, s.term[g], s.last_term[g], s.last_index[g], s.committed[g]
            m["from"], m["to"], m["type"], m["ent_first"], m["n_ents"] = me, to, MSG_APP, len(he) + f, k
            msgs[at] = m
            keep[at] = bool((int(voters[g]) >> to) & 1)
            run += 1
        s.last_index[g] += k
        s.last_term[g] = s.term[g]
        s.match[me, g] = max(int(s.match[me, g]), int(s.last_index[g]))
    return msgs, keep, ents


def encode_positional(msgs, keep, ents, pool):
    """the kept records alone through the wire oracle, their offsets spread over the positional slots -> (stream, frame_off
    [len(msgs) + 1]: a slot that is not kept has zero length)"""
    keep = np.asarray(keep, bool)
    sent = msgs[keep]
    stream, dense = W.wire_encode(sent, ents, pool) if len(sent) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    at = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return stream, np.asarray(dense, np.uint64)[at]


def propose_masks(rng, n, g, me, groups):
    """masks(), and in `groups` (the proposed ones) self votes and at least one other slot does"""
    v = masks(rng, n, g)
    groups = np.asarray(groups, np.int64)
    v[groups] |= np.uint16(1 << me)
    lone = groups[v[groups] == (1 << me)]
    others = np.array([p for p in range(n) if p != me])
    v[lone] |= (1 << others[rng.integers(0, len(others), len(lone))]).astype(np.uint16)
    return v


def propose_input(seed, G, N, me, n_props, n_host, max_per_group=3):
    """-> (NodeState, voters, props, prop_ents, pool, host msgs, host ents)"""
    from tests.test_wire_gpu import _propose_setup

    rng = np.random.default_rng(seed)
    d, props, pe, pool, hm, he = _propose_setup(rng, G, N, me, n_props, n_host, max_per_group)
    return propose_state(d, N, me), propose_masks(rng, N, G, me, props["group"]), props, pe, pool, hm, he


def shrink_example():
    """N = 5, self 0, Match 10, 8, 5, 5, 5, committed 5, voters {0, 1, 2}: the membership shrank since the last acknowledgement.
    -> (NodeState of 4 groups, all alike; voters)"""
    s = pyoracle.NodeState(4, 5, 0)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:], s.role[:], s.first_idx[:] = 3, 10, 3, 5, 2, 1
    s.vote[:] = s.lead[:] = 1
    for p, m in enumerate((10, 8, 5, 5, 5)):
        s.match[p] = m
    return s, np.full(4, 0b00111, np.uint16)


# the seeds and shapes the GPU tests use (tests/test_bcast_members_gpu.py), checked for discrimination on the CPU
# (tests/test_bcast_members_ref.py)
RESPOND_BIG = (14100, 3000, 5, 2, (1, 255, 257, 9000))  # seed, G, N, me, sizes
RESPOND_LONG = (14300, 40, 3, 1, (6000, 300, 50))       # > 32 frames of one group: the sorted walk and the replay
PROPOSE_SHAPES = [(3, 0, 1, 0), (3, 2, 700, 300), (5, 1, 5000, 0), (7, 6, 2000, 4000), (2, 1, 33, 7), (9, 4, 300, 0)]


def respond_slot_case(N, me):
    return (14200 + 16 * N + me, 1500, N, me, (257, 2000))


def propose_seed(N, n_props):
    return 16000 + n_props + N
