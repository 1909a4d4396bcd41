"""The reference of raftq_step_frames_respond with raftq_respond_set_lead on (include/raftq_wire.h "becomeLeader's broadcast"):
tests/test_respond_gpu.py::expected / tests/ref_bcast_members.py::expected with ONE more kind, restated from the header, run over
the oracle's Step results and marshalled by oracle/pywire.  Nothing in here runs the code under test.

The new rule: a RAFTQ_OUT_BECAME_LEADER inside its group's device-answered prefix is answered with one frame per peer (per member,
with masks) -- MsgApp{Index: lastIndex - 1, LogTerm: lastTerm BEFORE becomeLeader, Commit, Entries: [the empty entry (Term,
lastIndex)]} -- does not end the prefix, and puts the group at the tail whatever the caller's bitmap said."""
import numpy as np

from oracle import pywire as W
from tests import ref_step_voters as V

ANSWERED = 0x10
MSG_PROP, MSG_APP, MSG_APP_RESP, MSG_VOTE, MSG_VOTE_RESP, MSG_HB, MSG_HB_RESP = 2, 3, 4, 5, 6, 8, 9


def expected(rec, outs, last_term0, at_tail, N, me, voters=None):
    """-> (wire records, peer-major; their entry headers; peer_off; answered mask; the positions of the wins that were answered)
    voters: None (every slot is a member) or the masks raftq_bcast_set_voters sends the broadcasts over"""
    from raftsql_amd import step as S

    n = len(rec)
    per_peer = [[] for _ in range(N)]
    ents = []  # (term, index) of the empty entries, one per answered win
    answered = np.zeros(n, bool)
    wins = []
    st = {}  # group -> [at-tail, host owns the rest, lastTerm]
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
        last_term_was = s[2]
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
            elif t == S.OUT_BECAME_LEADER:  # THE new rule (idx is the empty entry's index)
                kind, to = MSG_APP, None
                fields = {"index": idx - 1, "log_term": last_term_was, "commit": int(o["commit"]), "ent_first": len(ents), "n_ents": 1}
                ents.append((int(o["term"]), idx))
                wins.append(i)
                s[0] = True
            elif t != S.OUT_NONE:
                s[1] = True
        if not kind:
            continue
        answered[i] = True
        for p in range(N):
            if p == me or (to is not None and p != to):
                continue
            if to is None and voters is not None and not (int(voters[g]) >> p) & 1:
                continue
            per_peer[p].append(dict(group=g, term=int(o["term"]), type=kind, to=p, **fields))
    recs = [r for p in range(N) for r in per_peer[p]]
    w = np.zeros(len(recs), W.WIRE_MSG_DT)
    for k, r in enumerate(recs):
        for f, v in r.items():
            w[k][f] = v
    w["from"] = me
    e = np.zeros(len(ents), W.WIRE_ENT_DT)
    for k, (term, index) in enumerate(ents):
        e[k]["term"], e[k]["index"] = term, index
    peer_off = np.zeros(N + 1, np.uint64)
    peer_off[1:] = np.cumsum([len(per_peer[p]) for p in range(N)])
    return w, e, peer_off, answered, wins


def encode(w, e):
    """the stream and the frame offsets the call must write"""
    if not len(w):
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    s, off = W.wire_encode(w, e, np.zeros(1, np.uint8))
    return np.asarray(s), np.asarray(off, np.uint64)


def want(st, s, off, at_tail, voters=None, tail_appends=True):
    """st MOVES.  -> dict(m, ents, outs, stream, off, peer_off, answered, wins, n_frames)"""
    from tests.test_wire_gpu import _node_filter

    wm, we, _ = W.wire_decode(s, off)
    want_m, rec = _node_filter(wm, we, st.G, st.N, st.self_peer, tail_appends)
    last_term0 = st.last_term.copy()
    outs = st.step_batch(rec) if voters is None else V.step_batch(st, voters, rec)
    w, e, po, ans, wins = expected(rec, outs, last_term0, at_tail, st.N, st.self_peer, voters)
    stream, woff = encode(w, e)
    return dict(m=want_m, ents=we, outs=outs, stream=stream, off=woff, peer_off=po, answered=ans, wins=wins, n_frames=len(w), sent=w)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def frames(rows, me):
    """hand-made payload-free frames addressed to `me` -> (stream, frame_off)"""
    m = np.zeros(len(rows), W.WIRE_MSG_DT)
    for k, r in enumerate(rows):
        for f, v in r.items():
            m[k][f] = v
    m["to"] = me
    s, off = W.wire_encode(m)
    return np.asarray(s).copy(), np.asarray(off, np.uint64)


def candidate_state(G, N, me, term=7, last=10, last_term=2, committed=8):
    """every group a candidate of `term` that has its own vote and nobody else's, its log ending at (last, last_term)"""
    from oracle import pyoracle

    st = pyoracle.NodeState(G, N, me)
    st.term[:], st.last_index[:], st.last_term[:], st.committed[:] = term, last, last_term, committed
    st.role[:] = 1
    st.vote[:] = me + 1
    st.votes[me] = 1
    st.match[me] = last
    return st


def one_grant_short(rng, G, N, me, voters=None):
    """tests/_stepgen.random_state in which every candidate lacks exactly ONE grant of its quorum (the quorum of its voters, with
    masks; a candidate that is no voter of its group, or whose quorum is itself, is made a follower) -> (NodeState, the
    candidates, for each a peer that has not answered yet and whose grant counts)"""
    from tests import _stepgen

    st = _stepgen.random_state(rng, G, N, self_peer=me)
    cands, granters = [], []
    for g in np.flatnonzero(st.role == 1):
        vm = (1 << N) - 1 if voters is None else int(voters[g])
        others = [p for p in range(N) if p != me and (vm >> p) & 1]
        q = bin(vm).count("1") // 2 + 1
        if not (vm >> me) & 1 or q < 2 or len(others) < q - 1:
            st.role[g], st.votes[:, g] = 0, 0
            continue
        order = rng.permutation(others)
        st.votes[:, g] = 0
        st.votes[me, g] = 1
        st.votes[order[: q - 2], g] = 1
        # the peers that do not count may have answered anything
        for p in range(N):
            if p != me and not (vm >> p) & 1:
                st.votes[p, g] = rng.integers(0, 3)
        cands.append(g)
        granters.append(order[q - 2])
    return st, np.array(cands, np.int64), np.array(granters, np.int64)


def shuffled(rng, parts):
    """the frames of several (stream, frame_off) in one random order -> (stream, frame_off)"""
    pieces = []
    for s, off in parts:
        s = np.asarray(s)
        pieces += [s[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
    pieces = [pieces[k] for k in rng.permutation(len(pieces))]
    off = np.zeros(len(pieces) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    return np.concatenate(pieces).astype(np.uint8), off


def random_call(rng, st, cands, granters, n_noise, n_grants, n_acks):
    """one batch: _node_frames' traffic, the missing grant of n_grants candidates, and for n_acks of those an acknowledgement of
    the empty entry from the granter -- which commits it when it comes behind the win"""
    from tests.test_wire_gpu import _node_frames

    still = st.role[cands] == 1
    pick = np.flatnonzero(still)[:n_grants]
    g, p = cands[pick], granters[pick]
    grants = frames([dict(group=int(a), type=MSG_VOTE_RESP, term=int(st.term[a]), **{"from": int(b)}) for a, b in zip(g, p)], st.self_peer)
    acks = frames([dict(group=int(a), type=MSG_APP_RESP, term=int(st.term[a]), index=int(st.last_index[a]) + 1, **{"from": int(b)})
                   for a, b in zip(g[:n_acks], p[:n_acks])], st.self_peer)
    return shuffled(rng, [_node_frames(rng, n_noise, st, st.self_peer), grants, acks])
