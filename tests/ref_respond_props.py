"""The reference of raftq_step_frames_respond with raftq_respond_set_props on (include/raftq_wire.h "A forwarded proposal's
MsgApps"): tests/ref_respond_lead.py::expected with ONE more rule, restated from the header, run over the reference's Step results
(tests/ref_step_props.py: Step with the MsgProp arms, held to the C oracle on the CPU) and marshalled by oracle/pywire with the
inbound stream as the pool.  Nothing in here runs the code under test.

The new rule: a RAFTQ_OUT_PROPOSED inside its group's device-answered prefix whose group is at the tail at that message -- by the
caller's bitmap or by a device-answered becomeLeader earlier in the batch -- is answered with one frame per peer (per member, with
masks): MsgApp{Term, Index / LogTerm: the tail BEFORE the proposal, Commit: committed AFTER the message, Entries: the frame's own,
entry k stamped {Term, old lastIndex + 1 + k}, Type and Data as received}.  The bit stays, the prefix does not end.  A proposal
with the bit clear -- or whose entry headers lie beyond ents_cap, which the decoder did not hand back -- is the host's: it ends
the prefix and the bit stays clear.  RAFTQ_OUT_FORWARD is the host's in every case."""
import numpy as np

from oracle import pywire as W
from tests import ref_respond_lead as L
from tests import ref_step_props as P

ANSWERED = L.ANSWERED
MSG_PROP, MSG_APP, MSG_APP_RESP, MSG_VOTE_RESP, MSG_HB, MSG_HB_RESP = 2, 3, 4, 6, 8, 9
ENT_MAX = 40  # RAFTQ_RESPOND_ENT_MAX


def expected(rec, wm, we, outs, last_term0, at_tail, N, me, voters=None, lead=True, props=True, ents_cap=None):
    """rec: the records Step read; wm / we: the decoder's records and entry headers (ent_first / n_ents, Type / Data of a proposal's
    entries); outs: the reference's full results.  lead / props: the two switches.  -> (wire records, peer-major; their entry headers
    (data_off into the inbound stream); peer_off; answered mask; positions of the answered wins; positions of the answered proposals)"""
    from raftsql_amd import step as S

    n = len(rec)
    per_peer = [[] for _ in range(N)]
    ents = []  # (term, index, data_off, data_len, type)
    answered = np.zeros(n, bool)
    wins, taken = [], []
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
        if t in (S.OUT_BECAME_LEADER, S.OUT_PROPOSED):  # becomeLeader's empty entry, appendEntry's: Term
            s[2] = int(o["term"])
        if int(o["role"]) != S.ROLE_LEADER:
            s[0] = False
        mt, rej, idx = int(m["type"]), int(m["reject"]), int(o["index"])
        if t == S.OUT_PROGRESS:
            if mt == MSG_APP_RESP and rej and int(m["index"]) > idx:
                s[0] = False
            elif mt == MSG_HB_RESP and idx < int(o["last_index"]):
                s[0] = False
        first, cnt = int(wm[i]["ent_first"]), int(wm[i]["n_ents"])
        prop_here = (t == S.OUT_PROPOSED and props and s[0] and not s[1] and (ents_cap is None or first + cnt <= ents_cap))
        if t == S.OUT_PROPOSED and not prop_here:
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
            elif t == S.OUT_BECAME_LEADER and lead:
                kind, to = MSG_APP, None
                fields = {"index": idx - 1, "log_term": last_term_was, "commit": int(o["commit"]), "ent_first": len(ents), "n_ents": 1}
                ents.append((int(o["term"]), idx, 0, 0, 0))
                wins.append(i)
                s[0] = True
            elif prop_here:  # THE new rule (idx is the first new entry's index)
                kind, to = MSG_APP, None
                fields = {"index": idx - 1, "log_term": last_term_was, "commit": int(o["commit"]), "ent_first": len(ents), "n_ents": cnt}
                for k in range(cnt):
                    h = we[first + k]
                    ents.append((int(o["term"]), idx + k, int(h["data_off"]), int(h["data_len"]), int(h["type"])))
                taken.append(i)
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
    for k, row in enumerate(ents):
        e[k]["term"], e[k]["index"], e[k]["data_off"], e[k]["data_len"], e[k]["type"] = row
    peer_off = np.zeros(N + 1, np.uint64)
    peer_off[1:] = np.cumsum([len(per_peer[p]) for p in range(N)])
    return w, e, peer_off, answered, wins, taken


def encode(w, e, pool):
    """the stream and the frame offsets the call must write; pool: the inbound stream"""
    if not len(w):
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    s, off = W.wire_encode(w, e, np.ascontiguousarray(pool, np.uint8) if len(pool) else np.zeros(1, np.uint8))
    return np.asarray(s), np.asarray(off, np.uint64)


def want(st, s, off, at_tail, voters=None, tail_appends=True, lead=True, props=True, ents_cap=None, step=P.step_batch):
    """st MOVES.  step: the Step reference, called as step(st, voters, records) (a module that composes more arms passes its own).
    -> dict(m, ents, outs, stream, off, peer_off, answered, wins, taken, n_frames, sent, sent_ents, rec)"""
    wm, we, _ = W.wire_decode(s, off)
    want_m, rec = P.node_filter(wm, we, st.G, st.N, st.self_peer, tail_appends, True)
    last_term0 = st.last_term.copy()
    outs = step(st, voters, rec)
    w, e, po, ans, wins, taken = expected(rec, want_m, we, outs, last_term0, at_tail, st.N, st.self_peer, voters, lead, props, ents_cap)
    stream, woff = encode(w, e, s)
    return dict(m=want_m, ents=we, outs=outs, stream=stream, off=woff, peer_off=po, answered=ans, wins=wins, taken=taken, n_frames=len(w),
                sent=w, sent_ents=e, rec=rec)


def cap_bound(n, N, nbytes, ents_cap, lead):
    """the header's bound on `out`, restated"""
    return n * (N - 1) * (109 if lead else 83) + (N - 1) * (nbytes + ents_cap * ENT_MAX)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def frames(rows, me, pad=0):
    """hand-made frames addressed to `me` -> (stream, frame_off).  A row is a dict of raftq_wire_msg_t fields; `ents`: a list of
    (type, payload bytes) -- the entries' Term and Index are junk (appendEntry overwrites them).  pad: bytes of pool in front of the
    first payload (the encoder copies payloads, so this only moves where they come from)"""
    m = np.zeros(len(rows), W.WIRE_MSG_DT)
    ents, pool = [], bytearray(b"\xee" * pad)
    for k, r in enumerate(rows):
        r = dict(r)
        es = r.pop("ents", [])
        for f, v in r.items():
            m[k][f] = v
        m[k]["ent_first"], m[k]["n_ents"] = len(ents), len(es)
        for j, (typ, data) in enumerate(es):
            ents.append((0x1111 + j, 0x2222 + 3 * j, len(pool), len(data), typ))
            pool += data
    m["to"] = me
    e = np.zeros(len(ents), W.WIRE_ENT_DT)
    for k, row in enumerate(ents):
        e[k]["term"], e[k]["index"], e[k]["data_off"], e[k]["data_len"], e[k]["type"] = row
    s, off = W.wire_encode(m, e, np.frombuffer(bytes(pool) + b"\0", np.uint8))
    return np.asarray(s).copy(), np.asarray(off, np.uint64)


def prop(g, frm, ents, term=0):
    return dict(group=g, type=MSG_PROP, term=term, ents=ents, **{"from": frm})


def ack(g, frm, term, index):
    return dict(group=g, type=MSG_APP_RESP, term=term, index=index, **{"from": frm})


def leader_state(G, N, me, term=5, last=10, last_term=3, committed=8, match=8):
    """every group led by `me` at `term`, its log ending at (last, last_term) -- LogTerm is neither Term nor Term - 1 -- committed
    up to `committed`, every follower's Match at `match`, the current-term gate open from `committed` on"""
    from oracle import pyoracle

    st = pyoracle.NodeState(G, N, me)
    st.term[:], st.last_index[:], st.last_term[:], st.committed[:] = term, last, last_term, committed
    st.role[:] = 2
    st.vote[:] = st.lead[:] = me + 1
    st.match[:] = match
    st.match[me] = last
    st.first_idx[:] = max(committed, 1)
    return st


def bitmap(G, groups):
    b = np.zeros((G + 63) // 64, np.uint64)
    for g in np.asarray(groups, np.int64):
        b[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
    return b


def random_case(seed, N, me, G=97, n_frames=600, band=None, masked=False, hot=False):
    """ref_step_props' state and traffic as frames, with what this rule needs planted in front: in led groups a proposal of three
    entries (the second with no Data) followed by an acknowledgement of the last new index from every other slot (it commits), and a
    second proposal behind that; the bitmap has 70 % of the led groups, the planted ones among them -- and PLANT of the planted
    without the bit.  -> (start state, voters | None, stream, frame_off, at_tail)"""
    from tests import _widegen as WG
    from tests import ref_step_voters as V

    rng = np.random.default_rng(seed)
    s = P.props_state(rng, N, me, G)
    if band is not None:
        s = WG.lift(s, band, rng)
    voters = None
    if masked:
        voters = rng.integers(0, 1 << N, G).astype(np.uint16) | np.uint16(1 << me)
        led = np.flatnonzero(s.role == 2)
        voters[led[-4:-2]] = 1 << me  # one-voter groups: commit on the append, zero frames
    m = P.props_batch(rng, s, n_frames, hot=int(rng.integers(0, G)) if hot else None)
    stream, off = P.frames_of(rng, m, me, empty_props=0.1)
    led = np.flatnonzero(s.role == 2)
    plant = led[: 2 * P.PLANT]
    rows = []
    others = [p for p in range(N) if p != me]
    for g in plant:
        t, li = int(s.term[g]), int(s.last_index[g])
        rows.append(prop(int(g), others[0], [(0, b"abc"), (1, b""), (0, bytes(range(17)))]))
        rows += [ack(int(g), p, t, li + 3) for p in others]
        rows.append(prop(int(g), others[-1], [(0, b"z" * 130)]))
    ps, poff = frames(rows, me, pad=5)
    # the planted frames go in front, in order (a group's frames keep their order); the rest behind them
    stream2 = np.concatenate([ps, np.asarray(stream, np.uint8)])
    off2 = np.concatenate([poff[:-1], np.asarray(off, np.uint64) + np.uint64(len(ps))])
    bits = set(int(g) for g in led[rng.random(len(led)) < 0.7]) | set(int(g) for g in plant[: P.PLANT])
    bits -= set(int(g) for g in plant[P.PLANT:])
    return V.copy_state(s), voters, stream2, off2, bitmap(G, sorted(bits))


def shows(w, rec):
    """what a case must contain for the tests to tell the feature from its absence -> dict of counts"""
    from raftsql_amd import step as S

    o, ans = w["outs"], w["answered"]
    propd = o["type"] == S.OUT_PROPOSED
    taken = np.zeros(len(o), bool)
    taken[w["taken"]] = True
    grp = rec["group"]
    two, ack_behind = 0, 0
    for g in np.unique(grp[taken]):
        idx = np.flatnonzero((grp == g) & (o["type"] != S.OUT_SKIPPED))
        tk = [i for i in idx if taken[i]]
        two += len(tk) >= 2
        ack_behind += any(ans[i] and rec["type"][i] == MSG_APP_RESP and (int(o["flags"][i]) & S.OUTF_COMMITTED) and i > tk[0] for i in idx)
    return {"answered proposals": int(taken.sum()), "unanswered proposals": int((propd & ~taken).sum()),
            "forwards": int((o["type"] == S.OUT_FORWARD).sum()),
            "frames with more than one entry": int((w["m"]["n_ents"][taken] > 1).sum()),
            "zero-length payloads": int((w["sent_ents"]["data_len"] == 0).sum() - len(w["wins"])),
            "a committing ack behind a proposal": int(ack_behind), "two proposals of one group": int(two)}


FLOORS = {"answered proposals": 8, "unanswered proposals": 4, "forwards": 1, "frames with more than one entry": 4, "zero-length payloads": 4,
          "a committing ack behind a proposal": 2, "two proposals of one group": 2}


def case_list():
    """the arguments of every random_case the GPU tests run (tests/test_respond_props_ref.py asserts FLOORS for each)"""
    from tests import _widegen as WG

    cases = [dict(seed=9500 + 16 * N + me, N=N, me=me, n_frames=300) for N in range(2, 10) for me in range(N)]
    cases += [dict(seed=9800 + k, N=5, me=2, n_frames=1500) for k in range(2)]
    cases += [dict(seed=9810, N=5, me=1, n_frames=800, masked=True), dict(seed=9811, N=3, me=0, n_frames=600, hot=True)]
    cases += [dict(seed=9820 + k, N=3, me=1, n_frames=400, band=b) for k, b in enumerate(WG.BAND_NAMES)]
    return cases
