"""The reference of raftq_propose_frames under raftq_propose_set_forward (include/raftq_wire.h "A follower's proposals"): a record
whose group this node leads is appendEntry + bcastAppend as it always was; one whose group it follows is ONE MsgProp frame to the
group's leader (etcd stepFollower: `m.To = r.lead; r.send(m)`, Term 0 because raft.send leaves a MsgProp's alone, the entries as the
client handed them in: Term 0, Index 0); one whose group knows no leader is dropped.  The layout is positional -- (N - 1) runs of
n_props slots behind the caller's own messages -- and a slot that holds no frame has zero length.

Built from oracle/pywire.wire_encode through tests/ref_bcast_members.encode_positional.  tests/test_propose_forward_ref.py holds it
to a literal hand table of frame bytes, to tests/ref_step_props (what Step makes of the same MsgProp) and to the leader rule of
tests/test_wire_gpu.py restated.  TEST INFRASTRUCTURE: nothing in the product imports it."""
import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from tests import _wiregen
from tests import ref_bcast_members as B

APPENDED, FORWARDED, DROPPED = 0, 1, 2  # RAFTQ_PROP_*
MSG_PROP, MSG_APP = 2, 3
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
PROP_DT = np.dtype([("group", "<u8"), ("ent_first", "<u4"), ("n_ents", "<u4")])
PROP_ENT_DT = np.dtype([("data_off", "<u8"), ("data_len", "<u4"), ("type", "<u4")])
U = np.uint64


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def outcome(role, lead, me):
    """what becomes of a record, from the group's role and lead (0 = None, else slot + 1) -> (RAFTQ_PROP_*, the leader's slot | None).
    A follower whose lead is itself is a loaded state upstream cannot reach; CHOICE (the header's): dropped."""
    if role == LEADER:
        return APPENDED, None
    if role == FOLLOWER and lead != 0 and lead - 1 != me:
        return FORWARDED, lead - 1
    return DROPPED, None


def expect(s, voters, props, pe, hm, he):
    """s MOVES (the leaders' appendEntry).  s: anything whose role / lead / term / last_index / last_term / committed index by group
    and whose match indexes by [slot, group] (a pyoracle.NodeState; the hand table uses dicts), with N and self_peer.  voters: the
    masks, or None.  -> dict(msgs: every slot's record, the host's then one run of n_props per peer slot != self; keep [slots]: the
    slots that hold a frame; ents: the entry headers, written for every record; what [n_props]: the outcomes; to [n_props]: the
    leader's slot of a forwarded record, -1 otherwise)"""
    N, me = s.N, s.self_peer
    n_props, n_hm, n_he = len(props), len(hm), len(he)
    msgs = np.zeros(n_hm + n_props * (N - 1), W.WIRE_MSG_DT)
    keep = np.ones(len(msgs), bool)
    ents = np.zeros(n_he + len(pe), W.WIRE_ENT_DT)
    msgs[:n_hm] = hm
    ents[:n_he] = he
    what = np.zeros(n_props, np.uint8)
    to_of = np.full(n_props, -1, np.int64)
    for i, p in enumerate(props):
        g, k, f = int(p["group"]), int(p["n_ents"]), int(p["ent_first"])
        o, leader = outcome(int(s.role[g]), int(s.lead[g]), me)
        what[i] = o
        for j in range(k):
            e = ents[n_he + f + j]
            # appendEntry stamps the leader's entries; a follower sends them as the client handed them in
            e["term"], e["index"] = (s.term[g], s.last_index[g] + 1 + j) if o == APPENDED else (0, 0)
            e["data_len"], e["type"] = pe["data_len"][f + j], pe["type"][f + j]
            e["data_off"] = pe["data_off"][f + j] if pe["data_len"][f + j] else 0
            ents[n_he + f + j] = e
        run = 0
        for to in range(N):
            if to == me:
                continue
            at = n_hm + run * n_props + i
            run += 1
            m = msgs[at]
            m["group"], m["from"], m["to"], m["ent_first"], m["n_ents"] = g, me, to, n_he + f, k
            if o == APPENDED:
                m["type"], m["term"], m["log_term"], m["index"], m["commit"] = MSG_APP, s.term[g], s.last_term[g], s.last_index[g], s.committed[g]
                keep[at] = voters is None or bool((int(voters[g]) >> to) & 1)  # bcastAppend ranges over r.prs
            else:
                m["type"] = MSG_PROP  # Term 0, and every other field: send consults no prs
                keep[at] = o == FORWARDED and to == leader
            msgs[at] = m
        if o == APPENDED:
            s.last_index[g] = int(s.last_index[g]) + k
            s.last_term[g] = s.term[g]
            s.match[me, g] = max(int(s.match[me, g]), int(s.last_index[g]))
        elif o == FORWARDED:
            to_of[i] = leader
    return dict(msgs=msgs, keep=keep, ents=ents, what=what, to=to_of)


def want(s, voters, props, pe, pool, hm, he):
    """s MOVES -> expect()'s dict + stream, off (len(msgs) + 1 offsets, zero-length slots where nothing is kept), n_frames: the
    frames with bytes among the device's slots"""
    w = expect(s, voters, props, pe, hm, he)
    stream, off = B.encode_positional(w["msgs"], w["keep"], w["ents"], pool if len(pool) else np.zeros(1, np.uint8))
    w["stream"], w["off"], w["n_frames"] = np.asarray(stream), np.asarray(off, np.uint64), int(w["keep"][len(hm):].sum())
    return w


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
# what a group is to this node: led; followed, the leader in the k-th other slot; campaigning; a follower that knows no leader; a
# follower whose lead is this node itself (loaded, not reachable)
K_LED, K_CAND, K_LOST, K_SELF, K_FOLLOW = 0, 1, 2, 3, 4  # K_FOLLOW + k: the leader is the k-th slot other than self
MIXES = ("one leader", "spread", "dropped", "mixed", "led")


def deal(rng, G, N, me, mix):
    """-> int [G]: a kind per group.  The kinds are drawn group by group, so the outcomes interleave within every wave of records"""
    if mix == "one leader":
        return np.full(G, K_FOLLOW + int(rng.integers(0, N - 1)))
    if mix == "spread":
        return K_FOLLOW + rng.integers(0, N - 1, G)
    if mix == "dropped":
        return rng.choice([K_CAND, K_LOST, K_SELF], G)
    if mix == "led":
        return np.full(G, K_LED)
    return np.where(rng.random(G) < 0.4, K_LED, np.where(rng.random(G) < 0.6, K_FOLLOW + rng.integers(0, N - 1, G), rng.choice([K_CAND, K_LOST, K_SELF], G)))


def state(rng, G, N, me, kinds):
    """a node's state with the roles dealt by `kinds`: random tails, every follower's Match at the commit index and self's at the
    tail (an append moves no commit index), first_idx 1"""
    s = pyoracle.NodeState(G, N, me)
    s.term[:] = rng.integers(2, 9, G)
    s.last_index[:] = rng.integers(1, 1000, G)
    s.last_term[:] = np.minimum(s.term, rng.integers(1, 9, G).astype(U))
    s.committed[:] = (s.last_index * rng.random(G)).astype(U)
    s.first_idx[:] = 1
    s.match[:] = s.committed[None, :]
    s.match[me] = s.last_index
    others = np.array([p for p in range(N) if p != me])
    follow = kinds >= K_FOLLOW
    s.role[:] = np.where(kinds == K_LED, LEADER, np.where(kinds == K_CAND, CANDIDATE, FOLLOWER))
    s.lead[:] = np.where(kinds == K_LED, me + 1, np.where(kinds == K_SELF, me + 1, 0))
    s.lead[follow] = others[kinds[follow] - K_FOLLOW] + 1
    s.vote[:] = np.where((kinds == K_LED) | (kinds == K_CAND), me + 1, s.lead)
    return s


def records(rng, G, n_props, n_host, max_per_group=3):
    """tests/test_wire_gpu.py::_propose_setup's records restated, with EntryConfChange (type 1) among the entries: n_props groups
    named once each, 1 .. max_per_group entries a record, one payload in ten empty; n_host messages of the caller's own in front,
    their payloads at the front of the same pool -> (props, prop_ents, pool, host msgs, host ents)"""
    groups = rng.choice(G, n_props, replace=False).astype(U)
    cnt = rng.integers(1, max_per_group + 1, n_props).astype(np.uint32)
    props = np.zeros(n_props, PROP_DT)
    props["group"], props["n_ents"] = groups, cnt
    props["ent_first"] = np.cumsum(cnt) - cnt
    ne = int(cnt.sum())
    pe = np.zeros(ne, PROP_ENT_DT)
    pe["data_len"] = rng.integers(1, 200, ne)
    pe["data_len"][rng.random(ne) < 0.1] = 0
    pe["type"][rng.random(ne) < 0.15] = 1
    if n_props >= 2:  # (whatever the draws: both are in every case of more than one record)
        pe["data_len"][0], pe["type"][ne - 1] = 0, 1
    if n_host:
        hm, he, hpool = _wiregen.random_msgs(rng, n_host, big_every=0, ent_frac=0.2)
        hpool = np.frombuffer(bytes(hpool), np.uint8) if not isinstance(hpool, np.ndarray) else hpool.view(np.uint8)
    else:
        hm, he, hpool = np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT), np.zeros(0, np.uint8)
    pe["data_off"] = len(hpool) + np.cumsum(pe["data_len"]) - pe["data_len"]
    pool = np.concatenate([hpool, rng.integers(0, 256, int(pe["data_len"].sum()), dtype=np.uint8)])
    return props, pe, pool, hm, he


def masks(rng, s, props):
    """uniform masks; in a LED group that is proposed in, self votes and at least one other slot does (ref_bcast_members'
    propose_masks: the two member refusals are not what these cases are about).  The groups this node follows keep whatever was
    drawn: a forward asks nobody's membership"""
    led = props["group"][s.role[props["group"].astype(np.int64)] == LEADER]
    return B.propose_masks(rng, s.N, s.G, s.self_peer, led)


def case(N, me, n_props, n_host, mix, seed, masked=False, G=4096):
    """one call: dict(G, N, me, s0: the state before, voters | None, props, pe, pool, hm, he, want: want()'s dict, after: the state
    after)"""
    rng = np.random.default_rng(seed)
    G = max(G, n_props)
    s0 = state(rng, G, N, me, deal(rng, G, N, me, mix))
    props, pe, pool, hm, he = records(rng, G, n_props, n_host)
    voters = masks(rng, s0, props) if masked else None
    after = copy_state(s0)
    w = want(after, voters, props, pe, pool, hm, he)
    return dict(G=G, N=N, me=me, mix=mix, s0=s0, voters=voters, props=props, pe=pe, pool=pool, hm=hm, he=he, want=w, after=after)


def copy_state(s):
    from tests import ref_step_voters as V

    return V.copy_state(s)


MEANT = {"one leader": {FORWARDED}, "spread": {FORWARDED}, "dropped": {DROPPED}, "mixed": {APPENDED, FORWARDED, DROPPED}, "led": {APPENDED}}


def shows(c):
    """what a case shows, read off the reference's own output"""
    w, s0 = c["want"], c["s0"]
    g = c["props"]["group"].astype(np.int64)
    dropped = w["what"] == DROPPED
    return {"outcomes": set(int(x) for x in np.unique(w["what"])), "leaders": len(np.unique(w["to"][w["to"] >= 0])),
            "dropped candidates": int((dropped & (s0.role[g] == CANDIDATE)).sum()), "dropped, no leader": int((dropped & (s0.role[g] == FOLLOWER) & (s0.lead[g] == 0)).sum()),
            "dropped, lead is self": int((dropped & (s0.role[g] == FOLLOWER) & (s0.lead[g] == c["me"] + 1)).sum()),
            "records of more than one entry": int((c["props"]["n_ents"] > 1).sum()), "empty payloads": int((c["pe"]["data_len"] == 0).sum()),
            "type 1": int((c["pe"]["type"] == 1).sum()),
            "member fillers among the leaders' slots": int((~w["keep"][len(c["hm"]):] & np.tile(w["what"] == APPENDED, c["N"] - 1)).sum())}


def assert_shows(c, what=""):
    """a case holds at least one record of each outcome it is meant to show; a case that spreads its forwards has at least two
    different leaders when N >= 3 (and enough records to); one of more than one record has an empty payload and a type-1 entry"""
    got = shows(c)
    assert MEANT[c["mix"]] <= got["outcomes"], (what, got)
    n = len(c["props"])
    if c["mix"] in ("one leader",):
        assert got["leaders"] == 1, (what, got)
    if c["mix"] in ("spread", "mixed") and c["N"] >= 3 and n >= 16:
        assert got["leaders"] >= 2, (what, got)
    if c["mix"] in ("dropped", "mixed") and n >= 255:
        assert min(got["dropped candidates"], got["dropped, no leader"], got["dropped, lead is self"]) >= 1, (what, got)
    if n >= 2:
        assert got["empty payloads"] >= 1 and got["type 1"] >= 1, (what, got)
    if n >= 255:
        assert got["records of more than one entry"] >= 1, (what, got)
    return got


# the cases the GPU suite runs (tests/test_propose_forward_gpu.py), every one checked on the CPU (tests/test_propose_forward_ref.py):
# (N, self, n_props, n_host, mix).  N in {2, 3, 5, 7}; self first, middle and last; n_props around kBlock = 256 (the check grid covers
# max(records, entries): 255 records have more entries than a workgroup has lanes) and ~3000; 0 and 300 queued messages in front
PARITY = [
    (3, 1, 1, 0, "one leader"), (3, 0, 255, 0, "one leader"), (3, 2, 256, 300, "spread"), (3, 1, 257, 0, "mixed"), (3, 1, 3001, 300, "mixed"),
    (2, 0, 257, 300, "one leader"), (2, 1, 256, 0, "mixed"), (2, 1, 255, 0, "dropped"),
    (5, 0, 256, 0, "spread"), (5, 2, 3001, 0, "spread"), (5, 4, 255, 300, "mixed"), (5, 2, 257, 300, "dropped"), (5, 3, 1, 300, "dropped"),
    (7, 0, 257, 0, "mixed"), (7, 3, 255, 300, "spread"), (7, 6, 3001, 300, "mixed"), (7, 6, 256, 0, "dropped"), (7, 3, 256, 300, "one leader"),
    (3, 0, 3001, 0, "dropped"), (5, 4, 257, 0, "led"),
]
MASKED = [(3, 0, 257, 0, "mixed"), (5, 2, 3001, 300, "mixed"), (7, 6, 256, 300, "mixed"), (5, 0, 255, 0, "spread")]


def parity_case(k):
    return case(*PARITY[k], seed=23000 + k)


def masked_case(k):
    """mixed cases over masks: forwards to leaders that are no members, forwards from a self that is no member, leader records with
    non-member slots -- all in one call (assert_masked_shows)"""
    return case(*MASKED[k], seed=23500 + k, masked=True)


def masked_shows(c):
    w, v, me = c["want"], c["voters"], c["me"]
    g = c["props"]["group"].astype(np.int64)
    fwd = w["what"] == FORWARDED
    to = np.where(fwd, w["to"], 0)
    return {"forwards to a non-member leader": int((fwd & (((v[g] >> to.astype(np.uint16)) & 1) == 0)).sum()),
            "forwards from a non-member self": int((fwd & (((v[g] >> np.uint16(me)) & 1) == 0)).sum()),
            "leader records with a non-member slot": int(((w["what"] == APPENDED) & (np.array([bin(int(x)).count("1") for x in v[g]]) < c["N"])).sum())}
