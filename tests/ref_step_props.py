"""Step with forwarded proposals (include/raftq_step.h raftq_step_set_props): tests/ref_raft_py.Raft and tests/ref_step_voters.VRaft
with the MsgProp arms of 2015-era etcd/raft's three role steps -- nothing else is overridden:

  stepLeader     appendEntry(m.Entries...) -- every entry stamped r.Term and the next index -- which ends in
                 prs[self].maybeUpdate(lastIndex) and maybeCommit(); then bcastAppend (the caller's).  An empty MsgProp panics.
  stepCandidate  the proposal is dropped.
  stepFollower   dropped when r.lead == None, else m.To = r.lead; r.send(m).

Also: a batch driver in the shape of ref_step_voters.step_batch (masked or not; the caller's records or the decoder's), the record
checks that fail a batch, the switch-off form of a batch (a MsgProp is held), and the generators of the GPU tests' inputs.
TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_raft_py as R
from tests import ref_step_voters as V

MsgProp = 2
OutProposed, OutForward = 12, 13
U = np.uint64


class _PropArms:
    """the three MsgProp arms; `leave_out_append` (tests only) makes the leader's arm answer without touching the log -- what a
    Step without the feature's bookkeeping would leave for the messages behind it"""
    leave_out_append = False

    def step_leader(self, m):
        if m.type != MsgProp:
            return super().step_leader(m)
        assert m.entries, "stepLeader panics on an empty MsgProp"
        first = self.last_index + 1
        if not self.leave_out_append:
            self.last_index += len(m.entries)  # appendEntry: es[i].Term = r.Term, es[i].Index = li + 1 + i; raftLog.append
            self.last_term = self.term
            self.prs[self.id].maybe_update(self.last_index)
            self.maybe_commit()
        return R.Result(OutProposed, index=first, log_term=self.term)

    def step_candidate(self, m):
        if m.type != MsgProp:
            return super().step_candidate(m)
        return R.Result()

    def step_follower(self, m):
        if m.type != MsgProp:
            return super().step_follower(m)
        return R.Result() if self.lead == R.NONE else R.Result(OutForward)


@dataclass
class PRaft(_PropArms, R.Raft):
    pass


@dataclass
class PVRaft(_PropArms, V.VRaft):
    pass


def from_node_state(s, g, mask=None, leave_out_append=False):
    n = s.N
    kw = dict(id=s.self_peer + 1, peers=list(range(1, n + 1)), term=int(s.term[g]), vote=int(s.vote[g]), lead=int(s.lead[g]),
              state=int(s.role[g]), elapsed=int(s.elapsed[g]), committed=int(s.committed[g]), last_index=int(s.last_index[g]),
              last_term=int(s.last_term[g]), first_index_of_term=int(s.first_idx[g]))
    if mask is None:
        r = PRaft(**kw)
    else:
        r = PVRaft(voters=frozenset(p + 1 for p in range(n) if (int(mask) >> p) & 1), **kw)
    r.prs = {p + 1: R.Progress(int(s.match[p, g])) for p in range(n)}
    r.votes = {p + 1: (int(s.votes[p, g]) == 1) for p in range(n) if int(s.votes[p, g]) in (1, 2)}
    r.leave_out_append = leave_out_append
    return r


def entry_count(m, frames=False):
    """a record's entry count under RAFTQ_MSGF_ENTRIES: the low half of _resv in a caller's record, the high half in a decoder's"""
    v = int(m["_resv"])
    return v >> 32 if frames else v & 0xFFFFFFFF


def malformed(msgs, n_groups, n_peers, frames=False):
    """-> bool[n]: the type-2 records that fail their batch with the switch on (the header's three cases; HOLD and SKIP win over
    the type)"""
    fl = msgs["_pad"][:, 1]
    looked_at = (msgs["type"] == MsgProp) & ((fl & (V.MSGF_HOLD | V.MSGF_SKIP)) == 0)
    cnt = (msgs["_resv"] >> U(32)) if frames else (msgs["_resv"] & U(0xFFFFFFFF))
    return looked_at & (((fl & V.MSGF_ENTRIES) == 0) | (cnt == 0) | (msgs["from"] >= n_peers))


def step_batch(s, voters, msgs, frames=False, leave_out_append=False):
    """Step for every message, in order, with the switch on -> raftq_step_out_t[]; `s` moves.  voters: the masks, or None for a
    handle without them.  A malformed batch raises ValueError and moves nothing."""
    if malformed(msgs, s.G, s.N, frames).any() or (msgs["group"][(msgs["_pad"][:, 1] & V.MSGF_SKIP) == 0] >= s.G).any():
        raise ValueError("malformed batch")
    out = np.zeros(len(msgs), dtype=pyoracle.STEP_OUT_DT)
    rafts = {}
    for i in range(len(msgs)):
        m = msgs[i]
        fl = int(m["_pad"][1])
        if fl & V.MSGF_SKIP:
            out[i]["type"] = V.OutSkipped
            continue
        g = int(m["group"])
        r = rafts.get(g)
        if r is None:
            r = rafts[g] = from_node_state(s, g, None if voters is None else voters[g], leave_out_append)
            r.held = False
        if fl & V.MSGF_HOLD:
            r.held = True
            V._common(out[i], r, m)
            out[i]["type"] = V.OutHeld
            continue
        t = int(m["type"])
        local = t in (R.MsgHup, R.MsgBeat)
        k = entry_count(m, frames)
        ent_term = 0 if t == MsgProp else int(m["reject_hint"])  # (a proposal's entries: their Term is not looked at)
        res = r.step(R.Message(type=t, frm=0 if local else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
                               index=int(m["index"]), commit=int(m["commit"]), reject=bool(m["reject"]),
                               entries=(ent_term,) * k if fl & V.MSGF_ENTRIES else None, barrier=bool(fl & V.MSGF_BARRIER)))
        V._common(out[i], r, m)
        if res.type == OutForward:
            out[i]["to"] = r.lead - 1  # the one result whose addressee is not the sender
        out[i]["type"], out[i]["index"], out[i]["log_term"], out[i]["reject"], out[i]["flags"] = res.type, res.index, res.log_term, res.reject, res.flags
    for g, r in rafts.items():
        V.to_node_state(r, s, g)
    return out


def hold_form(msgs):
    """the batch as a handle WITHOUT the switch sees a frames call's MsgProps: every type-2 record that is not skipped carries
    RAFTQ_MSGF_HOLD instead of RAFTQ_MSGF_ENTRIES (include/raftq_wire.h) -- the parent's behaviour, from its header"""
    m = msgs.copy()
    fl = m["_pad"][:, 1]
    prop = (m["type"] == MsgProp) & ((fl & V.MSGF_SKIP) == 0)
    m["_pad"][:, 1] = np.where(prop, (fl & ~np.uint8(V.MSGF_ENTRIES)) | np.uint8(V.MSGF_HOLD), fl)
    return m


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
G, N_MSGS = 97, 512
SHAPES = ((1, 0), (3, 0), (5, 4), (9, 8))
MAX_ENTS = 4
N_LEAD, N_CAND, N_LOST = 30, 20, 17  # of G = 97 groups: led, campaigning, following nobody; the other 30 follow somebody
PLANT = 12  # groups per planted outcome
N_FRONT = 6 * PLANT  # the records props_batch plants in front of its random traffic: five kinds of proposal and PLANT acknowledgements


def props_state(rng, n, self_peer, g=G):
    """tests/_stepgen.random_state with the roles dealt, not drawn -- N_LEAD leaders, N_CAND candidates, N_LOST followers without
    a leader, the rest followers of a peer -- so that every MsgProp outcome has groups to happen in.  In PLANT of the led groups
    every peer holds the whole log and nothing of it is committed (first_idx 1): the next maybeCommit there moves the commit
    index, whoever calls it."""
    assert g >= G
    n_lead, n_cand, n_lost = (k * g // G for k in (N_LEAD, N_CAND, N_LOST))  # (the same shares of a larger handle)
    s = _stepgen.random_state(rng, g, n, self_peer)
    role = np.zeros(g, np.uint8)
    role[:n_lead], role[n_lead:n_lead + n_cand] = 2, 1
    perm = rng.permutation(g)
    s.role[perm] = role
    lead, cand = s.role == 2, s.role == 1
    s.vote[:] = rng.integers(0, n + 1, g)
    s.vote[lead | cand] = self_peer + 1
    s.lead[:] = np.where(lead, self_peer + 1, np.where(cand, 0, 1 + (self_peer + 1 + rng.integers(0, max(n - 1, 1), g)) % n))
    s.lead[perm[n_lead + n_cand:n_lead + n_cand + n_lost]] = 0
    s.last_term[:] = np.minimum(s.term, s.last_term)
    s.last_term[lead] = s.term[lead]
    s.last_index[lead] = np.maximum(s.last_index[lead], 1)
    s.last_term[s.last_index == 0] = 0
    s.committed[:] = np.minimum(s.committed, s.last_index)
    s.first_idx[:] = 0
    s.first_idx[lead] = np.maximum(1, (s.last_index[lead] * rng.random(int(lead.sum()))).astype(U))
    for p in range(n):
        s.match[p] = np.where(lead, (s.last_index * rng.random(g)).astype(U), 0)
    s.match[self_peer] = s.last_index
    pend = perm[:PLANT * g // G]
    s.match[:, pend] = s.last_index[pend][None, :]
    s.committed[pend], s.first_idx[pend] = 0, 1
    v = rng.choice([0, 0, 1, 2], (n, g)).astype(np.uint8)
    s.votes[:] = np.where(cand[None, :], v, 0)
    s.votes[self_peer, cand] = 1
    return s


def _prop(m, at, group, k, term=0, frm=0):
    m["group"][at], m["type"][at], m["term"][at], m["from"][at] = group, MsgProp, term, frm
    m["index"][at] = m["log_term"][at] = m["commit"][at] = m["reject_hint"][at] = m["reject"][at] = 0
    m["_pad"][at] = (0, V.MSGF_ENTRIES)
    m["_resv"][at] = k


def props_batch(rng, s, n=N_MSGS, hot=None, max_ents=MAX_ENTS):
    """n records over s (small or lifted by tests/_widegen: every draw is saturating uint64).  In front, PLANT groups of each
    kind get one MsgProp as their first message -- led with a pending commit, led, campaigning, following nobody, following
    somebody -- and the second set of PLANT led groups an acknowledgement right behind it, at the group's term, from another slot,
    for an index inside the new entries.  Behind them tests/_widegen.wide_batch's traffic with three records in ten turned
    into MsgProps: 1..max_ents entries, term 0 (as raft.send leaves it) but for one in eight, which carries a term around the
    group's.  `hot`: a group that gets 40 records of the rest (a run longer than the list walk takes)."""
    n_peers, me = s.N, s.self_peer
    other = (me + 1) % n_peers
    led, cand = np.flatnonzero(s.role == 2), np.flatnonzero(s.role == 1)
    lost, fol = np.flatnonzero((s.role == 0) & (s.lead == 0)), np.flatnonzero((s.role == 0) & (s.lead != 0))
    pending = led[(s.committed[led] == 0) & (s.match[:, led] == s.last_index[led][None, :]).all(axis=0)]
    pend, plain = pending[:PLANT], np.setdiff1d(led, pending)[:PLANT]
    sets = [pend, plain, cand[:PLANT], lost[:PLANT], fol[:PLANT]]
    assert all(len(x) == PLANT for x in sets), [len(x) for x in sets]
    first = rng.permutation(np.concatenate(sets))
    n_front = len(first) + PLANT
    assert n_front == N_FRONT
    m = WG.wide_batch(rng, s, n)
    k_front = rng.integers(2, max_ents + 1, len(first))  # (two at least: an index strictly inside the new entries exists)
    for at, (g, k) in enumerate(zip(first, k_front)):
        _prop(m, at, g, int(k), frm=other)
    for j, g in enumerate(plain):  # the acknowledgement behind the proposal
        at = len(first) + j
        k = int(k_front[np.flatnonzero(first == g)[0]])
        m[at] = np.zeros(1, m.dtype)[0]
        m["group"][at], m["type"][at], m["term"][at], m["from"][at] = g, R.MsgAppResp, s.term[g], other
        m["index"][at] = s.last_index[g] + U(1 + int(rng.integers(0, k)))
    rest = np.arange(n_front, n)
    if hot is not None:
        m["group"][rest[:40]] = hot
    for at in rest[rng.random(len(rest)) < 0.3]:
        g = int(m["group"][at])
        term = int(WG.pick(rng, s.term[g:g + 1], [-1, 0, 1], 1)[0]) if rng.random() < 0.125 else 0
        _prop(m, at, g, int(rng.integers(1, max_ents + 1)) | (int(rng.integers(0, 2**31)) << 32), term=term, frm=int(rng.integers(0, n_peers)))
    WG.guard(m["term"], m["index"], s.last_index + U(max_ents) * np.bincount(m["group"].astype(np.int64), minlength=s.G).astype(U))
    return m


def outcomes(s0, voters, m, want):
    """what the input shows of the feature, read off the reference's own output -> dict of counts"""
    prop = (m["type"] == MsgProp) & ((m["_pad"][:, 1] & (V.MSGF_HOLD | V.MSGF_SKIP)) == 0)
    t, fl = want["type"], want["flags"]
    none = prop & (t == R.OutNone) & ((m["term"] == 0) | (m["term"] >= want["term"]))  # (not the stale-term kind of "ignored")
    without = step_batch(V.copy_state(s0), voters, m, leave_out_append=True)
    decided = ("type", "index", "reject", "flags", "commit")  # (last_index differs behind every left-out append: not a decision)
    ack = (m["type"] == R.MsgAppResp) & np.logical_or.reduce([want[k] != without[k] for k in decided])
    return {"proposed": int((prop & (t == OutProposed)).sum()),
            "proposed+committed": int((prop & (t == OutProposed) & ((fl & R.FlagCommitted) != 0)).sum()),
            "forward": int((prop & (t == OutForward)).sum()),
            "dropped, candidate": int((none & (want["role"] == 1)).sum()),
            "dropped, no leader": int((none & (want["role"] == 0) & (want["lead"] == 0)).sum()),
            "acks decided otherwise without the append": len(np.unique(m["group"][ack])),
            "share of type 2": float((m["type"] == MsgProp).mean())}


FLOORS = {"proposed": 8, "proposed+committed": 8, "forward": 8, "dropped, candidate": 8, "dropped, no leader": 8,
          "acks decided otherwise without the append": 8, "share of type 2": 0.25}


def assert_discriminates(s0, voters, m, want, what=""):
    got = outcomes(s0, voters, m, want)
    for k, floor in FLOORS.items():
        assert got[k] >= floor, (what, k, got)
    return got


def case(n, self_peer, seed, band=None, masks=None, hot=False, g=G):
    """one (start state, voters | None, batch, the reference's records, the state after): the unit every GPU test loads and steps.
    band: lift the state with tests/_widegen first.  masks: "random" (ref_step_voters' with a one-voter led group and a led group
    whose leader does not vote planted) or None."""
    rng = np.random.default_rng(seed)
    s = props_state(rng, n, self_peer, g)
    if band is not None:
        s = WG.lift(s, band, rng)
    voters = None
    if masks:
        voters = rng.integers(0, 1 << n, g).astype(np.uint16) | np.uint16(1 << self_peer)
        led = np.flatnonzero(s.role == 2)
        voters[led[-4:-2]] = 1 << self_peer  # a one-voter group: the leader commits on its own proposal
        if n > 1:
            voters[led[-2:]] = ((1 << n) - 1) & ~(1 << self_peer)  # the leader does not vote
    m = props_batch(rng, s, hot=int(rng.integers(0, g)) if hot else None)
    start = V.copy_state(s)
    want = step_batch(s, voters, m)
    WG.guard(s.term, s.last_term, s.last_index, s.committed, s.first_idx, s.match)
    for a in (m, want):
        a.setflags(write=False)
    return start, voters, m, want, s


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def frames_of(rng, m, self_peer, empty_props=0.15):
    """a batch of Step records as the rafthttp frames a peer would have sent them in, all addressed to self_peer: a MsgApp that
    says what it carries and every MsgProp get their entries (a MsgApp's last one at the term the record names; a proposal's
    with any Term and Index: appendEntry overwrites them), `empty_props` of the MsgProps get none.  The local kinds (MsgHup,
    MsgBeat) go out as they are: kinds a peer never sends.  -> (stream, frame_off)"""
    from oracle import pywire as W

    n = len(m)
    w = np.zeros(n, W.WIRE_MSG_DT)
    for k in ("group", "term", "log_term", "index", "commit", "reject_hint", "from", "type", "reject"):
        w[k] = m[k]
    w["to"] = self_peer
    prop, app = m["type"] == MsgProp, m["type"] == R.MsgApp
    says = (m["_pad"][:, 1] & V.MSGF_ENTRIES) != 0
    w["reject_hint"] = np.where(prop | app, 0, w["reject_hint"])
    k = np.where(says, m["_resv"] & U(0xFFFFFFFF), 0).astype(np.int64)
    k = np.where(prop & (rng.random(n) < empty_props), 0, k)
    w["n_ents"] = k
    w["ent_first"] = np.where(k > 0, np.cumsum(k) - k, 0)
    ne = int(k.sum())
    e = np.zeros(ne, W.WIRE_ENT_DT)
    owner = np.repeat(np.arange(n), k)
    nth = np.arange(ne) - (np.cumsum(k) - k)[owner]
    e["term"] = np.where(prop[owner], rng.integers(0, 2**40, ne).astype(U), m["reject_hint"][owner])
    e["index"] = np.where(prop[owner], rng.integers(0, 2**40, ne).astype(U), m["index"][owner] + U(1) + nth.astype(U))
    e["data_len"] = rng.integers(0, 40, ne)
    e["data_off"] = np.cumsum(e["data_len"]) - e["data_len"] if ne else 0
    pool = rng.integers(0, 256, int(e["data_len"].sum()) + 1, dtype=np.uint8)
    return W.wire_encode(w, e, pool)


def node_filter(wm, we, n_groups, n_peers, self_peer, tail_appends, props):
    """what the frames calls' decoder makes of the decoded records (include/raftq_wire.h) -> (the records handed to the caller,
    the same as Step reads them, in a caller's form).  props = False is tests/test_wire_gpu._node_filter, the restatement the
    existing suites hold the switch-off behaviour to; props = True changes what the header says the switch changes: a MsgProp
    frame with entries carries RAFTQ_MSGF_ENTRIES in place of RAFTQ_MSGF_HOLD, one without carries RAFTQ_MSGF_SKIP."""
    from tests.test_wire_gpu import _node_filter

    out, rec = _node_filter(wm, we, n_groups, n_peers, self_peer, tail_appends)
    if props:
        held = (out["flags"] & V.MSGF_HOLD) != 0
        assert (out["type"][held] == MsgProp).all()
        fl = (out["flags"] & ~np.uint8(V.MSGF_HOLD)) | np.where(out["n_ents"] > 0, V.MSGF_ENTRIES, V.MSGF_SKIP).astype(np.uint8)
        out["flags"] = np.where(held, fl, out["flags"])
        rec["_pad"][:, 1] = out["flags"]
    return out, rec


def frames_case(n, self_peer, seed, g=G, n_frames=N_MSGS, band=None, hot=False, with_without=True):
    """one frames call: (start state, stream, frame_off, the oracle's decode (records, entry headers), per switch setting the
    filtered records, Step's records and the reference's results and state after).  The state is props_state's, the traffic
    props_batch's as frames."""
    from oracle import pywire as W

    rng = np.random.default_rng(seed)
    s = props_state(rng, n, self_peer, g)
    if band is not None:
        s = WG.lift(s, band, rng)
    m = props_batch(rng, s, n_frames, hot=int(rng.integers(0, g)) if hot else None)
    stream, off = frames_of(rng, m, self_peer)
    wm, we, bad = W.wire_decode(stream, off)
    assert bad == 0
    by_switch = {}
    for props in ((True, False) if with_without else (True,)):
        want_m, rec = node_filter(wm, we, g, n, self_peer, True, props)
        after = V.copy_state(s)
        want_o = step_batch(after, None, rec)
        by_switch[props] = (want_m, rec, want_o, after)
    return s, stream, off, wm, we, by_switch


def case_list():
    """the arguments of every case() and frames_case() the GPU tests step (tests/test_step_props_ref.py asserts that each one
    tells the feature from its absence) -> (case kwargs list, frames_case kwargs list)"""
    cases, frames = [], []
    for n, me in SHAPES:
        cases.append(dict(n=n, self_peer=me, seed=9300 + n))
        cases.append(dict(n=n, self_peer=me, seed=9310 + n, hot=True))
        cases.append(dict(n=n, self_peer=me, seed=9320 + n, masks="random"))
        frames.append(dict(n=n, self_peer=me, seed=9340 + n))
    for band in WG.BAND_NAMES:
        for n, me in SHAPES[1:]:
            cases.append(dict(n=n, self_peer=me, seed=9330 + n + 100 * WG.BAND_NAMES.index(band), band=band))
        frames.append(dict(n=5, self_peer=4, seed=9350 + WG.BAND_NAMES.index(band), band=band))
    frames.append(dict(n=3, self_peer=0, seed=9360, hot=True))
    return cases, frames


BIG = dict(n=3, self_peer=1, seed=9370, g=32768, n_frames=65536, with_without=False)  # every tile path of the decoder and the walks
