"""PreVote (include/raftq.h "PreVote", include/raftq_step.h "PreVote"): tests/ref_check_quorum.CRaft / CVRaft with the five Step
rules of etcd/raft's preVote and its answer to a stale leader -- Step's head (the term rules, the vote rule in front of the role
functions) is restated here, the role functions and everything below them are inherited:

  1  MsgHup on a non-leader is becomePreCandidate (role 3, no term moves); an own grant that is the quorum campaigns at once
  2  m.Term > r.Term: MsgPreVote is ignored inside the lease and changes nothing outside it; a granting MsgPreVoteResp changes
     nothing, a rejecting one is becomeFollower(m.Term, None)
  3  0 < m.Term < r.Term: MsgPreVote is rejected with the own term; MsgApp / MsgHeartbeat get RAFTQ_OUT_TERM_RESP
  4  a MsgPreVote that got this far is answered by one rule in every role and changes nothing
  5  role 3 is stepped by the candidate's arm, polling MsgPreVoteResp: a won pre-election campaigns, a lost one follows nobody

Also: a batch driver in the shape of ref_check_quorum.step_batch, the generators of the GPU tests' inputs, and a three-node
scripted cluster (the reason for the feature) with ref_check_quorum's Tick for the clock.
TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

MsgPreVote, MsgPreVoteResp = 17, 18
PRE = 3  # RAFTQ_ROLE_PRE_CANDIDATE
OutPreCampaign, OutPreVoteResp, OutTermResp = 14, 15, 16
ELECTION_TICK = Q.ELECTION_TICK


class _PreVoteArms:
    """the five rules; `pv_out` (tests only): rule numbers this instance does NOT apply.  Without rule 1 MsgHup campaigns; without
    2 and 3 the two kinds get what every other kind gets from the term rules; without 4 a MsgPreVote falls to the role functions,
    none of which knows it; without 5 role 3 is what a Step without the switch takes it for, a follower."""
    pv_out = frozenset()

    def _recorded(self):
        return sum(1 for p in self.votes if p in self.members())

    def _campaign(self):
        self.become_candidate()
        if self.q() == self.poll(self.id, True):
            self.become_leader()
            return R.Result(R.OutBecameLeader, self.last_index, self.last_term)
        return R.Result(R.OutCampaign, self.last_index, self.last_term)

    def _step(self, m):
        out = self.pv_out
        if m.type == R.MsgHup:
            if self.state == R.StateLeader:
                return R.Result()
            if 1 in out:
                return self._campaign()
            self.state, self.lead, self.votes, self.elapsed = PRE, R.NONE, {}, 0  # becomePreCandidate
            if self.q() == self.poll(self.id, True):
                return self._campaign()
            return R.Result(OutPreCampaign, self.last_index, self.last_term)
        if m.term == 0:
            pass
        elif m.term > self.term:
            pre = m.type in (MsgPreVote, MsgPreVoteResp) and 2 not in out
            if (m.type == R.MsgVote or (pre and m.type == MsgPreVote)) and 3 not in self.leave_out and self.in_lease():
                return R.Result()
            if not (pre and (m.type == MsgPreVote or not m.reject)):
                self.become_follower(m.term, R.NONE if m.type == R.MsgVote or pre else m.frm)
        elif m.term < self.term:
            if 3 not in out:
                if m.type == MsgPreVote:
                    return R.Result(OutPreVoteResp, index=self.term, reject=1)
                if m.type in (R.MsgApp, R.MsgHeartbeat):
                    return R.Result(OutTermResp)
            return R.Result()
        if m.type == MsgPreVote and 4 not in out:
            if (self.vote == R.NONE or m.term > self.term or self.vote == m.frm) and self.is_up_to_date(m.index, m.log_term):
                return R.Result(OutPreVoteResp, index=m.term)
            return R.Result(OutPreVoteResp, index=self.term, reject=1)
        if self.state == PRE:
            return self.step_follower(m) if 5 in out else self.step_pre_candidate(m)
        return {R.StateLeader: self.step_leader, R.StateCandidate: self.step_candidate, R.StateFollower: self.step_follower}[self.state](m)

    def step_pre_candidate(self, m):
        if m.type == MsgPreVoteResp:
            gr = self.poll(m.frm, not m.reject)
            if self.q() == gr:
                return self._campaign()
            if self.q() == self._recorded() - gr:
                self.become_follower(self.term, R.NONE)
            return R.Result()
        if m.type == R.MsgVoteResp:
            return R.Result()
        return self.step_candidate(m)  # MsgApp, MsgHeartbeat, MsgVote of the own term; everything else is dropped there too


@dataclass
class PRaft(_PreVoteArms, Q.CRaft):
    pass


@dataclass
class PVRaft(_PreVoteArms, Q.CVRaft):
    pass


LOCAL = (R.MsgHup, R.MsgBeat, Q.MsgCheckQuorum)


def step_batch(s, voters, active, lead_elapsed, msgs, election_tick=ELECTION_TICK, leave_out=frozenset()):
    """Step for every message, in order, with both switches on -> raftq_step_out_t[]; `s`, `active` and `lead_elapsed` move.
    voters: the masks, or None for a handle without them.  leave_out: PreVote's rule numbers."""
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
            r = rafts[g] = Q.from_node_state(s, g, None if voters is None else voters[g], active[g], lead_elapsed[g], election_tick,
                                             classes=(PRaft, PVRaft))
            r.pv_out = frozenset(leave_out)
            r.held = False
        if fl & V.MSGF_HOLD:
            r.held = True
            V._common(out[i], r, m)
            out[i]["type"] = V.OutHeld
            continue
        t = int(m["type"])
        res = r.step(R.Message(type=t, frm=0 if t in LOCAL else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
                               index=int(m["index"]), commit=int(m["commit"]), reject=bool(m["reject"]),
                               entries=(int(m["reject_hint"]),) * (int(m["_resv"]) & 0xFFFFFFFF) if fl & V.MSGF_ENTRIES else None,
                               barrier=bool(fl & V.MSGF_BARRIER)))
        V._common(out[i], r, m)
        out[i]["type"], out[i]["index"], out[i]["log_term"], out[i]["reject"], out[i]["flags"] = res.type, res.index, res.log_term, res.reject, res.flags
    for g, r in rafts.items():
        V.to_node_state(r, s, g)
        active[g] = sum(1 << (p - 1) for p in r.active)
        lead_elapsed[g] = r.lead_elapsed
    return out


# ---- the Step inputs ---------------------------------------------------------------------------------------------------------------
G, N_MSGS = Q.G, Q.N_MSGS
SHAPES = Q.SHAPES
PLANT = 4


def _rec(m, at, group, type, term=0, frm=0, index=0, log_term=0, reject=0, flags=0):
    Q._rec(m, at, group, type, term, frm, index, log_term, reject)
    m["_pad"][at] = (0, flags)


def step_case(n, self_peer, seed, masks=False, hot=False, g=G, n_msgs=N_MSGS, band=None, plants=None):
    """one (start state, voters | None, batch, the reference's records, (state, active, lead_elapsed) after).
    ref_step_props.props_state's dealt roles -- every third candidate made a pre-candidate --, elapsed on both sides of
    election_tick, and _stepgen's traffic with half the MsgVote / MsgVoteResp records turned into their pre-election kinds (so every
    term relation meets every role) and one record in ten into a MsgCheckQuorum.  In front, per kind PLANT groups with one directed
    exchange each:
      following nobody      MsgHup, then grants from q - 1 peers at term + 1: pre-candidate, then the campaign (or, N = 1, the lot at once)
      following nobody      MsgHup, then rejections from q peers at the own term: follows nobody again, Term and Vote kept
      following nobody      MsgHup, then ONE rejection of a higher term: becomeFollower(that term, None)
      following, elapsed 0  a MsgPreVote of the next term: in lease, ignored
      following, past it    the same: out of lease, granted, nothing changes
      following             a MsgHeartbeat and a MsgApp (barrier, entries) of the term before, then a MsgPreVote of it: TERM_RESP twice, a rejection
      led                   a MsgPreVote of the next term (ignored) and one of the own (rejected: the log is behind)
      candidate             a MsgPreVoteResp (ignored) and a MsgPreVote of the own term
    `hot`: a group following nobody with 40 records in a row -- MsgHup, then responses of both kinds from every peer, again and again.
    band: the state lifted by tests/_widegen first and the traffic drawn by its wide_batch; in
    b32 / b63 the `win`, `bump`, in-lease, out-of-lease and led groups stand at term B - 1 -- the MsgPreVote or MsgPreVoteResp "of the
    next term" is B, "two up" beyond it -- and the stale groups at term B: their TERM_RESP answers the term before from across the
    boundary.  plants: a dict that is told these groups."""
    rng = np.random.default_rng(seed)
    s = P.props_state(rng, n, self_peer, g)
    if band is not None:
        s = WG.lift(s, band, rng)
    s.elapsed[:] = rng.integers(0, 2 * ELECTION_TICK, g)
    cand = np.flatnonzero(s.role == 1)
    s.role[cand[::3]] = PRE
    full = (1 << n) - 1
    active = rng.integers(0, full + 1, g).astype(np.uint16)
    lead_elapsed = rng.integers(0, ELECTION_TICK, g).astype(np.uint32)
    voters = None
    if masks:  # (self votes in three groups of four: the own grant is recorded either way and counts only there)
        voters = rng.integers(0, full + 1, g).astype(np.uint16)
        voters[rng.random(g) < 0.75] |= np.uint16(1 << self_peer)
    lost = np.flatnonzero((s.role == 0) & (s.lead == 0))
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0))
    led = np.flatnonzero(s.role == 2)
    cnd = np.flatnonzero(s.role == 1)
    assert len(lost) >= 3 * PLANT + 1 and len(fol) >= 3 * PLANT and len(led) >= PLANT and len(cnd) >= PLANT, (len(lost), len(fol), len(led), len(cnd))
    win, lose, bump = (lost[k * PLANT:(k + 1) * PLANT] for k in range(3))
    hot_group = int(lost[3 * PLANT])
    in_lease, out_lease, stale = (fol[k * PLANT:(k + 1) * PLANT] for k in range(3))
    led_p, cnd_p = led[:PLANT], cnd[:PLANT]
    planted = np.concatenate([win, lose, bump, [hot_group], in_lease, out_lease, stale, led_p, cnd_p])
    if masks:
        voters[planted] = full
    s.elapsed[in_lease], s.elapsed[out_lease] = 0, ELECTION_TICK + 3
    s.term[stale] = np.maximum(s.term[stale], 2)
    s.last_term[stale] = np.minimum(s.last_term[stale], s.term[stale])
    free = np.setdiff1d(np.arange(g), planted)
    if band is None:
        m = _stepgen.random_batch(rng, s, n_msgs)
    else:
        if WG.BANDS[band]:
            WG.set_term(s, np.concatenate([win, bump, in_lease, out_lease, led_p]), WG.BANDS[band] - 1)
            WG.set_term(s, stale, WG.BANDS[band])
        m = WG.wide_batch(rng, s, n_msgs)
    if plants is not None:
        plants.update(win=win, bump=bump, in_lease=in_lease, out_lease=out_lease, stale=stale, led=led_p)
    others = [(self_peer + 1 + k) % n for k in range(n - 1)]
    peer = others[0] if others else 0
    q = n // 2 + 1
    at = 0
    for grp in win:
        _rec(m, at, grp, R.MsgHup); at += 1
        for p in others[:q - 1]:
            _rec(m, at, grp, MsgPreVoteResp, term=int(s.term[grp]) + 1, frm=p); at += 1
    for grp in lose:
        _rec(m, at, grp, R.MsgHup); at += 1
        for p in others[:q]:
            _rec(m, at, grp, MsgPreVoteResp, term=int(s.term[grp]), frm=p, reject=1); at += 1
    for grp in bump:
        _rec(m, at, grp, R.MsgHup); at += 1
        _rec(m, at, grp, MsgPreVoteResp, term=int(s.term[grp]) + 2, frm=peer, reject=1); at += 1
    for grp in np.concatenate([in_lease, out_lease]):
        _rec(m, at, grp, MsgPreVote, term=int(s.term[grp]) + 1, frm=others[-1] if others else 0, index=int(s.last_index[grp]) + 5, log_term=int(s.term[grp]) + 1); at += 1
    for grp in stale:
        t = int(s.term[grp]) - 1
        _rec(m, at, grp, R.MsgHeartbeat, term=t, frm=peer); at += 1
        _rec(m, at, grp, R.MsgApp, term=t, frm=peer, index=int(s.last_index[grp]), log_term=int(s.last_term[grp]), flags=V.MSGF_BARRIER | V.MSGF_ENTRIES); at += 1
        _rec(m, at, grp, MsgPreVote, term=t, frm=peer, index=int(s.last_index[grp]) + 5, log_term=t); at += 1
    for grp in led_p:
        _rec(m, at, grp, MsgPreVote, term=int(s.term[grp]) + 1, frm=peer, index=int(s.last_index[grp]) + 5, log_term=int(s.term[grp]) + 1); at += 1
        _rec(m, at, grp, MsgPreVote, term=int(s.term[grp]), frm=peer, index=0, log_term=0); at += 1
    for grp in cnd_p:
        _rec(m, at, grp, MsgPreVoteResp, term=int(s.term[grp]), frm=peer); at += 1
        _rec(m, at, grp, MsgPreVote, term=int(s.term[grp]), frm=peer, index=int(s.last_index[grp]) + 5, log_term=int(s.term[grp])); at += 1
    assert at < n_msgs // 2, at
    rest = np.arange(at, n_msgs)
    m["group"][rest] = rng.choice(free, len(rest))  # (the directed exchanges stay undisturbed)
    if hot:
        t0 = int(s.term[hot_group])
        for j, i in enumerate(rest[:40]):
            k = j % 8
            if k == 0:
                _rec(m, i, hot_group, R.MsgHup)
            elif j < 8:  # the first pre-election is won: grants at term + 1 from one peer after the other
                _rec(m, i, hot_group, MsgPreVoteResp, term=t0 + 1, frm=others[(k - 1) % len(others)])
            else:
                _rec(m, i, hot_group, MsgPreVoteResp if k % 2 else R.MsgVoteResp, term=t0 + int(rng.integers(0, 3)), frm=int(rng.integers(0, n)),
                     reject=int(rng.random() < 0.4))
        rest = rest[40:]
    turn = rest[rng.random(len(rest)) < 0.5]
    m["type"][turn] = np.where(m["type"][turn] == R.MsgVote, MsgPreVote, np.where(m["type"][turn] == R.MsgVoteResp, MsgPreVoteResp, m["type"][turn]))
    for i in rest[rng.random(len(rest)) < 0.1]:
        _rec(m, i, int(m["group"][i]), Q.MsgCheckQuorum, frm=int(rng.integers(0, 256)))
    start = (V.copy_state(s), active.copy(), lead_elapsed.copy())
    if band is not None:
        WG.guard_case(s, m)
    want = step_batch(s, voters, active, lead_elapsed, m)
    if band is not None:
        WG.guard_case(s, m)
    for a in (m, want):
        a.setflags(write=False)
    return start, voters, m, want, (s, active, lead_elapsed)


def case_list():
    """the arguments of every step_case() the GPU tests step (tests/test_pre_vote_ref.py shows that each one discriminates)"""
    cases = []
    for n, me in SHAPES:
        cases.append(dict(n=n, self_peer=me, seed=9800 + n))
        cases.append(dict(n=n, self_peer=me, seed=9810 + n, masks=True))
    cases.append(dict(n=3, self_peer=1, seed=9820, hot=True))
    cases.append(dict(n=5, self_peer=0, seed=9821, hot=True, masks=True))
    for k, band in enumerate(WG.BAND_NAMES):  # appended: the positions above are what the GPU tests pick by
        cases.append(dict(n=3, self_peer=0, seed=9830 + k, band=band))
        cases.append(dict(n=9, self_peer=8, seed=9840 + k, masks=True, band=band))
    return cases


case_id = Q.case_id


def changed_records(start, voters, m, want, after, rule):
    """the records whose result, or whose group's final state, is another when `rule` is left out -> their batch positions"""
    st = (V.copy_state(start[0]), start[1].copy(), start[2].copy())
    without = step_batch(st[0], voters, st[1], st[2], np.array(m), leave_out={rule})
    k = want.dtype.itemsize
    differs = (without.view(np.uint8).reshape(-1, k) != np.array(want).view(np.uint8).reshape(-1, k)).any(axis=1)
    sa, sb = st[0], after[0]
    moved = np.zeros(sa.G, bool)
    for name, _ in pyoracle.NodeState.FIELDS:
        moved |= getattr(sa, name) != getattr(sb, name)
    moved |= (sa.match != sb.match).any(axis=0) | (sa.votes != sb.votes).any(axis=0) | (st[1] != after[1]) | (st[2] != after[2])
    return np.flatnonzero(differs | moved[m["group"].astype(np.int64)])


# ---- three nodes, scripted ---------------------------------------------------------------------------------------------------------
def route(k, outs, n=3):
    """what node k's host sends for its results (include/raftq_step.h RAFTQ_OUT_*) -> {addressee: raftq_msg_t[]}, in
    result order.  The scenario moves terms, roles and leaders, not logs: becomeLeader's MsgApps are not sent, a heartbeat carries
    commit 0."""
    per = {p: [] for p in range(n) if p != k}
    for o in outs:
        t = int(o["type"])
        kw = dict(group=int(o["group"]), frm=k)
        if t == R.OutBcastHeartbeat:
            one, to = dict(type=R.MsgHeartbeat, term=int(o["term"]), **kw), None
        elif t == R.OutHeartbeatResp:
            one, to = dict(type=R.MsgHeartbeatResp, term=int(o["term"]), **kw), int(o["to"])
        elif t == R.OutCampaign:
            one, to = dict(type=R.MsgVote, term=int(o["term"]), index=int(o["index"]), log_term=int(o["log_term"]), **kw), None
        elif t == OutPreCampaign:
            one, to = dict(type=MsgPreVote, term=int(o["term"]) + 1, index=int(o["index"]), log_term=int(o["log_term"]), **kw), None
        elif t == R.OutVoteResp:
            one, to = dict(type=R.MsgVoteResp, term=int(o["term"]), reject=int(o["reject"]), **kw), int(o["to"])
        elif t == OutPreVoteResp:
            one, to = dict(type=MsgPreVoteResp, term=int(o["index"]), reject=int(o["reject"]), **kw), int(o["to"])
        elif t == OutTermResp:
            one, to = dict(type=R.MsgAppResp, term=int(o["term"]), **kw), int(o["to"])
        else:
            continue
        for p in (per if to is None else (to,)):
            per[p].append(one)
    out = {}
    for p, lst in per.items():
        a = np.zeros(len(lst), pyoracle.STEP_MSG_DT)
        for i, one in enumerate(lst):
            _rec(a, i, **one)
        out[p] = a
    return out


class Cluster:
    """Three nodes over G groups, node 0 leading every group at term 1 with an equal log everywhere.  One round = every node in
    turn: a Tick (ref_check_quorum.tick_array), then ONE Step batch -- what arrived since its last turn, then the Tick's MsgHup /
    MsgBeat / MsgCheckQuorum records in group order -- whose results are routed at once.  A message to or from a node in `cut` is
    dropped.  on_tick(k, actions) and on_step(k, batch, results) are called after each move (the GPU test's hooks)."""
    N = 3

    def __init__(self, g, pre_vote, election_tick=5, heartbeat_tick=2, seed=0xC0FFEE, on_tick=None, on_step=None):
        self.g, self.pre_vote, self.et, self.ht, self.seed = g, pre_vote, election_tick, heartbeat_tick, seed
        self.on_tick, self.on_step = on_tick, on_step
        self.s, self.active, self.lead_elapsed = [], [], []
        for k in range(self.N):
            s = pyoracle.NodeState(g, self.N, k)
            s.term[:], s.lead[:], s.vote[:], s.last_index[:], s.last_term[:] = 1, 1, 1, 5, 1
            s.match[k] = 5
            if k == 0:
                s.role[:], s.first_idx[:] = 2, 1
            self.s.append(s)
            self.active.append(np.zeros(g, np.uint16))
            self.lead_elapsed.append(np.zeros(g, np.uint32))
        self.inbox = [np.zeros(0, pyoracle.STEP_MSG_DT) for _ in range(self.N)]
        self.cut = set()
        self.tick_no = [0] * self.N
        self.rounds = 0

    def _step(self, s, active, lead_elapsed, msgs):
        if self.pre_vote:
            return step_batch(s, None, active, lead_elapsed, msgs, self.et)
        return Q.step_batch(s, None, active, lead_elapsed, msgs, self.et)

    def turn(self, k):
        s = self.s[k]
        el, act, ac, le, _, _ = Q.tick_array(pyoracle, s.role, s.elapsed, self.active[k], self.lead_elapsed[k], None, k, self.N, self.et, self.ht,
                                             self.seed + k, self.tick_no[k])
        self.tick_no[k] += 1
        s.elapsed[:], self.active[k][:], self.lead_elapsed[k][:] = el, ac, le
        if self.on_tick:
            self.on_tick(k, act)
        local = np.zeros(int((act != 0).sum()), pyoracle.STEP_MSG_DT)
        at = 0
        for a, t in ((1, R.MsgHup), (2, R.MsgBeat), (3, Q.MsgCheckQuorum)):
            for grp in np.flatnonzero(act == a):
                _rec(local, at, int(grp), t); at += 1
        batch = np.concatenate([self.inbox[k], local])
        self.inbox[k] = np.zeros(0, pyoracle.STEP_MSG_DT)
        if len(batch) == 0:
            return
        outs = self._step(s, self.active[k], self.lead_elapsed[k], batch)
        if self.on_step:
            self.on_step(k, batch, outs)
        if k in self.cut:
            return
        for p, msgs in route(k, outs, self.N).items():
            if p not in self.cut:
                self.inbox[p] = np.concatenate([self.inbox[p], msgs])

    def round(self):
        for k in range(self.N):
            self.turn(k)
        self.rounds += 1

    def run(self, rounds):
        for _ in range(rounds):
            self.round()

    def leaders(self):
        """[G] the number of nodes leading each group, [G] the slot of one of them"""
        lead = np.stack([s.role == 2 for s in self.s])
        return lead.sum(axis=0), lead.argmax(axis=0)

    def converged(self):
        """every group has ONE leader, at the largest term any node holds, and the other two follow it"""
        cnt, who = self.leaders()
        if not (cnt == 1).all():
            return False
        terms = np.stack([s.term for s in self.s])
        top = terms.max(axis=0)
        for k in range(self.N):
            mine = who == k
            follows = (self.s[k].role == 0) & (self.s[k].lead == who + 1) & (self.s[k].term == top)
            leads = (self.s[k].role == 2) & (self.s[k].term == top)
            if not np.where(mine, leads, follows).all():
                return False
        return True
