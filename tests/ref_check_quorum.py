"""CheckQuorum (include/raftq.h "CheckQuorum", include/raftq_step.h "CheckQuorum"): tests/ref_raft_py.Raft and
tests/ref_step_voters.VRaft with the four Step rules of etcd/raft's checkQuorum -- nothing else is overridden:

  1  stepLeader, MsgAppResp / MsgHeartbeatResp from p: Progress[p].RecentActive = true, in front of the reject branch
  2  reset() clears every RecentActive and the leader's electionElapsed
  3  Step, m.Term > r.Term, MsgVote only: ignored while inLease = leader || (lead != None && elapsed < electionTimeout)
  4  MsgCheckQuorum (type 12, local): a leader counts the active members (self included) against q, clears the bits and steps
     down below q; every other role ignores it

Also: a batch driver in the shape of ref_step_props.step_batch, the Tick stated twice -- array-shaped on oracle.pyoracle.tick (and
ref_tick_members.tick_array over masks) and as a per-group loop -- and the generators of the GPU tests' inputs.
TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V
from tests import ref_tick_members as TM

MsgCheckQuorum = 12
LEADER = 2
ELECTION_TICK = 10  # the Step inputs' (the reference's ElectionTick, raft.go:154)


class _CheckArms:
    """the four rules; `leave_out` (tests only): rule numbers this instance does NOT apply -- what a Step without that rule does"""
    active = frozenset()   # raft IDs whose Progress.RecentActive is true
    lead_elapsed = 0
    election_tick = ELECTION_TICK
    leave_out = frozenset()

    def members(self):
        return self.voters if hasattr(self, "voters") else frozenset(self.prs)

    def reset(self, term):
        super().reset(term)
        if 2 not in self.leave_out:
            self.active = frozenset()
            self.lead_elapsed = 0

    def in_lease(self):
        return self.state == R.StateLeader or (self.lead != R.NONE and self.elapsed < self.election_tick)

    def _step(self, m):
        if 3 not in self.leave_out and m.type == R.MsgVote and m.term > self.term and self.in_lease():
            return R.Result()
        return super()._step(m)

    def step_leader(self, m):
        if 1 not in self.leave_out and m.type in (R.MsgAppResp, R.MsgHeartbeatResp):
            self.active = self.active | {m.frm}
        if m.type != MsgCheckQuorum:
            return super().step_leader(m)
        if 4 in self.leave_out:
            return R.Result()
        act = len((self.active | {self.id}) & self.members())
        self.active = frozenset()
        if act < self.q():
            self.become_follower(self.term, R.NONE)
        return R.Result()


@dataclass
class CRaft(_CheckArms, R.Raft):
    pass


@dataclass
class CVRaft(_CheckArms, V.VRaft):
    pass


def from_node_state(s, g, mask, active, lead_elapsed, election_tick, leave_out=frozenset(), classes=None):
    """classes: the (unmasked, masked) pair to build -- (CRaft, CVRaft) unless a module that composes more arms passes its own"""
    plain, masked = classes or (CRaft, CVRaft)
    n = s.N
    kw = dict(id=s.self_peer + 1, peers=list(range(1, n + 1)), term=int(s.term[g]), vote=int(s.vote[g]), lead=int(s.lead[g]),
              state=int(s.role[g]), elapsed=int(s.elapsed[g]), committed=int(s.committed[g]), last_index=int(s.last_index[g]),
              last_term=int(s.last_term[g]), first_index_of_term=int(s.first_idx[g]))
    if mask is None:
        r = plain(**kw)
    else:
        r = masked(voters=frozenset(p + 1 for p in range(n) if (int(mask) >> p) & 1), **kw)
    r.prs = {p + 1: R.Progress(int(s.match[p, g])) for p in range(n)}
    r.votes = {p + 1: (int(s.votes[p, g]) == 1) for p in range(n) if int(s.votes[p, g]) in (1, 2)}
    r.active = frozenset(p + 1 for p in range(16) if (int(active) >> p) & 1)
    r.lead_elapsed, r.election_tick, r.leave_out = int(lead_elapsed), int(election_tick), frozenset(leave_out)
    return r


def step_batch(s, voters, active, lead_elapsed, msgs, election_tick=ELECTION_TICK, leave_out=frozenset()):
    """Step for every message, in order, with the switch on -> raftq_step_out_t[]; `s`, `active` and `lead_elapsed` move.
    voters: the masks, or None for a handle without them."""
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
            r = rafts[g] = from_node_state(s, g, None if voters is None else voters[g], active[g], lead_elapsed[g], election_tick, leave_out)
            r.held = False
        if fl & V.MSGF_HOLD:
            r.held = True
            V._common(out[i], r, m)
            out[i]["type"] = V.OutHeld
            continue
        t = int(m["type"])
        local = t in (R.MsgHup, R.MsgBeat, MsgCheckQuorum)
        res = r.step(R.Message(type=t, frm=0 if local else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
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


# ---- Tick --------------------------------------------------------------------------------------------------------------------------
def _popcount(x):
    x = np.asarray(x, np.uint32)
    return sum(((x >> np.uint32(k)) & 1) for k in range(16)).astype(np.int64)


def tick_array(oracle, role, elapsed, active, lead_elapsed, voters, self_peer, n_peers, election_tick, heartbeat_tick, seed, tick_no):
    """oracle.tick (ref_tick_members.tick_array over masks), then the leader's check on top -> (elapsed' u32, action u8, active' u16,
    lead_elapsed' u32, n_hup, n_beat).  voters: the masks Tick reads (raftq_tick_set_voters on and masks loaded), or None."""
    role, elapsed = np.asarray(role), np.asarray(elapsed, np.uint32)
    active, lead_elapsed = np.asarray(active, np.uint16).astype(np.uint32), np.asarray(lead_elapsed, np.uint32)
    if voters is None:
        el, act, _, _ = oracle.tick(role, elapsed, election_tick, heartbeat_tick, seed, tick_no)
        members = np.full(len(role), (1 << n_peers) - 1, np.uint32)
    else:
        el, act, _, _ = TM.tick_array(oracle, role, elapsed, voters, self_peer, election_tick, heartbeat_tick, seed, tick_no)
        members = np.asarray(voters, np.uint16).astype(np.uint32)
    leads = role == LEADER
    le = lead_elapsed + np.uint32(1)
    due = leads & (le >= election_tick)
    n_act = _popcount((active | np.uint32(1 << self_peer)) & members)
    lost = due & (n_act < _popcount(members) // 2 + 1)
    act = np.where(lost, 3, act).astype(np.uint8)
    el = np.where(lost, elapsed + np.uint32(1), el).astype(np.uint32)  # no beat this tick: the heartbeat counter is not cleared
    active2 = np.where(due & ~lost, 0, active).astype(np.uint16)
    le2 = np.where(leads, np.where(due, 0, le), lead_elapsed).astype(np.uint32)
    return el, act, active2, le2, int((act == 1).sum()), int((act == 2).sum())


def tick_scalar(oracle, role, elapsed, active, lead_elapsed, voters, self_peer, n_peers, election_tick, heartbeat_tick, seed, tick_no):
    """group by group: tickElection for a non-leader exactly as ref_tick_members.tick_scalar states it; for a leader
        tickHeartbeat:  r.elapsed++; le++
                        if le >= electionTimeout { le = 0; act = |(active + self) & members|
                                                   if act >= q { active = {} } else { action 3, no beat, return } }
                        if r.elapsed >= r.heartbeatTimeout { r.elapsed = 0; r.Step(MsgBeat) }"""
    G = len(role)
    el = np.asarray(elapsed, np.uint32).copy()
    ac = np.asarray(active, np.uint16).copy()
    le = np.asarray(lead_elapsed, np.uint32).copy()
    act = np.zeros(G, np.uint8)
    for g in range(G):
        members = (1 << n_peers) - 1 if voters is None else int(voters[g])
        if int(role[g]) != LEADER:
            if not (members >> self_peer) & 1:
                el[g] = 0
                continue
            e = int(el[g]) + 1
            d = e - election_tick
            if d >= 0 and d > oracle.tick_rand(seed, tick_no, g) % election_tick:
                e, act[g] = 0, 1
            el[g] = e
            continue
        e = int(el[g]) + 1
        el[g] = e
        x = int(le[g]) + 1
        if x >= election_tick:
            le[g] = 0
            n_act = bin((int(ac[g]) | (1 << self_peer)) & members).count("1")
            if n_act < bin(members).count("1") // 2 + 1:
                act[g] = 3
                continue
            ac[g] = 0
        else:
            le[g] = x
        if e >= heartbeat_tick:
            el[g], act[g] = 0, 2
    return el, act, ac, le, int((act == 1).sum()), int((act == 2).sum())


def tick_input(g, n, self_peer, election_tick, seed, masks=False):
    """roles mixed (half leaders), elapsed and lead_elapsed spread so that timers and checks fall due on different ticks of the
    2 * election_tick the tests run, activity words from empty to full (so checks both pass and fail), and -- masks -- voter sets
    in which self does and does not vote, the empty one included -> (role, elapsed, active, lead_elapsed, voters | None)"""
    rng = np.random.default_rng(seed)
    role = rng.choice([0, 1, 2, 2], g).astype(np.uint8)
    elapsed = rng.integers(0, 2 * election_tick, g).astype(np.uint32)
    full = (1 << n) - 1
    active = np.where(rng.random(g) < 0.3, 0, np.where(rng.random(g) < 0.3, full, rng.integers(0, full + 1, g))).astype(np.uint16)
    lead_elapsed = rng.integers(0, election_tick, g).astype(np.uint32)
    voters = None
    if masks:
        voters = rng.integers(0, full + 1, g).astype(np.uint16)
        voters[rng.random(g) < 0.1] = 0
        voters[rng.random(g) < 0.2] = full
    return role, elapsed, active, lead_elapsed, voters


# ---- the Step inputs ---------------------------------------------------------------------------------------------------------------
G, N_MSGS = 194, 512  # (ref_step_props.props_state deals 60 led groups and 60 followers of a peer at this size)
OWN_KINDS = (MsgCheckQuorum, R.MsgVote)  # the kinds its rules decide: the check itself, and the vote the lease rule (3) ignores
SHAPES = ((1, 0), (3, 0), (5, 4), (9, 8))
PLANT = 6


def _rec(m, at, group, type, term=0, frm=0, index=0, log_term=0, reject=0):
    m[at] = np.zeros(1, m.dtype)[0]
    m["group"][at], m["type"][at], m["term"][at], m["from"][at] = group, type, term, frm
    m["index"][at], m["log_term"][at], m["reject"][at] = index, log_term, reject


def step_case(n, self_peer, seed, masks=False, hot=False, g=G, n_msgs=N_MSGS, band=None, plants=None):
    """one (start state, voters | None, active, lead_elapsed, batch, the reference's records, (state, active, lead_elapsed) after).
    ref_step_props.props_state's dealt roles with elapsed on both sides of election_tick and random activity words; its traffic with one record in
    seven turned into a MsgCheckQuorum; in front, per kind PLANT groups with one directed exchange each:
      led, every bit set        a check: passes, clears the bits
      led, no bit set           a check: fails (N > 1), steps down
      led, no bit set           q - 1 acknowledgements from distinct peers (one of them rejected), then a check: the acks save it
      led, every bit set        a MsgHeartbeat of the next term: reset() clears the bits
      led                       a MsgVote of the next term: in lease, ignored
      following, elapsed 0      a MsgVote of the next term: in lease, ignored
      following, elapsed past   the same: out of lease, answered
    `hot`: a led group with 40 acknowledgements and checks in a row (a run longer than the list walk takes).
    band: the state lifted by tests/_widegen first and the traffic drawn by its wide_batch; in
    b32 / b63 the three MsgVote sets stand at term B - 1, so that the vote "of the next term" is B: ignored in the lease (the term
    stays B - 1), granted past it (the term becomes B).  plants: a dict that is told these groups."""
    rng = np.random.default_rng(seed)
    s = P.props_state(rng, n, self_peer, g)
    if band is not None:
        s = WG.lift(s, band, rng)
    s.elapsed[:] = rng.integers(0, 2 * ELECTION_TICK, g)
    full = (1 << n) - 1
    active = rng.integers(0, full + 1, g).astype(np.uint16)
    lead_elapsed = rng.integers(0, ELECTION_TICK, g).astype(np.uint32)
    voters = None
    if masks:
        voters = rng.integers(0, full + 1, g).astype(np.uint16) | np.uint16(1 << self_peer)
    led = np.flatnonzero(s.role == 2)
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0))
    assert len(led) >= 5 * PLANT + 3 and len(fol) >= 2 * PLANT, (len(led), len(fol))
    sets = [led[k * PLANT:(k + 1) * PLANT] for k in range(5)]
    hot_group = int(led[5 * PLANT])
    if masks:  # a group whose voter set is empty, and one in which only a non-voter answers
        voters[led[5 * PLANT + 1]] = 0
        active[led[5 * PLANT + 1]] = full
        if n > 1:
            voters[led[5 * PLANT + 2]] = full & ~(1 << ((self_peer + 1) % n))
            active[led[5 * PLANT + 2]] = 1 << ((self_peer + 1) % n)
        voters[np.concatenate(sets)] = full
    active[sets[0]], active[sets[1]], active[sets[2]], active[sets[3]] = full, 0, 0, full
    in_lease, out_lease = fol[:PLANT], fol[PLANT:2 * PLANT]
    s.elapsed[in_lease], s.elapsed[out_lease] = 0, ELECTION_TICK + 3
    planted = np.concatenate(sets + [in_lease, out_lease, led[5 * PLANT:5 * PLANT + 3]])
    free = np.setdiff1d(np.arange(g), planted)
    if band is None:
        m = _stepgen.random_batch(rng, s, n_msgs)
    else:
        if WG.BANDS[band]:
            WG.set_term(s, np.concatenate([sets[4], in_lease, out_lease]), WG.BANDS[band] - 1)
        m = WG.wide_batch(rng, s, n_msgs)
    if plants is not None:
        plants.update(led=sets[4], in_lease=in_lease, out_lease=out_lease)
    others = [(self_peer + 1 + k) % n for k in range(n - 1)]
    at = 0
    for grp in sets[0]:
        _rec(m, at, grp, MsgCheckQuorum); at += 1
    for grp in sets[1]:
        _rec(m, at, grp, MsgCheckQuorum); at += 1
    for grp in sets[2]:
        for k, p in enumerate(others[:n // 2]):  # q - 1 = n / 2 more members
            _rec(m, at, grp, R.MsgAppResp if k % 2 == 0 else R.MsgHeartbeatResp, term=int(s.term[grp]), frm=p, index=int(s.last_index[grp]), reject=int(k == 0)); at += 1
        _rec(m, at, grp, MsgCheckQuorum); at += 1
    for grp in sets[3]:
        _rec(m, at, grp, R.MsgHeartbeat, term=int(s.term[grp]) + 1, frm=others[0] if others else 0); at += 1
    for grp in np.concatenate([sets[4], in_lease, out_lease]):
        _rec(m, at, grp, R.MsgVote, term=int(s.term[grp]) + 1, frm=others[-1] if others else 0, index=int(s.last_index[grp]) + 5, log_term=int(s.term[grp]) + 1); at += 1
    for grp in (led[5 * PLANT + 1], led[5 * PLANT + 2]):
        _rec(m, at, grp, MsgCheckQuorum); at += 1
    assert at < n_msgs // 2
    rest = np.arange(at, n_msgs)
    m["group"][rest] = rng.choice(free, len(rest))  # (the directed exchanges stay undisturbed)
    if hot:
        for j, i in enumerate(rest[:40]):
            if j % 5 == 4:
                _rec(m, i, hot_group, MsgCheckQuorum)
            else:
                _rec(m, i, hot_group, R.MsgAppResp, term=int(s.term[hot_group]), frm=int(rng.integers(0, n)), index=int(s.last_index[hot_group]), reject=int(rng.random() < 0.3))
        rest = rest[40:]
    for i in rest[rng.random(len(rest)) < 1 / 7]:
        _rec(m, i, int(m["group"][i]), MsgCheckQuorum, frm=int(rng.integers(0, 256)))  # (`from` is ignored on a local kind)
    start = (V.copy_state(s), active.copy(), lead_elapsed.copy())
    if band is not None:
        WG.guard_case(s, m)
    want = step_batch(s, voters, active, lead_elapsed, m)
    if band is not None:
        WG.guard_case(s, m)
    for a in (m, want):
        a.setflags(write=False)
    return start, voters, m, want, (s, active, lead_elapsed)


def state_differs(a, b):
    """two (NodeState, active, lead_elapsed) triples"""
    sa, sb = a[0], b[0]
    same = all(np.array_equal(getattr(sa, k), getattr(sb, k)) for k, _ in pyoracle.NodeState.FIELDS)
    same = same and np.array_equal(sa.match, sb.match) and np.array_equal(sa.votes, sb.votes)
    return not (same and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def outcomes(start, voters, m, want):
    """what the input shows of the feature, read off the reference's own output -> dict of counts"""
    s0, active0, _ = start
    chk = m["type"] == MsgCheckQuorum
    led_before = np.zeros(len(m), bool)
    role = {}
    for i in range(len(m)):  # the group's role in front of record i
        grp = int(m["group"][i])
        led_before[i] = role.get(grp, int(s0.role[grp])) == LEADER
        role[grp] = int(want["role"][i])
    down = (want["flags"] & R.FlagSteppedDown) != 0
    vote_up = (m["type"] == R.MsgVote) & (m["term"] > want["term"])  # a higher term that did not become the group's: ignored
    ack = np.isin(m["type"], (R.MsgAppResp, R.MsgHeartbeatResp)) & (want["type"] == R.OutProgress)
    new_bit = np.zeros(len(m), bool)
    seen = {}
    for i in np.flatnonzero(ack | (chk & led_before) | down):
        grp = int(m["group"][i])
        bits = seen.get(grp, int(active0[grp]))
        if ack[i]:
            new_bit[i] = not (bits >> int(m["from"][i])) & 1
            bits |= 1 << int(m["from"][i])
        else:
            bits = 0
        seen[grp] = bits
    return {"passing checks": int((chk & led_before & ~down).sum()), "failing checks": int((chk & led_before & down).sum()),
            "checks on a non-leader": int((chk & ~led_before).sum()), "lease-ignored votes": int((vote_up & (want["type"] == R.OutNone)).sum()),
            "acks that set a bit": int(new_bit.sum())}


def case_list():
    """the arguments of every step_case() the GPU tests step (tests/test_check_quorum_ref.py shows that each one discriminates)"""
    cases = []
    for n, me in SHAPES:
        cases.append(dict(n=n, self_peer=me, seed=9500 + n))
        cases.append(dict(n=n, self_peer=me, seed=9510 + n, masks=True))
    cases.append(dict(n=3, self_peer=1, seed=9520, hot=True))
    cases.append(dict(n=5, self_peer=0, seed=9521, hot=True, masks=True))
    for k, band in enumerate(WG.BAND_NAMES):  # appended: the positions above are what the GPU tests pick by
        cases.append(dict(n=3, self_peer=0, seed=9530 + k, band=band))
        cases.append(dict(n=9, self_peer=8, seed=9540 + k, masks=True, band=band))
    return cases


def case_id(c):
    return "n%d-self%d%s%s%s" % (c["n"], c["self_peer"], "-masks" if c.get("masks") else "", "-hot" if c.get("hot") else "",
                                 "-" + c["band"] if c.get("band") else "")
