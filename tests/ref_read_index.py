"""ReadIndex (include/raftq.h "ReadIndex", include/raftq_step.h "ReadIndex in Step"): tests/ref_lead_transfer's classes -- and
tests/ref_pre_vote's / tests/ref_check_quorum's for a handle without those switches, each with ref_step_props' MsgProp arms -- and the
Step rules of etcd/raft's ReadIndex on top.  Rule numbers are the header's; the ones Step itself runs can be left out:

  2  leader, MsgReadIndex: dropped behind a closed gate and at a full counter, else RAFTQ_OUT_READ_INDEX (numbered, or released at once)
  3  leader, MsgHeartbeatResp with a context: acked[p] = max(acked[p], c); a confirmed() that moved carries RAFTQ_OUTF_READ_READY
  4  reset() clears seq and every acked word
  5  leader, MsgBeat: the round carries the last pending request's number
  6  follower: MsgReadIndex forwarded, MsgHeartbeat echoed (the candidate's arm too), MsgReadIndexResp -> RAFTQ_OUT_READ_STATE

(1, 7, 8 and 9 are the records, the compact forms, the frames and the refusals: nothing of Step's to leave out.)

Also: a batch driver that takes and returns seq / acked, the generators of the GPU tests' inputs, a three-node cluster whose hosts
keep the read queue the header describes, and a second, independent model of upstream's readOnly (a queue of contexts, one
acknowledgement set per context, advance).
TEST INFRASTRUCTURE: nothing in the product imports it."""
from collections import Counter
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_lead_transfer as T
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

MsgReadIndex, MsgReadIndexResp = 15, 16
OutReadIndex, OutReadState = 18, 19
FlagReadReady = 0x40
SAFE, LEASE = 1, 2
SEQ_MAX = 2**32 - 1
ELECTION_TICK = Q.ELECTION_TICK
RULES = (2, 3, 4, 5, 6)
RULE_NAMES = {2: "leader_read", 3: "ack", 4: "reset", 5: "beat", 6: "follower"}
_BY_NAME = {v: k for k, v in RULE_NAMES.items()}


def rules(leave_out):
    return frozenset(_BY_NAME.get(x, x) for x in leave_out)


class _ReadArms:
    """the rules; `ri_out` (tests only): rule numbers this instance does NOT apply.  Without 2 the leader ignores the request; without
    3 a context is not looked at; without 4 the record survives reset(); without 5 a round carries no context; without 6 a follower
    ignores the two kinds and echoes nothing.  `arm_count` (a Counter, or None) is told which arm every message took."""
    ri_mode = 0
    ri_out = frozenset()
    seq = 0
    acked = None  # {raft ID: the largest sequence number it has acknowledged}
    arm_count = None

    def _arm(self, name):
        if self.arm_count is not None:
            self.arm_count[name] += 1

    def confirmed(self):
        """the q-th largest acknowledgement over the members (sorted form; the kernel counts)"""
        mem = self.members()
        vals = sorted((self.acked.get(p, 0) for p in mem), reverse=True)
        q = len(mem) // 2 + 1
        return vals[q - 1] if len(vals) >= q else 0

    def reset(self, term):
        super().reset(term)
        if self.ri_mode == SAFE and 4 not in self.ri_out:
            if self.seq or any(self.acked.values()):
                self._arm("4 cleared a record")
                self._cleared = True  # (this batch: told apart below)
            self.seq, self.acked = 0, {}

    def _step(self, m):
        # either read kind at a higher term: becomeFollower(m.Term, None), as for any kind that is not a leader's (a MsgReadIndex's
        # `from` is the requester, who leads nothing)
        if self.ri_mode and m.type in (MsgReadIndex, MsgReadIndexResp) and m.term > self.term:
            self.become_follower(m.term, R.NONE)
        return super()._step(m)

    def step_leader(self, m):
        mode, out = self.ri_mode, self.ri_out
        if mode and m.type == MsgReadIndexResp:
            self._arm("6 resp ignored by role")
            return R.Result()
        if mode and m.type == MsgReadIndex:
            if 2 in out:
                return R.Result()
            if self.first_index_of_term == 0 or self.committed < self.first_index_of_term:
                self._arm("2 gate closed")
                return R.Result()
            if mode == LEASE:
                self._arm("2 lease")
                return R.Result(OutReadIndex, index=self.committed, flags=FlagReadReady)
            if self.seq == SEQ_MAX:
                self._arm("2 counter full")
                return R.Result()
            self.seq += 1
            self.acked[self.id] = self.seq
            ready = self.confirmed() >= self.seq
            self._arm("2 ready at once" if ready else "2 taken")
            return R.Result(OutReadIndex, index=self.committed, log_term=self.seq, flags=FlagReadReady if ready else 0)
        res = super().step_leader(m)
        if mode == SAFE and m.type == R.MsgHeartbeatResp and 3 not in out:
            c = m.index
            if c == 0:
                self._arm("3 no context")
            elif c > self.seq:
                self._arm("3 beyond seq")
                if getattr(self, "_cleared", False):
                    self._arm("3 beyond seq after a reset")
            else:
                before = self.confirmed()
                if self.acked.get(m.frm, 0) < c:
                    self.acked[m.frm] = c
                    self._arm("3 raised a non-voter" if m.frm not in self.members() else "3 raised")
                else:
                    self._arm("3 duplicate or late")
                after = self.confirmed()
                if after > before:
                    self._arm("3 confirmed")
                    res.flags |= FlagReadReady
                    res.log_term = after
        if mode == SAFE and m.type == R.MsgBeat and 5 not in out and self.state == R.StateLeader:
            pending = self.seq > self.confirmed()
            self._arm("5 pending" if pending else "5 nothing pending")
            res.index = self.seq if pending else 0
        return res

    def step_candidate(self, m):
        if self.ri_mode and m.type in (MsgReadIndex, MsgReadIndexResp):
            self._arm("6 ignored by a candidate")
            return R.Result()
        res = super().step_candidate(m)
        if self.ri_mode and m.type == R.MsgHeartbeat and 6 not in self.ri_out:
            self._arm("6 echo, candidate")
            res.index = m.index
        return res

    def step_follower(self, m):
        mode, out = self.ri_mode, self.ri_out
        if mode and m.type == MsgReadIndex:
            if 6 in out or self.lead == R.NONE:
                self._arm("6 no leader")
                return R.Result()
            self._arm("6 forwarded")
            return R.Result(P.OutForward)
        if mode and m.type == MsgReadIndexResp:
            if 6 in out:
                return R.Result()
            self._arm("6 read state")
            return R.Result(OutReadState, index=m.index)
        res = super().step_follower(m)
        if mode and m.type == R.MsgHeartbeat and 6 not in out:
            self._arm("6 echo")
            res.index = m.index
        return res


@dataclass
class NPRaft(PV.PRaft, P.PRaft):  # PreVote without leadership transfer
    pass


@dataclass
class NPVRaft(PV.PVRaft, P.PVRaft):
    pass


@dataclass
class NCRaft(Q.CRaft, P.PRaft):  # CheckQuorum alone
    pass


@dataclass
class NCVRaft(Q.CVRaft, P.PVRaft):
    pass


def _with_read_arms(base):
    return dataclass(type("R" + base.__name__, (_ReadArms, base), {}))


_CLASSES = {(pv, lt): tuple(_with_read_arms(b) for b in pair)
            for (pv, lt), pair in {(True, True): (T.TPRaft, T.TPVRaft), (False, True): (T.TCRaft, T.TCVRaft),
                                   (True, False): (NPRaft, NPVRaft), (False, False): (NCRaft, NCVRaft)}.items()}
LOCAL = (R.MsgHup, R.MsgBeat, Q.MsgCheckQuorum)


@dataclass
class Extra:
    """what a handle holds beside the node state: the activity word's three parts and the read records"""
    active: np.ndarray
    lead_elapsed: np.ndarray
    transferee: np.ndarray
    seq: np.ndarray    # [G] u32
    acked: np.ndarray  # [N][G] u32

    def copy(self):
        return Extra(*(a.copy() for a in (self.active, self.lead_elapsed, self.transferee, self.seq, self.acked)))

    def parts(self):
        return self.active, self.lead_elapsed, self.transferee, self.seq, self.acked


def zero_extra(g, n):
    return Extra(np.zeros(g, np.uint16), np.zeros(g, np.uint32), np.zeros(g, np.uint8), np.zeros(g, np.uint32), np.zeros((n, g), np.uint32))


def confirmed_of(x, voters, n):
    """confirmed(g) of every group, off the arrays (what raftq_read_reads gives)"""
    g = len(x.seq)
    out = np.zeros(g, np.uint32)
    for grp in range(g):
        mem = [p for p in range(n) if voters is None or (int(voters[grp]) >> p) & 1]
        vals = sorted((int(x.acked[p, grp]) for p in mem), reverse=True)
        q = len(mem) // 2 + 1
        out[grp] = vals[q - 1] if len(vals) >= q else 0
    return out


def step_batch(s, voters, x, msgs, mode=SAFE, pre_vote=True, lead_transfer=True, election_tick=ELECTION_TICK, leave_out=frozenset(), frames=False,
               arm_count=None, lt_leave_out=frozenset(), pv_leave_out=frozenset()):
    """Step for every message, in order, with raftq_set_check_quorum, raftq_step_set_props and raftq_set_read_index(mode) on (and
    raftq_set_pre_vote / raftq_set_lead_transfer as said) -> raftq_step_out_t[]; `s` and the Extra `x` move.  voters: the masks, or
    None for a handle without them.  leave_out: this module's rule numbers or names; lt_leave_out / pv_leave_out: ref_lead_transfer's
    and ref_pre_vote's, for the classes that hold those arms."""
    out = np.zeros(len(msgs), dtype=pyoracle.STEP_OUT_DT)
    rafts = {}
    ri_out, lt_out, pv_out = rules(leave_out), T.rules(lt_leave_out), frozenset(pv_leave_out)
    assert (lead_transfer or not lt_out) and (pre_vote or not pv_out), "a rule of a switch that is off cannot be left out"
    n = s.N
    for i in range(len(msgs)):
        m = msgs[i]
        fl = int(m["_pad"][1])
        if fl & V.MSGF_SKIP:
            out[i]["type"] = V.OutSkipped
            continue
        g = int(m["group"])
        r = rafts.get(g)
        if r is None:
            r = rafts[g] = Q.from_node_state(s, g, None if voters is None else voters[g], x.active[g], x.lead_elapsed[g], election_tick,
                                             classes=_CLASSES[(bool(pre_vote), bool(lead_transfer))])
            r.transferee = int(x.transferee[g])
            r.ri_mode, r.ri_out, r.arm_count = mode, ri_out, arm_count
            if lt_out:
                r.lt_out = lt_out
            if pv_out:
                r.pv_out = pv_out
            r.seq = int(x.seq[g])
            r.acked = {p + 1: int(x.acked[p, g]) for p in range(n) if x.acked[p, g]}
            r.held = False
        if fl & V.MSGF_HOLD:
            r.held = True
            V._common(out[i], r, m)
            out[i]["type"] = V.OutHeld
            continue
        t = int(m["type"])
        k = P.entry_count(m, frames)
        ent_term = 0 if t == P.MsgProp else int(m["reject_hint"])
        res = r.step(R.Message(type=t, frm=0 if t in LOCAL else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
                               index=int(m["index"]), commit=int(m["commit"]), reject=bool(m["reject"]),
                               entries=(ent_term,) * k if fl & V.MSGF_ENTRIES else None, barrier=bool(fl & V.MSGF_BARRIER)))
        V._common(out[i], r, m)
        if res.type == P.OutForward:
            out[i]["to"] = r.lead - 1
        out[i]["type"], out[i]["index"], out[i]["log_term"], out[i]["reject"], out[i]["flags"] = res.type, res.index, res.log_term, res.reject, res.flags
    for g, r in rafts.items():
        V.to_node_state(r, s, g)
        x.active[g] = sum(1 << (p - 1) for p in r.active)
        x.lead_elapsed[g] = r.lead_elapsed
        x.transferee[g] = r.transferee
        x.seq[g] = r.seq
        for p in range(n):
            x.acked[p, g] = r.acked.get(p + 1, 0)
    return out


# ---- upstream's readOnly, restated on its own ----------------------------------------------------------------------------------------
class ReadOnly:
    """etcd/raft's read_only.go: pendingReadIndex (context -> {index, acks}), readIndexQueue, addRequest / recvAck / advance /
    lastPendingRequestCtx.  Nothing here knows of sequence numbers: a context is an opaque key."""

    def __init__(self):
        self.pending = {}
        self.queue = []

    def add_request(self, index, ctx, self_id):
        if ctx in self.pending:
            return
        self.pending[ctx] = (index, {self_id})
        self.queue.append(ctx)

    def recv_ack(self, frm, ctx):
        """-> the acknowledgement set of ctx, or None if nobody waits for it"""
        st = self.pending.get(ctx)
        if st is None:
            return None
        st[1].add(frm)
        return st[1]

    def advance(self, ctx):
        """every request up to and including ctx leaves the queue -> their (ctx, index), in order"""
        if ctx not in self.queue:
            return []
        at = self.queue.index(ctx)
        done, self.queue = self.queue[:at + 1], self.queue[at + 1:]
        return [(c, self.pending.pop(c)[0]) for c in done]

    def last_pending(self):
        return self.queue[-1] if self.queue else None


# ---- the Step inputs ---------------------------------------------------------------------------------------------------------------
G, N_MSGS = 194, 512
SHAPES = T.SHAPES  # N in {3, 5, 9}, self in the first and in the last slot
PLANT = 4
ARM_FLOOR = 4


def _rec(m, at, group, type, term=0, frm=0, index=0, log_term=0, reject=0, flags=0):
    PV._rec(m, at, group, type, term, frm, index, log_term, reject, flags)


def step_case(n, self_peer, seed, mode=SAFE, masks=False, pre_vote=True, lead_transfer=True, hot=False, g=G, n_msgs=N_MSGS, band=None, plants=None):
    """one (start = (state, Extra), voters | None, batch, the reference's records, (state, Extra) after).
    ref_step_props.props_state's dealt roles over g groups, led groups with a read record (seq up to 5, every acked word <= seq), and
    _stepgen's traffic in which every MsgHeartbeat / MsgHeartbeatResp carries a small context and one record in five is turned into
    a MsgReadIndex or MsgReadIndexResp.  In front, PLANT groups per arm with one directed exchange each (`others` = the peers in
    slot order behind self, `last` the highest slot that is not self):
      led, gate open            a local and a forwarded MsgReadIndex, the acknowledgements of the SECOND round from one peer after
                                the other until a quorum stands (both released by one flag), a duplicate, a late one of round 1,
                                a MsgBeat (nothing pending)
      led, gate open            MsgReadIndex, MsgBeat: the round is resent with its number
      led, gate closed          first_idx 0, or committed behind it: the request is dropped
      led, seq = 2^32 - 2       one request is taken, the next is dropped
      led                       MsgReadIndex, a MsgApp of the next term (reset() clears the record), a late acknowledgement of the old
                                term (stale), then MsgHup and the grants that make the node leader again two terms up, and an
                                acknowledgement of round 1 at that term: it finds c > seq on the cleared record
      led, pending              MsgCheckQuorum with every bit set (the record stays) / with none (a step-down clears it)
      led, seq 3                acknowledgements of 5 and of 0: no context
      led, every acked word distinct   an acknowledgement that moves confirmed() by one selection slot
      led                       MsgReadIndexResp: ignored
      following                 MsgReadIndex at term 0 and at the own term (forwarded), a MsgHeartbeat with a context (echoed)
      following                 MsgReadIndexResp of the own term, of the next (follows nobody, then the read state), of the one before (ignored)
      following nobody          MsgReadIndex: RAFTQ_OUT_NONE
      candidate                 MsgReadIndex and MsgReadIndexResp (ignored), a MsgHeartbeat with a context (becomes a follower, echoes)
    masks: the planted groups vote in full, but for PLANT led groups in which self is the ONE voter (released at once; then a MsgApp
    of the next term, a MsgHup that wins on its own grant, and an acknowledgement that finds c > seq on the fresh record) and PLANT
    led groups whose `last` is no voter (its acknowledgement is stored and does not count).
    `hot`: a led group with 40 records in a row -- three requests and their acknowledgements out of order, with a duplicate.
    band: the state lifted by tests/_widegen first and the traffic drawn by its wide_batch, one
    heartbeat context in eight moved up by 2^32, a MsgReadIndexResp's index around the group's tail.  The plants above, changed:
      led, gate open            (the first two sets) committed = tail - 1; first_idx == committed in one half, == committed - 2^32 in
                                the other (b32: the tail raised to 2^32 + 2 for it)
      led, gate closed          the last group's first_idx == committed + 2^32 (not under "top": it would pass the guard)
      led, seq 3                three more acknowledgements, of 2^32 + 1, 2^32 and 2^63 + 2: beyond seq, nothing stored or released
      following, candidate      the MsgHeartbeat's context is 2^32 + 7: echoed whole
      following                 the MsgReadIndexResp's index is the lifted committed (or, where that is below 2^32, the band's edge + k)
    plants: a dict that is told these groups."""
    rng = np.random.default_rng(seed)
    s = P.props_state(rng, n, self_peer, g)
    if band is not None:
        s = WG.lift(s, band, rng)
    s.elapsed[:] = rng.integers(0, 2 * ELECTION_TICK, g)
    if pre_vote:
        cand = np.flatnonzero(s.role == 1)
        s.role[cand[::3]] = PV.PRE
    full = (1 << n) - 1
    others = [(self_peer + 1 + k) % n for k in range(n - 1)]
    last, other = max(others), min(others)
    q = n // 2 + 1
    x = zero_extra(g, n)
    x.active[:] = rng.integers(0, full + 1, g)
    x.lead_elapsed[:] = rng.integers(0, ELECTION_TICK, g)
    led = np.flatnonzero(s.role == 2)
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0))
    lost = np.flatnonzero((s.role == 0) & (s.lead == 0))
    cnd = np.flatnonzero(s.role == 1)
    if mode == SAFE:
        x.seq[led] = rng.integers(0, 6, len(led))
        x.acked[:, led] = (rng.random((n, len(led))) * (x.seq[led] + 1)[None, :]).astype(np.uint32)
    voters = None
    if masks:
        voters = rng.integers(0, full + 1, g).astype(np.uint16)
        voters[rng.random(g) < 0.75] |= np.uint16(1 << self_peer)
    n_led_sets = 11 + (2 if masks else 0)
    assert len(led) >= n_led_sets * PLANT + 1 and len(fol) >= 2 * PLANT and len(lost) >= PLANT and len(cnd) >= PLANT, (len(led), len(fol), len(lost), len(cnd))
    L = [led[k * PLANT:(k + 1) * PLANT] for k in range(n_led_sets)]
    quorum, resend, closed, fullc, rst, chk_pass, chk_fail, beyond, distinct, led_resp, spare = L[:11]
    hot_group = int(led[n_led_sets * PLANT])
    one_voter, non_voter = (L[11], L[12]) if masks else (led[:0], led[:0])
    fwd, rstate = fol[:PLANT], fol[PLANT:2 * PLANT]
    lost_p, cnd_p = lost[:PLANT], cnd[:PLANT]
    planted = np.concatenate([np.concatenate(L), [hot_group], fwd, rstate, lost_p, cnd_p])
    assert len(np.unique(planted)) == len(planted)
    if masks:
        voters[planted] = full
        voters[one_voter] = 1 << self_peer
        voters[non_voter] = full & ~(1 << last)
    # the led plants: the gate open (an entry of the term committed), the record empty
    opened = np.concatenate([quorum, resend, fullc, rst, chk_pass, chk_fail, beyond, distinct, led_resp, spare, [hot_group], one_voter, non_voter])
    s.first_idx[opened] = 1
    s.committed[opened] = np.maximum(s.committed[opened], 1)
    x.seq[opened], x.acked[:, opened] = 0, 0
    s.first_idx[closed[::2]] = 0
    s.first_idx[closed[1::2]] = s.committed[closed[1::2]] + np.uint64(1)
    if mode == SAFE:
        x.seq[fullc] = SEQ_MAX - 1
        x.acked[:, fullc] = SEQ_MAX - 1
        x.seq[beyond], x.acked[self_peer, beyond] = 3, 3
        x.seq[distinct] = 20
        x.acked[:, distinct] = (2 * (1 + rng.permutation(n)))[:, None]  # every word another, every selection slot live
        x.acked[self_peer, distinct] = 20
    x.active[chk_pass], x.active[chk_fail] = full, 0
    s.term[rstate] = np.maximum(s.term[rstate], 2)
    s.last_term[rstate] = np.minimum(s.last_term[rstate], s.term[rstate])
    free = np.setdiff1d(np.arange(g), planted)
    ctx = lambda small: small if band is None else 2**32 + 7  # noqa: E731
    read_at = {int(grp): 11 + k for k, grp in enumerate(rstate)}
    if band is None:
        m = _stepgen.random_batch(rng, s, n_msgs)
    else:
        H = PLANT // 2
        same, apart = np.concatenate([quorum[:H], resend[:H]]), np.concatenate([quorum[H:], resend[H:]])
        s.last_index[apart] = np.maximum(s.last_index[apart], np.uint64(2**32 + 2))
        s.match[self_peer, apart] = s.last_index[apart]
        both = np.concatenate([same, apart])
        s.committed[both] = s.last_index[both] - np.uint64(1)
        s.first_idx[same], s.first_idx[apart] = s.committed[same], s.committed[apart] - np.uint64(2**32)
        if band != "top":
            s.first_idx[closed[-1]] = s.committed[closed[-1]] + np.uint64(2**32)
        read_at = {int(grp): int(s.committed[grp]) if s.committed[grp] >= 2**32 else WG.band_edge(band) + k for k, grp in enumerate(rstate)}
        m = WG.wide_batch(rng, s, n_msgs)
        if plants is not None:
            plants.update(same=same, apart=apart, closed=closed, beyond=beyond, fwd=fwd, cnd=cnd_p, rstate=rstate, read_at=read_at)
    at = 0

    def put(*a, **kw):
        nonlocal at
        _rec(m, at, *a, **kw)
        at += 1

    for grp in quorum:
        t = int(s.term[grp])
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, MsgReadIndex, term=t, frm=other)
        for p in others[:q - 1]:
            put(grp, R.MsgHeartbeatResp, term=t, frm=p, index=2)
        put(grp, R.MsgHeartbeatResp, term=t, frm=others[0], index=2)
        put(grp, R.MsgHeartbeatResp, term=t, frm=others[-1], index=1)
        put(grp, R.MsgBeat)
    for grp in resend:
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, R.MsgBeat)
    for grp in closed:
        put(grp, MsgReadIndex, frm=self_peer)
    for grp in fullc:
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, MsgReadIndex, frm=other)
    for grp in rst:
        t = int(s.term[grp])
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, R.MsgApp, term=t + 1, frm=other, index=int(s.last_index[grp]) + 9, log_term=t + 1)
        put(grp, R.MsgHeartbeatResp, term=t, frm=last, index=1)
        put(grp, R.MsgHup)
        if pre_vote:
            for p in others[:q - 1]:
                put(grp, PV.MsgPreVoteResp, term=t + 2, frm=p)
        for p in others[:q - 1]:
            put(grp, R.MsgVoteResp, term=t + 2, frm=p)
        put(grp, R.MsgHeartbeatResp, term=t + 2, frm=last, index=1)
    for grp in np.concatenate([chk_pass, chk_fail]):
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, Q.MsgCheckQuorum)
    for grp in beyond:
        t = int(s.term[grp])
        put(grp, R.MsgHeartbeatResp, term=t, frm=other, index=5)
        put(grp, R.MsgHeartbeatResp, term=t, frm=other, index=0)
        if band is not None:
            for c in (2**32 + 1, 2**32, 2**63 + 2):
                put(grp, R.MsgHeartbeatResp, term=t, frm=last, index=c)
    for grp in distinct:
        t = int(s.term[grp])
        put(grp, R.MsgHeartbeatResp, term=t, frm=last, index=19)
        put(grp, R.MsgHeartbeatResp, term=t, frm=other, index=7)
    for grp in led_resp:
        put(grp, MsgReadIndexResp, term=int(s.term[grp]), frm=other, index=4)
    for grp in one_voter:
        t = int(s.term[grp])
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, R.MsgApp, term=t + 1, frm=other, index=int(s.last_index[grp]) + 9, log_term=t + 1)
        put(grp, R.MsgHup)
        put(grp, R.MsgHeartbeatResp, term=t + 2, frm=other, index=1)
    for grp in non_voter:
        t = int(s.term[grp])
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, R.MsgHeartbeatResp, term=t, frm=last, index=1)
        for p in [p for p in others if p != last][:(n - 1) // 2]:
            put(grp, R.MsgHeartbeatResp, term=t, frm=p, index=1)
    for k, grp in enumerate(fwd):
        t = int(s.term[grp])
        put(grp, MsgReadIndex, term=t if k % 2 else 0, frm=self_peer if k < 2 else other)
        put(grp, R.MsgHeartbeat, term=t, frm=int(s.lead[grp]) - 1, index=ctx(7 + k))
    for k, grp in enumerate(rstate):
        t = int(s.term[grp])
        put(grp, MsgReadIndexResp, term=t - 1, frm=other, index=9)
        put(grp, MsgReadIndexResp, term=t + (k % 2), frm=int(s.lead[grp]) - 1, index=read_at[int(grp)])
    for grp in lost_p:
        put(grp, MsgReadIndex, frm=self_peer)
    for grp in cnd_p:
        t = int(s.term[grp])
        put(grp, MsgReadIndex, frm=self_peer)
        put(grp, MsgReadIndexResp, term=t, frm=other, index=3)
        put(grp, R.MsgHeartbeat, term=t, frm=other, index=ctx(5))
    assert at < n_msgs * 3 // 5, at
    rest = np.arange(at, n_msgs)
    m["group"][rest] = rng.choice(free, len(rest))  # (the directed exchanges stay undisturbed)
    if hot:
        t0 = int(s.term[hot_group])
        script = [(MsgReadIndex, self_peer, 0), (MsgReadIndex, other, 0), (R.MsgHeartbeatResp, others[-1], 2), (MsgReadIndex, self_peer, 0),
                  (R.MsgHeartbeatResp, others[0], 1), (R.MsgHeartbeatResp, others[0], 3), (R.MsgHeartbeatResp, others[0], 3), (R.MsgBeat, 0, 0)]
        for j, i in enumerate(rest[:40]):
            if j < len(script):
                kind, frm, c = script[j]
            else:  # acknowledgements of every round handed out so far and of one beyond, from every peer, in any order
                kind, frm, c = R.MsgHeartbeatResp, int(rng.choice(others)), int(rng.integers(0, 5))
            _rec(m, i, hot_group, kind, term=0 if kind in (R.MsgBeat,) or (kind == MsgReadIndex and frm == self_peer) else t0, frm=frm, index=c)
        rest = rest[40:]
    beats = rest[np.isin(m["type"][rest], (R.MsgHeartbeat, R.MsgHeartbeatResp))]
    m["index"][beats] = rng.integers(0, 7, len(beats))
    if band is not None:
        m["index"][beats] += np.where(rng.random(len(beats)) < 0.125, np.uint64(2**32), np.uint64(0))
    for i in rest[rng.random(len(rest)) < 0.2]:
        grp = int(m["group"][i])
        kind = MsgReadIndex if rng.random() < 0.6 else MsgReadIndexResp
        term = 0 if kind == MsgReadIndex and rng.random() < 0.5 else max(1, int(s.term[grp]) + int(rng.choice([-1, 0, 0, 0, 1])))
        frm = int(rng.integers(0, n))
        index = int(rng.integers(0, 50)) if band is None else int(WG.around(rng, s.last_index[grp:grp + 1], -3, 4, 1)[0])
        _rec(m, i, grp, kind, term=term, frm=frm, index=index)
    if lead_transfer:
        for i in rest[rng.random(len(rest)) < 0.04]:
            _rec(m, i, int(m["group"][i]), T.MsgTransferLeader if rng.random() < 0.5 else T.MsgTimeoutNow, term=int(s.term[int(m["group"][i])]), frm=int(rng.integers(0, n)))
    for i in rest[rng.random(len(rest)) < 0.05]:
        P._prop(m, i, int(m["group"][i]), int(rng.integers(1, 4)), frm=int(rng.integers(0, n)))
        m["_pad"][i] = (0, V.MSGF_ENTRIES)
    start = (V.copy_state(s), x.copy())
    if band is not None:
        WG.guard_case(s, m)
    want = step_batch(s, voters, x, m, mode, pre_vote, lead_transfer)
    if band is not None:
        WG.guard_case(s, m)
    for a in (m, want):
        a.setflags(write=False)
    return start, voters, m, want, (s, x)


def case_list():
    """the arguments of every step_case() the GPU tests step (tests/test_read_index_ref.py shows that each one discriminates)"""
    cases = []
    for k, (n, me) in enumerate(SHAPES):
        for masks in (False, True):
            # PreVote and leadership transfer on and off, dealt over the shapes: every pair occurs with and without masks
            pv, lt = bool((k + masks) & 1), bool((k >> 1) & 1) != masks
            cases.append(dict(n=n, self_peer=me, seed=11500 + 2 * k + masks, masks=masks, pre_vote=pv, lead_transfer=lt))
    cases.append(dict(n=5, self_peer=0, seed=11520, mode=LEASE))
    cases.append(dict(n=9, self_peer=8, seed=11521, mode=LEASE, masks=True, pre_vote=False, lead_transfer=False))
    cases.append(dict(n=3, self_peer=1, seed=11530, hot=True))
    cases.append(dict(n=9, self_peer=0, seed=11531, hot=True, masks=True, pre_vote=False))
    for k, band in enumerate(WG.BAND_NAMES):  # appended: the positions above are what the GPU tests pick by
        cases.append(dict(n=3, self_peer=0, seed=11540 + k, pre_vote=bool(k & 1), lead_transfer=k != 1, band=band))
        cases.append(dict(n=9, self_peer=8, seed=11550 + k, masks=True, pre_vote=not k & 1, lead_transfer=k != 2, band=band))
    cases.append(dict(n=5, self_peer=4, seed=11560, mode=LEASE, band="b63"))
    cases.append(dict(n=5, self_peer=0, seed=11561, hot=True, pre_vote=False, band="b32"))
    return cases


def case_id(c):
    return "n%d-self%d-%s%s%s%s%s" % (c["n"], c["self_peer"], "lease" if c.get("mode", SAFE) == LEASE else "safe", "-masks" if c.get("masks") else "",
                                     "-pv" if c.get("pre_vote", True) else "", "-lt" if c.get("lead_transfer", True) else "", "-hot" if c.get("hot") else "") + ("-" + c["band"] if c.get("band") else "")


def case_switches(c):
    return dict(mode=c.get("mode", SAFE), pre_vote=c.get("pre_vote", True), lead_transfer=c.get("lead_transfer", True))


def case_rules(c):
    """the rules a case is held to discriminate: the lease mode keeps no record, so 3, 4 and 5 have nothing to change there"""
    return (2, 6) if c.get("mode", SAFE) == LEASE else RULES


def copy_start(t):
    return V.copy_state(t[0]), t[1].copy()


def changed_records(start, voters, m, want, after, rule, **switches):
    """the records whose result, or whose group's final state, is another when `rule` is left out -> their batch positions"""
    st = copy_start(start)
    without = step_batch(st[0], voters, st[1], np.array(m), leave_out={rule}, **switches)
    k = want.dtype.itemsize
    differs = (without.view(np.uint8).reshape(-1, k) != np.array(want).view(np.uint8).reshape(-1, k)).any(axis=1)
    sa, sb = st[0], after[0]
    moved = np.zeros(sa.G, bool)
    for name, _ in pyoracle.NodeState.FIELDS:
        moved |= getattr(sa, name) != getattr(sb, name)
    moved |= (sa.match != sb.match).any(axis=0) | (sa.votes != sb.votes).any(axis=0)
    for a, b in zip(st[1].parts(), after[1].parts()):
        moved |= (a != b) if a.ndim == 1 else (a != b).any(axis=0)
    return np.flatnonzero(differs | moved[m["group"].astype(np.int64)])


def arms(start, voters, m, **switches):
    """which arm every record took, counted by the reference itself -> Counter"""
    st = copy_start(start)
    c = Counter()
    step_batch(st[0], voters, st[1], np.array(m), arm_count=c, **switches)
    return c


def arm_floors(c):
    """the arms a case must hold at least ARM_FLOOR times, by its arguments"""
    both = ["6 forwarded", "6 no leader", "6 echo", "6 echo, candidate", "6 read state", "6 ignored by a candidate", "6 resp ignored by role", "2 gate closed"]
    if c.get("mode", SAFE) == LEASE:
        return both + ["2 lease"]
    safe = both + ["2 taken", "2 counter full", "3 raised", "3 confirmed", "3 duplicate or late", "3 beyond seq", "3 beyond seq after a reset", "3 no context",
                   "4 cleared a record",
                   "5 pending", "5 nothing pending"]
    if c.get("masks"):
        safe += ["2 ready at once", "3 raised a non-voter"]
    return safe


# ---- three nodes, scripted ---------------------------------------------------------------------------------------------------------
_ROUND_KINDS = (R.OutBcastHeartbeat, R.OutCampaign, PV.OutPreCampaign)
_REPLY_KINDS = (R.OutHeartbeatResp, R.OutVoteResp, PV.OutPreVoteResp, PV.OutTermResp)


class Cluster(T.Cluster):
    """ref_lead_transfer.Cluster whose nodes run the read rules, and whose hosts do what INTEGRATION.md asks of a caller: per group
    a queue of (seq, index, from) for every RAFTQ_OUT_READ_INDEX that came without the flag, a MsgHeartbeat{Index: seq} round for
    it, a release -- local into `released`, or as MsgReadIndexResp to the follower that forwarded -- on RAFTQ_OUTF_READ_READY, the
    echo of a heartbeat's context, and the queue dropped when the node stops leading.  `released[k]`: (group, index) of every read
    node k asked for that came back good, in order.  lose(k, p, msg) -> True drops a message from k to p (the tests' seam)."""

    def __init__(self, g, pre_vote, mode=SAFE, lead_transfer=True, ri_leave_out=frozenset(), **kw):
        super().__init__(g, pre_vote, **kw)
        self.mode, self.lead_transfer, self.ri_leave_out = mode, lead_transfer, rules(ri_leave_out)
        self.x = [Extra(self.active[k], self.lead_elapsed[k], self.transferee[k], np.zeros(g, np.uint32), np.zeros((self.N, g), np.uint32))
                  for k in range(self.N)]
        self.queue = [dict() for _ in range(self.N)]  # group -> [(seq, index, from)]
        self.released = [[] for _ in range(self.N)]
        self.lose = None

    def _step(self, s, active, lead_elapsed, msgs):
        k = next(i for i in range(self.N) if self.s[i] is s)
        return step_batch(s, None, self.x[k], msgs, self.mode, self.pre_vote, self.lead_transfer, self.et, self.ri_leave_out)

    def _route(self, k, outs, batch):
        per = T.route(k, outs, batch, self.N)
        base = PV.route(k, outs, self.N)
        for p, a in per.items():  # the contexts: a round's from the leader's result, an echo's from the follower's
            j = 0
            for o in outs:
                t = int(o["type"])
                if t in _ROUND_KINDS or (t in _REPLY_KINDS and int(o["to"]) == p):
                    if t in (R.OutBcastHeartbeat, R.OutHeartbeatResp):
                        a["index"][j] = int(o["index"])
                    j += 1
            assert j == len(base[p])
        extra = {p: [] for p in per}

        def send(p, **kw):
            one = np.zeros(1, pyoracle.STEP_MSG_DT)
            _rec(one, 0, **kw)
            extra[p].append(one)

        def release(grp, index, frm, term):
            if frm == k:
                self.released[k].append((grp, index))
            else:
                send(frm, group=grp, type=MsgReadIndexResp, term=term, frm=k, index=index)

        for o, b in zip(outs, batch):
            t, grp, fl, term = int(o["type"]), int(o["group"]), int(o["flags"]), int(o["term"])
            if int(o["role"]) != 2:
                self.queue[k].pop(grp, None)  # the caller drops its queue when it stops leading
            if t == OutReadIndex:
                if fl & FlagReadReady:
                    release(grp, int(o["index"]), int(o["to"]), term)
                else:
                    self.queue[k].setdefault(grp, []).append((int(o["log_term"]), int(o["index"]), int(o["to"])))
                    for p in per:
                        send(p, group=grp, type=R.MsgHeartbeat, term=term, frm=k, index=int(o["log_term"]))
            elif t == R.OutProgress and fl & FlagReadReady:
                qd = self.queue[k].get(grp, [])
                for sq, index, frm in [e for e in qd if e[0] <= int(o["log_term"])]:
                    release(grp, index, frm, term)
                self.queue[k][grp] = [e for e in qd if e[0] > int(o["log_term"])]
            elif t == OutReadState:
                self.released[k].append((grp, int(o["index"])))
        return {p: np.concatenate([per[p]] + extra[p]) for p in per}

    def turn(self, k):
        s = self.s[k]
        el, act, ac, le, tr, _, _ = T.tick(pyoracle, s.role, s.elapsed, self.active[k], self.lead_elapsed[k], self.transferee[k], None, k, self.N,
                                           self.et, self.ht, self.seed + k, self.tick_no[k])
        self.tick_no[k] += 1
        s.elapsed[:], self.active[k][:], self.lead_elapsed[k][:], self.transferee[k][:] = el, ac, le, tr
        if self.on_tick:
            self.on_tick(k, act)
        local = np.zeros(int((act != 0).sum()), pyoracle.STEP_MSG_DT)
        at = 0
        for a, t in ((1, R.MsgHup), (2, R.MsgBeat), (3, Q.MsgCheckQuorum)):
            for grp in np.flatnonzero(act == a):
                _rec(local, at, int(grp), t)
                at += 1
        batch = np.concatenate([self.inbox[k], local])
        self.inbox[k] = np.zeros(0, pyoracle.STEP_MSG_DT)
        if len(batch) == 0:
            return
        outs = self._step(s, self.active[k], self.lead_elapsed[k], batch)
        self.log.append((k, batch, outs))
        if self.on_step:
            self.on_step(k, batch, outs)
        routed = self._route(k, outs, batch)  # (the host's queue moves whether or not the wire is cut)
        if k in self.cut:
            return
        for p, msgs in routed.items():
            if p in self.cut or not len(msgs):
                continue
            if self.lose is not None:
                msgs = msgs[[not self.lose(k, p, one) for one in msgs]]
            self.inbox[p] = np.concatenate([self.inbox[p], msgs])


def read_msgs(groups, frm):
    """one local MsgReadIndex per group (what node.ReadIndex steps)"""
    a = np.zeros(len(groups), pyoracle.STEP_MSG_DT)
    for i, grp in enumerate(groups):
        _rec(a, i, int(grp), MsgReadIndex, frm=frm)
    return a
