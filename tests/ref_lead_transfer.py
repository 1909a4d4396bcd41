"""Leadership transfer (include/raftq.h "Leadership transfer", include/raftq_step.h "Leadership transfer"): tests/ref_pre_vote.PRaft /
PVRaft -- and tests/ref_check_quorum.CRaft / CVRaft for a handle without PreVote --, each with ref_step_props' MsgProp arms, and
the Step rules of etcd/raft's leadTransferee on top.  Rule numbers are the header's:

  3  the lease ignores a MsgVote of a higher term only if it is not marked (reject == 0)
  4  leader, MsgTransferLeader: ignored / aborts / cancels / sets leadTransferee and lead_elapsed = 0 -> RAFTQ_OUT_TRANSFER
  5  leader, the pending transferee's updating MsgAppResp that reaches the tail carries RAFTQ_OUTF_TIMEOUT_NOW
  6  leader, MsgProp with a transfer pending is dropped
  7  reset() and MsgCheckQuorum clear the transferee
  8  follower, MsgTransferLeader: forwarded to the leader
  9  follower, MsgTimeoutNow: campaigns at once if promotable(), with the votes marked

Also: a batch driver in the shape of ref_pre_vote.step_batch that takes and returns the transferee array, the Tick composed of
ref_check_quorum's over the packed low half of the word, the generators of the GPU tests' inputs, and ref_pre_vote's three-node
cluster extended by the transfer's messages.
TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

MsgTransferLeader, MsgTimeoutNow = 13, 14
OutTransfer = 17
FlagTimeoutNow = 0x20
ELECTION_TICK = Q.ELECTION_TICK
RULES = (3, 4, 5, 6, 7, 8, 9)
RULE_NAMES = {3: "lease", 4: "leader_transfer", 5: "ack_timeout_now", 6: "drop_props", 7: "reset", 8: "forward", 9: "timeout_now"}
_BY_NAME = {v: k for k, v in RULE_NAMES.items()}


def rules(leave_out):
    """leave_out= as rule numbers or as RULE_NAMES' names -> frozenset of numbers"""
    return frozenset(_BY_NAME.get(x, x) for x in leave_out)


class _TransferArms:
    """the rules; `lt_out` (tests only): rule numbers this instance does NOT apply.  Without 3 a marked MsgVote is any MsgVote;
    without 4, 8, 9 the role ignores the message; without 5 no ack carries the flag; without 6 the proposal is taken; without 7
    the transferee survives reset() and the check."""
    lt_out = frozenset()
    transferee = R.NONE  # raft ID (slot + 1)
    _marked = False

    def reset(self, term):
        super().reset(term)
        if 7 not in self.lt_out:
            self.transferee = R.NONE

    def in_lease(self):  # (asked by the lease rule alone)
        return not self._marked and super().in_lease()

    def _step(self, m):
        self._marked = m.type == R.MsgVote and bool(m.reject) and 3 not in self.lt_out
        return super()._step(m)

    def step_leader(self, m):
        if m.type == MsgTransferLeader:
            t = m.frm
            if 4 in self.lt_out or t not in self.members() or self.transferee == t:
                return R.Result()
            self.transferee = R.NONE  # abortLeaderTransfer (lead_elapsed is left as it is)
            if t == self.id:
                return R.Result()
            self.transferee, self.lead_elapsed = t, 0
            mt = self.prs[t].match
            return R.Result(OutTransfer, index=mt, flags=FlagTimeoutNow if mt == self.last_index else 0)
        if m.type == P.MsgProp and self.transferee != R.NONE and 6 not in self.lt_out:
            return R.Result()
        res = super().step_leader(m)
        if m.type == Q.MsgCheckQuorum and 7 not in self.lt_out:
            self.transferee = R.NONE
        if (m.type == R.MsgAppResp and 5 not in self.lt_out and res.flags & R.FlagUpdated and self.transferee == m.frm
                and self.prs[m.frm].match == self.last_index):
            res.flags |= FlagTimeoutNow
        return res

    def step_follower(self, m):
        if m.type == MsgTransferLeader:
            return R.Result() if 8 in self.lt_out or self.lead == R.NONE else R.Result(P.OutForward)
        if m.type == MsgTimeoutNow:
            if 9 in self.lt_out or self.id not in self.members():
                return R.Result()
            self.become_candidate()  # campaign(campaignTransfer): never the pre-candidate step
            if self.q() == self.poll(self.id, True):
                self.become_leader()
                return R.Result(R.OutBecameLeader, self.last_index, self.last_term)
            return R.Result(R.OutCampaign, self.last_index, self.last_term, reject=1)
        return super().step_follower(m)


@dataclass
class TPRaft(_TransferArms, PV.PRaft, P.PRaft):
    pass


@dataclass
class TPVRaft(_TransferArms, PV.PVRaft, P.PVRaft):
    pass


@dataclass
class TCRaft(_TransferArms, Q.CRaft, P.PRaft):
    pass


@dataclass
class TCVRaft(_TransferArms, Q.CVRaft, P.PVRaft):
    pass


LOCAL = (R.MsgHup, R.MsgBeat, Q.MsgCheckQuorum)


def step_batch(s, voters, active, lead_elapsed, transferee, msgs, pre_vote=True, election_tick=ELECTION_TICK, leave_out=frozenset(),
               frames=False):
    """Step for every message, in order, with raftq_set_check_quorum, raftq_set_lead_transfer and raftq_step_set_props on (and
    raftq_set_pre_vote, if pre_vote) -> (raftq_step_out_t[], transferee); `s`, `active`, `lead_elapsed` and `transferee` move.
    voters: the masks, or None for a handle without them.  leave_out: this module's rule numbers or names."""
    out = np.zeros(len(msgs), dtype=pyoracle.STEP_OUT_DT)
    rafts = {}
    lt_out = rules(leave_out)
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
                                             classes=(TPRaft, TPVRaft) if pre_vote else (TCRaft, TCVRaft))
            r.lt_out, r.transferee = lt_out, int(transferee[g])
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
        active[g] = sum(1 << (p - 1) for p in r.active)
        lead_elapsed[g] = r.lead_elapsed
        transferee[g] = r.transferee
    return out, transferee


# ---- Tick --------------------------------------------------------------------------------------------------------------------------
def tick(oracle, role, elapsed, active, lead_elapsed, transferee, voters, self_peer, n_peers, election_tick, heartbeat_tick, seed, tick_no):
    """ref_check_quorum.tick_array over the word's packed low half (activity bits | transferee << 12): a check that falls due and
    passes clears the half, every other case keeps it -> (elapsed', action, active', lead_elapsed', transferee', n_hup, n_beat)"""
    low = (np.asarray(active, np.uint16) & np.uint16(0x0FFF)) | (np.asarray(transferee, np.uint16) << np.uint16(12))
    el, act, low2, le2, n_hup, n_beat = Q.tick_array(oracle, role, elapsed, low, lead_elapsed, voters, self_peer, n_peers, election_tick,
                                                     heartbeat_tick, seed, tick_no)
    return el, act, (low2 & np.uint16(0x0FFF)).astype(np.uint16), le2, (low2 >> np.uint16(12)).astype(np.uint8), n_hup, n_beat


def tick_input(g, n, self_peer, election_tick, seed, masks=False):
    """ref_check_quorum.tick_input with a pending transferee in two leaders of three (a non-leader holds none) and lead_elapsed
    staggered over the whole timeout -> (role, elapsed, active, lead_elapsed, transferee, voters | None)"""
    role, elapsed, active, lead_elapsed, voters = Q.tick_input(g, n, self_peer, election_tick, seed, masks)
    rng = np.random.default_rng(seed + 1)
    transferee = np.where((role == Q.LEADER) & (rng.random(g) < 2 / 3), 1 + rng.integers(0, n, g), 0).astype(np.uint8)
    lead_elapsed = (np.arange(g) % election_tick).astype(np.uint32)
    return role, elapsed, active, lead_elapsed, transferee, voters


# ---- the Step inputs ---------------------------------------------------------------------------------------------------------------
G, N_MSGS = Q.G, Q.N_MSGS
SHAPES = ((3, 0), (3, 2), (5, 0), (5, 4), (9, 0), (9, 8))  # self in the first and in the last slot
PLANT = 8
ARM_FLOOR = 8


def _rec(m, at, group, type, term=0, frm=0, index=0, log_term=0, reject=0, flags=0):
    PV._rec(m, at, group, type, term, frm, index, log_term, reject, flags)


def _prop(m, at, group, k=1, frm=0):
    m[at] = np.zeros(1, m.dtype)[0]
    P._prop(m, at, group, k, frm=frm)


def step_case(n, self_peer, seed, masks=False, pre_vote=True, hot=False, g=G, n_msgs=N_MSGS, band=None, plants=None):
    """one (start = (state, active, lead_elapsed, transferee), voters | None, batch, the reference's records, the four after).
    ref_step_props.props_state's dealt roles (with pre_vote every third candidate a pre-candidate), elapsed on both sides of
    election_tick, a pending transferee in one led group of three, and _stepgen's traffic with one record in six turned into a
    MsgTransferLeader or MsgTimeoutNow, one in ten into a MsgProp, and every MsgVote's reject byte drawn.  In front, per arm PLANT
    groups with one directed exchange each; `last` = the highest slot that is not self (N = 9, self 0: slot 8, nibble 9, activity
    bit 8 set):
      led, none pending         MsgTransferLeader(last), Match behind the tail: OUT_TRANSFER; then the ack that reaches the tail
                                (TIMEOUT_NOW), then a MsgProp (dropped)
      led, none pending         MsgTransferLeader(last), Match at the tail: OUT_TRANSFER with TIMEOUT_NOW
      led, none pending         MsgTransferLeader(last), Match beyond the tail: no flag; an ack beyond the tail (clamped) sets it
      led, pending `last`       the same transferee again: ignored; lead_elapsed 65535 stays; an ack that does not update: no flag
      led, pending `last`       MsgTransferLeader(another peer): aborted and replaced, lead_elapsed 65535 -> 0
      led, pending `last`       MsgProp (dropped), MsgTransferLeader(self) (cancelled), MsgProp (taken)
      led, pending              a MsgHeartbeat of the next term: reset() clears it
      led, pending              MsgCheckQuorum with every bit set / with none: cleared either way
      led                       marked and unmarked MsgVote of the next term: the first deposes, the second (another group) is ignored
      following, elapsed 0      marked MsgVote of the next term: passes the lease; in other groups unmarked: ignored
      following, past it        marked and unmarked: answered as always
      following                 MsgTransferLeader at term 0 and at the own term: OUT_FORWARD; MsgTimeoutNow of the term before: ignored
      following nobody          MsgTransferLeader: OUT_NONE; MsgTimeoutNow at the own term: campaigns
      following                 MsgTimeoutNow at the own term, and of the next term: campaigns, votes marked
      candidate                 MsgTransferLeader and MsgTimeoutNow: ignored
      led                       MsgTimeoutNow: ignored
    masks: the planted groups vote in full, but for PLANT led groups whose `last` is no voter (ignored), PLANT followers in which
    self is no voter (MsgTimeoutNow: OUT_NONE) and PLANT in which self is the ONE voter (OUT_BECAME_LEADER).
    `hot`: a led group with 40 records in a row -- MsgTransferLeader, acks from every peer, MsgProps, a cancel, again.
    band: the state lifted by tests/_widegen first and the traffic drawn by its wide_batch.  Five
    more led groups with the tail at B (b32 / b63; "top": where the lift put it) and none pending get MsgTransferLeader(last):
      Match == tail             OUT_TRANSFER with TIMEOUT_NOW at once
      Match == far(tail)        2^32 away (tests/_widegen.far), the low words equal: OUT_TRANSFER, no flag
      Match == tail - 1         no flag; the acknowledgement that moves it to the tail carries TIMEOUT_NOW
    and in b32 / b63 the `tn_up` followers stand at term B - 1: the MsgTimeoutNow of the next term is B.  plants: a dict that is
    told these groups."""
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
    last = max(others)
    other = min(others)
    active = rng.integers(0, full + 1, g).astype(np.uint16)
    lead_elapsed = rng.integers(0, ELECTION_TICK, g).astype(np.uint32)
    led = np.flatnonzero(s.role == 2)
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0))
    lost = np.flatnonzero((s.role == 0) & (s.lead == 0))
    cnd = np.flatnonzero(s.role == 1)
    transferee = np.zeros(g, np.uint8)
    transferee[led] = np.where(rng.random(len(led)) < 1 / 3, 1 + rng.integers(0, n, len(led)), 0)
    voters = None
    if masks:
        voters = rng.integers(0, full + 1, g).astype(np.uint16)
        voters[rng.random(g) < 0.75] |= np.uint16(1 << self_peer)
    n_fol_sets = 7
    H, T = PLANT // 2, 3
    assert len(led) >= 3 * PLANT + H + 6 * T + 1 + (PLANT if masks else 0) and len(fol) >= n_fol_sets * PLANT and len(lost) >= PLANT and len(cnd) >= PLANT, \
        (len(led), len(fol), len(lost), len(cnd))
    S1, S2, S3 = (led[k * PLANT:(k + 1) * PLANT] for k in range(3))
    S4 = led[3 * PLANT:3 * PLANT + H]
    rest_led = led[3 * PLANT + H:]
    rst, chk_pass, chk_fail, led_vote_m, led_vote_u, led_tn = (rest_led[k * T:(k + 1) * T] for k in range(6))
    hot_group = int(rest_led[6 * T])
    non_voter_t = rest_led[6 * T + 1:6 * T + 1 + PLANT] if masks else rest_led[:0]
    F = [fol[k * PLANT:(k + 1) * PLANT] for k in range(n_fol_sets)]
    in_m, in_u, out_l, fwd, tn_own, tn_up = F[0][:H], F[0][H:], F[1], F[2], F[3], F[4]
    self_out, self_only = (F[5], F[6]) if masks else (fol[:0], fol[:0])
    lost_p, cnd_p = lost[:PLANT], cnd[:PLANT]
    wide = rest_led[6 * T + 1 + len(non_voter_t):][:5] if band is not None else led[:0]
    assert len(wide) == (5 if band is not None else 0), len(led)
    at_tail, far_off, by_ack = wide[:1], wide[1:3], wide[3:]
    planted = np.concatenate([S1, S2, S3, S4, rst, chk_pass, chk_fail, [hot_group], led_vote_m, led_vote_u, led_tn, non_voter_t, F[0], out_l, fwd,
                              tn_own, tn_up, self_out, self_only, lost_p, cnd_p, wide])
    assert len(np.unique(planted)) == len(planted)
    if masks:
        voters[planted] = full
        voters[non_voter_t] = full & ~(1 << last)
        voters[self_out] = full & ~(1 << self_peer)
        voters[self_only] = 1 << self_peer
    # the led plants: a log of some length, every peer's Match where the arm wants it
    for grp in np.concatenate([S1, S2, S3, S4, [hot_group]]):
        s.last_index[grp] = max(int(s.last_index[grp]), 6)
        s.match[self_peer, grp] = s.last_index[grp]
        s.match[last, grp] = int(s.last_index[grp]) - 3
        s.match[other, grp] = int(s.last_index[grp]) - 1
    s.match[last, S2] = s.match[other, S2] = s.last_index[S2]
    s.match[last, S3[:H]] = s.last_index[S3[:H]]
    s.match[last, S3[H:]] = s.last_index[S3[H:]] + np.uint64(2)
    transferee[np.concatenate([S1, S3, S4, [hot_group], led_vote_m, led_vote_u, led_tn, non_voter_t])] = 0
    transferee[np.concatenate([S2, rst, chk_pass, chk_fail])] = last + 1
    active[np.concatenate([S1, S2])] = full  # (the top activity bit beside the nibble)
    lead_elapsed[S2] = 65535
    active[chk_pass], active[chk_fail] = full, 0
    s.elapsed[F[0]], s.elapsed[out_l] = 0, ELECTION_TICK + 3
    s.term[fwd] = np.maximum(s.term[fwd], 2)
    s.last_term[fwd] = np.minimum(s.last_term[fwd], s.term[fwd])
    free = np.setdiff1d(np.arange(g), planted)
    if band is None:
        m = _stepgen.random_batch(rng, s, n_msgs)
    else:
        if WG.BANDS[band]:
            s.last_index[wide] = s.match[self_peer, wide] = WG.BANDS[band]
            s.committed[wide] = np.minimum(s.committed[wide], s.last_index[wide])
            WG.set_term(s, tn_up, WG.BANDS[band] - 1)
        s.match[:, wide] = np.where(np.arange(n)[:, None] == self_peer, s.last_index[wide][None, :], s.last_index[wide][None, :] - np.uint64(3))
        s.match[last, at_tail] = s.last_index[at_tail]
        s.match[last, far_off] = [WG.far(band, int(v)) for v in s.last_index[far_off]]
        s.match[last, by_ack] = s.last_index[by_ack] - np.uint64(1)
        transferee[wide] = 0
        m = WG.wide_batch(rng, s, n_msgs)
    if plants is not None:
        plants.update(at_tail=at_tail, far=far_off, by_ack=by_ack, tn_up=tn_up, last=last)
    at = 0

    def put(*a, **kw):
        nonlocal at
        _rec(m, at, *a, **kw)
        at += 1

    def put_prop(grp):
        nonlocal at
        _prop(m, at, grp, 2, frm=other)
        at += 1

    for grp in S1:
        t, li = int(s.term[grp]), int(s.last_index[grp])
        put(grp, MsgTransferLeader, frm=last)                          # set, behind
        put(grp, R.MsgAppResp, term=t, frm=last, index=li)             # the completing ack: TIMEOUT_NOW
        put_prop(grp)                                                  # dropped
        put(grp, MsgTransferLeader, frm=last)                          # the same again: ignored
        put(grp, MsgTransferLeader, frm=other)                         # aborted and replaced
        put(grp, MsgTransferLeader, frm=self_peer)                     # cancelled
        put_prop(grp)                                                  # taken
        put(grp, MsgTransferLeader, frm=self_peer)                     # nothing to cancel
    for k, grp in enumerate(S2):
        t, li = int(s.term[grp]), int(s.last_index[grp])
        put(grp, MsgTransferLeader, frm=last)                          # the same again: lead_elapsed 65535 stays
        put(grp, R.MsgAppResp, term=t, frm=last, index=li)             # no update: no flag
        if k % 2:
            put(grp, MsgTransferLeader, term=t, frm=other)             # replaced (the forwarded form), at the tail, 65535 -> 0
            put(grp, R.MsgAppResp, term=t, frm=last, index=li)
    for k, grp in enumerate(S3):
        put(grp, MsgTransferLeader, term=int(s.term[grp]) if k % 2 else 0, frm=last)  # at the tail | beyond it
        if k >= H:
            put(grp, R.MsgAppResp, term=int(s.term[grp]), frm=last, index=int(s.last_index[grp]) + 4)  # no update
    for grp in S4:
        put(grp, MsgTransferLeader, frm=last)
        put(grp, R.MsgAppResp, term=int(s.term[grp]), frm=last, index=int(s.last_index[grp]) + 4)  # beyond the tail: clamped, TIMEOUT_NOW
    for grp in rst:
        put(grp, R.MsgHeartbeat, term=int(s.term[grp]) + 1, frm=other)
    for grp in np.concatenate([chk_pass, chk_fail]):
        put(grp, Q.MsgCheckQuorum)
    vote = lambda grp, mark: put(grp, R.MsgVote, term=int(s.term[grp]) + 1, frm=last, index=int(s.last_index[grp]) + 5,
                                 log_term=int(s.term[grp]) + 1, reject=mark)
    for grp in np.concatenate([led_vote_m, in_m]):
        vote(grp, 1)
    for grp in np.concatenate([led_vote_u, in_u]):
        vote(grp, 0)
    for k, grp in enumerate(out_l):
        vote(grp, k % 2)
    for grp in led_tn:
        put(grp, MsgTimeoutNow, term=int(s.term[grp]), frm=other)
    for grp in non_voter_t:
        put(grp, MsgTransferLeader, frm=last)
    for k, grp in enumerate(fwd):
        put(grp, MsgTransferLeader, term=int(s.term[grp]) if k % 2 else 0, frm=last)
        put(grp, MsgTimeoutNow, term=int(s.term[grp]) - 1, frm=other)
    for grp in lost_p:
        put(grp, MsgTransferLeader, frm=last)
        put(grp, MsgTimeoutNow, term=int(s.term[grp]), frm=other)
    for grp in np.concatenate([tn_own, self_out, self_only]):
        put(grp, MsgTimeoutNow, term=int(s.term[grp]), frm=int(s.lead[grp]) - 1)
    for grp in tn_up:
        put(grp, MsgTimeoutNow, term=int(s.term[grp]) + 1, frm=other)
    for grp in cnd_p:
        put(grp, MsgTransferLeader, frm=last)
        put(grp, MsgTimeoutNow, term=int(s.term[grp]), frm=other)
    for grp in wide:
        put(grp, MsgTransferLeader, frm=last)
    for grp in by_ack:
        put(grp, R.MsgAppResp, term=int(s.term[grp]), frm=last, index=int(s.last_index[grp]))
    assert at < n_msgs * 3 // 5, at
    rest = np.arange(at, n_msgs)
    m["group"][rest] = rng.choice(free, len(rest))  # (the directed exchanges stay undisturbed)
    if hot:
        t0, li = int(s.term[hot_group]), int(s.last_index[hot_group])
        for j, i in enumerate(rest[:40]):
            k = j % 10
            if k == 0:
                _rec(m, i, hot_group, MsgTransferLeader, frm=last if j < 20 else other)
            elif j == 1:
                _rec(m, i, hot_group, R.MsgAppResp, term=t0, frm=last, index=li)  # the completing ack
            elif k in (3, 8):
                _prop(m, i, hot_group, 1, frm=other)
            elif k == 6:
                _rec(m, i, hot_group, MsgTransferLeader, frm=self_peer)
            else:  # (the tail moves with every proposal taken: acks around it, from every peer)
                _rec(m, i, hot_group, R.MsgAppResp, term=t0, frm=int(rng.choice(others)), index=li + int(rng.integers(-1, 4)))
        rest = rest[40:]
    votes = rest[m["type"][rest] == R.MsgVote]
    m["reject"][votes] = rng.random(len(votes)) < 0.5
    for i in rest[rng.random(len(rest)) < 1 / 6]:
        grp = int(m["group"][i])
        kind = MsgTransferLeader if rng.random() < 0.5 else MsgTimeoutNow
        term = 0 if kind == MsgTransferLeader and rng.random() < 0.5 else max(1, int(s.term[grp]) + int(rng.choice([-1, 0, 0, 0, 1])))
        _rec(m, i, grp, kind, term=term, frm=int(rng.integers(0, n)))
    for i in rest[rng.random(len(rest)) < 0.1]:
        _prop(m, i, int(m["group"][i]), int(rng.integers(1, 4)), frm=int(rng.integers(0, n)))
    start = (V.copy_state(s), active.copy(), lead_elapsed.copy(), transferee.copy())
    if band is not None:
        WG.guard_case(s, m)
    want, _ = step_batch(s, voters, active, lead_elapsed, transferee, m, pre_vote)
    if band is not None:
        WG.guard_case(s, m)
    for a in (m, want):
        a.setflags(write=False)
    return start, voters, m, want, (s, active, lead_elapsed, transferee)


def case_list():
    """the arguments of every step_case() the GPU tests step (tests/test_lead_transfer_ref.py shows that each one discriminates)"""
    cases = []
    for k, (n, me) in enumerate(SHAPES):
        for masks in (False, True):
            for pv in (False, True):
                cases.append(dict(n=n, self_peer=me, seed=10500 + 4 * k + 2 * masks + pv, masks=masks, pre_vote=pv))
    cases.append(dict(n=3, self_peer=1, seed=10540, hot=True))
    cases.append(dict(n=9, self_peer=0, seed=10541, hot=True, masks=True, pre_vote=False))
    for k, band in enumerate(WG.BAND_NAMES):  # appended: the positions above are what the GPU tests pick by
        cases.append(dict(n=3, self_peer=0, seed=10550 + k, pre_vote=bool(k & 1), band=band))
        cases.append(dict(n=9, self_peer=8, seed=10560 + k, masks=True, pre_vote=not k & 1, band=band))
    return cases


def case_id(c):
    return "n%d-self%d%s%s%s" % (c["n"], c["self_peer"], "-masks" if c.get("masks") else "", "-pv" if c.get("pre_vote", True) else "", "-hot" if c.get("hot") else "") + ("-" + c["band"] if c.get("band") else "")


def case_rules(c):
    """the rules a case is held to discriminate (every case plants every arm)"""
    return RULES


def copy_start(t):
    return V.copy_state(t[0]), t[1].copy(), t[2].copy(), t[3].copy()


def changed_records(start, voters, m, want, after, rule, pre_vote=True):
    """the records whose result, or whose group's final state, is another when `rule` is left out -> their batch positions"""
    st = copy_start(start)
    without, _ = step_batch(st[0], voters, st[1], st[2], st[3], np.array(m), pre_vote, leave_out={rule})
    k = want.dtype.itemsize
    differs = (without.view(np.uint8).reshape(-1, k) != np.array(want).view(np.uint8).reshape(-1, k)).any(axis=1)
    sa, sb = st[0], after[0]
    moved = np.zeros(sa.G, bool)
    for name, _ in pyoracle.NodeState.FIELDS:
        moved |= getattr(sa, name) != getattr(sb, name)
    moved |= (sa.match != sb.match).any(axis=0) | (sa.votes != sb.votes).any(axis=0)
    for x, y in zip(st[1:], after[1:]):
        moved |= x != y
    return np.flatnonzero(differs | moved[m["group"].astype(np.int64)])


def arms(start, voters, m, want):
    """which arm of rules 4 and 9 every record took, read off the reference's run -> dict of counts"""
    s0 = start[0]
    n = s0.N
    c = {k: 0 for k in ("4 set, behind", "4 set, at the tail", "4 same again", "4 replaced", "4 cancelled", "4 nothing to cancel",
                        "9 campaigns", "9 stale", "9 ignored by role")}
    if voters is not None:
        c.update({"4 no voter": 0, "9 not promotable": 0, "9 became leader": 0})
    role, tr, term = {}, {}, {}
    for i in range(len(m)):
        grp, t = int(m["group"][i]), int(m["type"][i])
        r0, t0, term0 = role.get(grp, int(s0.role[grp])), tr.get(grp, int(start[3][grp])), term.get(grp, int(s0.term[grp]))
        o = want[i]
        fl = int(m["_pad"][i][1])
        live = not fl & (V.MSGF_SKIP | V.MSGF_HOLD) and int(o["type"]) != R.OutDeferred
        stale = 0 < int(m["term"][i]) < term0
        frm = int(m["from"][i])
        if live and t == MsgTransferLeader and r0 == 2 and int(o["role"]) == 2 and not stale:
            if voters is not None and not (int(voters[grp]) >> frm) & 1:
                c["4 no voter"] += 1
            elif t0 == frm + 1:
                c["4 same again"] += 1
            elif frm == s0.self_peer:
                c["4 cancelled" if t0 else "4 nothing to cancel"] += 1
            else:
                assert int(o["type"]) == OutTransfer
                if t0:
                    c["4 replaced"] += 1
                c["4 set, at the tail" if int(o["flags"]) & FlagTimeoutNow else "4 set, behind"] += 1
        if live and t == MsgTimeoutNow:
            if stale:
                c["9 stale"] += 1
            elif int(o["type"]) == R.OutCampaign:
                assert int(o["reject"]) == 1
                c["9 campaigns"] += 1
            elif int(o["type"]) == R.OutBecameLeader:
                c["9 became leader"] += 1
            elif int(o["role"]) == 0 and voters is not None and not (int(voters[grp]) >> s0.self_peer) & 1:
                c["9 not promotable"] += 1
            else:
                c["9 ignored by role"] += 1
        if live:
            role[grp], term[grp] = int(o["role"]), int(o["term"])
            # the transferee behind record i, as the rules say it (the reference's own is only known at the batch's end)
            if int(o["type"]) == OutTransfer:
                tr[grp] = frm + 1
            elif int(o["role"]) != 2 or r0 != 2 or t == Q.MsgCheckQuorum or (t == MsgTransferLeader and frm == s0.self_peer and not stale):
                tr[grp] = 0
            elif int(o["type"]) == R.OutBecameLeader:
                tr[grp] = 0
    return c


# ---- three nodes, scripted ---------------------------------------------------------------------------------------------------------
def route(k, outs, batch, n=3):
    """ref_pre_vote.route, plus: an OUT_CAMPAIGN's MsgVotes carry its mark; OUT_TRANSFER without the flag and an updating ack's
    OUT_PROGRESS below the tail send the MsgApp that brings the peer to the tail (sendAppend, the entries' count said); the flag
    sends MsgTimeoutNow; OUT_APPENDED is acknowledged; OUT_FORWARD sends the record on as it came.  -> {addressee: raftq_msg_t[]}"""
    per = {p: [] for p in range(n) if p != k}
    base = PV.route(k, outs, n)
    marked = {int(o["group"]) for o in outs if int(o["type"]) == R.OutCampaign and int(o["reject"])}
    for p, a in base.items():
        a = a.copy()
        for i in range(len(a)):
            if int(a["type"][i]) == R.MsgVote and int(a["group"][i]) in marked:
                a["reject"][i] = 1
        per[p] = [a]
    for o, b in zip(outs, batch):
        t, grp, to = int(o["type"]), int(o["group"]), int(o["to"])
        one = np.zeros(1, pyoracle.STEP_MSG_DT)
        send = []
        if int(o["flags"]) & FlagTimeoutNow:
            _rec(one, 0, grp, MsgTimeoutNow, term=int(o["term"]), frm=k)
            send.append(one.copy())
        elif t == OutTransfer or (t == R.OutProgress and int(b["type"]) == R.MsgHeartbeatResp and int(o["index"]) < int(o["last_index"])):
            # sendAppend(to): everything behind its Match (the scenario's logs hold one term, so LogTerm is the log's)
            _rec(one, 0, grp, R.MsgApp, term=int(o["term"]), frm=k, index=int(o["index"]), log_term=1, flags=V.MSGF_ENTRIES)
            one["_resv"][0] = int(o["last_index"]) - int(o["index"])
            one["reject_hint"][0] = 1
            one["commit"][0] = int(o["commit"])
            send.append(one.copy())
        elif t == R.OutAppended:
            _rec(one, 0, grp, R.MsgAppResp, term=int(o["term"]), frm=k, index=int(o["index"]))
            send.append(one.copy())
        elif t == P.OutForward:
            one[0] = b
            send.append(one.copy())
        if to != k and to in per:
            per[to].extend(send)
    return {p: np.concatenate(lst) if lst else np.zeros(0, pyoracle.STEP_MSG_DT) for p, lst in per.items()}


class Cluster(PV.Cluster):
    """ref_pre_vote.Cluster whose nodes run the transfer's rules and route its messages; node 2's log can be left `behind` by
    some entries (the leader then has to bring it up to date before MsgTimeoutNow).  leave_out: this module's rules, on every node."""

    def __init__(self, g, pre_vote, behind=0, leave_out=frozenset(), **kw):
        super().__init__(g, pre_vote, **kw)
        self.transferee = [np.zeros(g, np.uint8) for _ in range(self.N)]
        self.leave_out = rules(leave_out)
        self.log = []  # (node, batch, results) of every Step, in order
        for k in range(self.N):
            self.s[k].match[:, :] = 0
            self.s[k].match[k] = 5
        self.s[0].match[1], self.s[0].match[2] = 5, 5 - behind
        self.s[2].last_index[:] = 5 - behind
        self.s[2].match[2] = 5 - behind
        for k in range(self.N):
            self.s[k].committed[:] = 5 - behind

    def _step(self, s, active, lead_elapsed, msgs):
        k = next(i for i in range(self.N) if self.s[i] is s)
        out, _ = step_batch(s, None, active, lead_elapsed, self.transferee[k], msgs, self.pre_vote, self.et, self.leave_out)
        return out

    def inject(self, k, msgs):
        self.inbox[k] = np.concatenate([self.inbox[k], msgs])

    def turn(self, k):
        s = self.s[k]
        el, act, ac, le, tr, _, _ = tick(pyoracle, s.role, s.elapsed, self.active[k], self.lead_elapsed[k], self.transferee[k], None, k, self.N,
                                         self.et, self.ht, self.seed + k, self.tick_no[k])
        self.tick_no[k] += 1
        s.elapsed[:], self.active[k][:], self.lead_elapsed[k][:], self.transferee[k][:] = el, ac, le, tr
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
        self.log.append((k, batch, outs))
        if self.on_step:
            self.on_step(k, batch, outs)
        if k in self.cut:
            return
        for p, msgs in route(k, outs, batch, self.N).items():
            if p not in self.cut and len(msgs):
                self.inbox[p] = np.concatenate([self.inbox[p], msgs])


def transfer_msgs(g, to, frm_term=0):
    """one local MsgTransferLeader per group (what node.TransferLeadership steps on the leader)"""
    a = np.zeros(g, pyoracle.STEP_MSG_DT)
    for grp in range(g):
        _rec(a, grp, grp, MsgTransferLeader, term=frm_term, frm=to)
    return a


def prop_msgs(g, frm):
    a = np.zeros(g, pyoracle.STEP_MSG_DT)
    for grp in range(g):
        _prop(a, grp, grp, 1, frm=frm)
    return a
