"""Every writer of a handle interleaved with Step, with the Step switches on: the schedules and the reference composed of what the
suite already trusts.  A group's Step record holds copies of role, committed, the term gate and the match words (raftq_step_kernels.hpp
NodeRec); every writer that is not Step marks them stale (raftq_internal.hpp dense_changed) and Step writes back what it changed
(NodeT::store).  A schedule is a seeded sequence of MOVES -- one call of one writer -- each followed by one Step batch that reads
what the move changed, on ONE handle from the first move to the last.

  schedule(case)     the moves of a case, built once (functools.lru_cache): per move the inputs of its call, the outputs the call
                     must produce, the groups it changed, the Step batch behind it (or a pipelined pair of batches) with the
                     records it must give, and the reference's state before the move, behind it and behind the batch
  what_if(ref)       what the two RAFTQ_SWEEP_NO_ADOPT sweeps must find on a handle that stands where `ref` stands
  discriminates(mv)  the batch behind a move, stepped on the state in FRONT of the move, gives other records in a changed group

The reference of every move is the one its own suite uses (oracle.pyoracle, ref_voters, ref_step_voters, ref_tick_members,
ref_check_quorum, ref_propose_forward, ref_respond_props / ref_check_quorum_props, test_tick_frames_gpu.want_frames,
test_tick_elect_gpu.want_round); Step is ref_step_props.step_batch, ref_check_quorum_props.step_batch under CheckQuorum.
The cases with raftq_set_pre_vote, raftq_set_lead_transfer, raftq_set_read_index and raftq_tick_set_checks on (CASES' second half, "extended"
below) carry a ref_read_index.Extra beside the node state; their Step is ref_read_index.step_batch, their Tick ref_lead_transfer.tick,
their fused Tick calls ref_tick_checks' composition, and their batches hold the records that read the transferee, the read record
and role 3 (follow_records_x, random_records_x).  The six cases of round 26 take none of those paths: their schedules are byte for
byte what they were (python -m tests.interleave_digest).
Nothing in here runs the code under test.  TEST INFRASTRUCTURE: nothing in the product imports it."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import pyoracle
from oracle import pywire as W
from tests import _stepgen, _wiregen
from tests import ref_bcast_members as B
from tests import ref_check_quorum as Q
from tests import ref_check_quorum_props as CP
from tests import ref_lead_transfer as T
from tests import ref_pre_vote as PV
from tests import ref_propose_forward as RF
from tests import ref_raft_py as R
from tests import ref_read_index as RI
from tests import ref_respond_props as RP
from tests import ref_step_props as P
from tests import ref_step_voters as V
from tests import ref_tick_checks as RC
from tests import ref_tick_members as TM
from tests import ref_voters as RV

U = np.uint64
G = 1027  # four full 256-lane workgroups of the mirror and walk kernels and a ragged fifth; one group past a 1,024-group Tick block
ET, HB, SEED = Q.ELECTION_TICK, 1, 0x5EED
K_RUN = 40  # records of one group in a pipelined pair: more than the list walk's kMaxRun = 32
N_RANDOM, N_HOT = 320, 160  # the random part of a batch: records, and the groups they are drawn over
MAX_CHANGED = 512

CASES = {
    "n3": dict(n=3, me=1, masks=False, cq=False, walk="lists", schedule="n3"),
    "n9": dict(n=9, me=8, masks=False, cq=False, walk="lists", schedule="n9"),  # 32-bit vote words
    "n5-masked": dict(n=5, me=4, masks=True, cq=False, walk="lists", schedule="n5-masked"),
    "n3-cq": dict(n=3, me=1, masks=False, cq=True, walk="lists", schedule="n3-cq"),
    "n5-masked-cq": dict(n=5, me=4, masks=True, cq=True, walk="lists", schedule="n5-masked-cq"),
    "n5-masked-cq-sort": dict(n=5, me=4, masks=True, cq=True, walk="sort", schedule="n5-masked-cq"),  # the same schedule
}
SEEDS = {"n3": 26003, "n9": 26009, "n5-masked": 26005, "n3-cq": 26103, "n5-masked-cq": 26105}

# Round 33: the same writers crossed with raftq_set_pre_vote (pv), raftq_set_lead_transfer (lt), raftq_set_read_index (ri: its mode) and
# the fused Tick calls raftq_tick_set_checks reopens (checks).  All of them run under CheckQuorum.  A case with these keys is
# "extended" below (Ref.ext): its moves, batches and Step reference are the *_x forms; the six cases above take none of those paths.
SAFE, LEASE = RI.SAFE, RI.LEASE
CASES.update({
    "n3-all-safe": dict(n=3, me=1, masks=False, cq=True, walk="lists", schedule="n3-all-safe", pv=True, lt=True, ri=SAFE, checks=False),
    "n5-masked-all-safe": dict(n=5, me=4, masks=True, cq=True, walk="lists", schedule="n5-masked-all-safe", pv=True, lt=True, ri=SAFE, checks=False),
    "n5-masked-all-safe-sort": dict(n=5, me=4, masks=True, cq=True, walk="sort", schedule="n5-masked-all-safe", pv=True, lt=True, ri=SAFE, checks=False),
    "n9-lt-lease-checks": dict(n=9, me=8, masks=False, cq=True, walk="lists", schedule="n9-lt-lease-checks", pv=False, lt=True, ri=LEASE, checks=True),
    "n3-pv-lease-checks": dict(n=3, me=1, masks=False, cq=True, walk="lists", schedule="n3-pv-lease-checks", pv=True, lt=False, ri=LEASE, checks=True),
})
SEEDS.update({"n3-all-safe": 33003, "n5-masked-all-safe": 33005, "n9-lt-lease-checks": 33009, "n3-pv-lease-checks": 33103})
EXTENDED = tuple(k for k, c in CASES.items() if "pv" in c)
PV_RULES = (1, 2, 3, 4, 5)  # tests/ref_pre_vote.py's

# kinds that leave every word of the reference where it was (the issue's moves 13 to 15)
NO_CHANGE = ("clone", "narrow_rebuild", "refused")
# Tick without CheckQuorum and without the device's campaigns moves `elapsed` alone, a word Step neither reads nor reports with the
# switch off: no Step record can tell such a move from its absence (tests/test_interleave_ref.py asserts exactly that instead)
ELAPSED_ONLY = ("tick_lists", "tick_frames")
TICKS = ("tick", "tick_lists", "tick_frames", "tick_elect")
ONCE = ("unmask", "remask", "pv_off", "pv_on")
FORCED = {"unmask": "remask", "pv_off": "pv_on"}  # a window of one batch: the second kind comes right behind the first and nowhere else


def no_change(case):
    """the kinds that leave every word of a case's reference where it was: the lease mode holds no read record, so switching it
    over and back clears nothing"""
    c = CASES[case]
    if "pv" not in c:
        return NO_CHANGE
    return NO_CHANGE + ("tally_rebuild", "closed") + (("ri_toggle",) if c["ri"] == LEASE else ())


def closed_calls(case):
    """-> [(call, the word its refusal names)] for every call the case's switches close (include/raftq.h "What the switch closes",
    include/raftq_wire.h).  Without raftq_tick_set_checks the Tick forms are closed to CheckQuorum -- raftq_tick_elect_frames to
    PreVote first --, so what the safe mode closes shows only behind raftq_tick_set_checks: the "+checks" forms are tried with that
    switch turned on for the one call and off again.  raftq_set_check_quorum(0) names the first switch that needs it."""
    c = CASES[case]
    calls = []
    if not c["checks"]:
        calls += [("tick_collect", "check quorum"), ("tick_collect_lists", "check quorum"), ("tick_frames", "check quorum"),
                  ("tick_elect_frames", "pre vote" if c["pv"] else "check quorum")]
        if c["ri"] == SAFE:
            calls += [("tick_frames+checks", "read index"), ("tick_elect_frames+checks", "read index")]
    if c["lt"]:
        calls.append(("propose_frames", "lead transfer"))
    calls.append(("set_check_quorum(0)", "pre vote" if c["pv"] else "lead transfer" if c["lt"] else "read index"))
    return calls


def _kinds_x(c):
    """the kinds of an extended case.  Left out: `respond` -- no reference of the suite builds raftq_step_frames_respond's streams
    under these switches (ref_check_quorum_props.want knows CheckQuorum alone: no echoed context, no result kind above 13) --,
    `propose` where a transfer closes raftq_propose_frames, and `cq_toggle`, which every one of the three switches refuses."""
    k = dict.fromkeys(("deltas", "vote_deltas", "sweep", "cycle", "roles", "campaign", "term_deltas", "log_deltas", "log_deltas_nowait",
                       "clone", "narrow_rebuild", "refused", "tally_rebuild", "closed", "activity", "ri_toggle"), 2)
    if c["checks"]:
        k.update(tick_lists=2, tick_frames=2, tick_elect=2)
    else:
        k.update(tick=3)
    if c["lt"]:
        k.update(transfer=2, lt_toggle=2)
    else:
        k.update(propose=2)
    if c["ri"] == SAFE:
        k.update(reads=2)
    if c["pv"]:
        k.update(pv_off=1, pv_on=1)
    if c["masks"]:
        k.update(voter_deltas=2, unmask=1, remask=1)
    return k


def kinds_of(case):
    """-> {kind: how often} for a case of CASES"""
    c = CASES[case]
    if "pv" in c:
        return _kinds_x(c)
    k = dict.fromkeys(("deltas", "vote_deltas", "sweep", "cycle", "roles", "campaign", "term_deltas", "log_deltas", "log_deltas_nowait",
                       "propose", "respond", "clone", "narrow_rebuild", "refused"), 2)
    if c["cq"]:
        k.update(tick=3, activity=2, cq_toggle=2)
    else:
        k.update(tick_lists=1, tick_frames=1, tick_elect=2)
    if c["masks"]:
        k.update(voter_deltas=2, unmask=1, remask=1)
    return k


class Ref:
    """the reference side of a handle: an oracle NodeState, the masks (None: none loaded), the activity arrays (read only under
    CheckQuorum) and the handle's tick number"""

    def __init__(self, s, voters, cq, active, lead_elapsed):
        self.s, self.voters, self.cq, self.active, self.le, self.tick_no = s, voters, cq, active, lead_elapsed, 0
        self.saved = None  # the masks while they are dropped
        # an extended case (extend()): the switches as they stand, the case's PreVote (pv is off inside the pv_off window), and a
        # ref_read_index.Extra's other three arrays -- the transferees [G] u8, seq [G] u32 and acked [N][G] u32
        self.ext, self.pv, self.pv_case, self.lt, self.ri, self.checks = False, False, False, False, 0, False
        self.transferee = self.seq = self.acked = None

    def extend(self, case, transferee, seq, acked):
        c = CASES[case]
        self.case = case
        self.ext, self.pv, self.pv_case, self.lt, self.ri, self.checks = True, c["pv"], c["pv"], c["lt"], c["ri"], c["checks"]
        self.transferee, self.seq, self.acked = transferee, seq, acked
        return self

    def copy(self):
        c = Ref(V.copy_state(self.s), None if self.voters is None else self.voters.copy(), self.cq, self.active.copy(), self.le.copy())
        c.tick_no, c.saved = self.tick_no, self.saved
        if self.ext:
            c.case, c.ext, c.pv, c.pv_case, c.lt, c.ri, c.checks = self.case, True, self.pv, self.pv_case, self.lt, self.ri, self.checks
            c.transferee, c.seq, c.acked = self.transferee.copy(), self.seq.copy(), self.acked.copy()
        return c

    @property
    def masks(self):
        return V.full_masks(self.s.N, self.s.G) if self.voters is None else self.voters

    @property
    def extra(self):
        """the arrays as the ref_read_index.Extra Step moves (views: the Ref moves with it)"""
        return RI.Extra(self.active, self.le, self.transferee, self.seq, self.acked)

    def unknown(self, m):
        """[len(m)] bool: records of a kind the handle's switches do not know (a batch that holds one is refused as a malformed one is)"""
        looked = (m["_pad"][:, 1] & (V.MSGF_SKIP | V.MSGF_HOLD)) == 0
        bad = np.zeros(len(m), bool)
        if not self.pv:
            bad |= np.isin(m["type"], (PV.MsgPreVote, PV.MsgPreVoteResp))
        if not self.lt:
            bad |= np.isin(m["type"], (T.MsgTransferLeader, T.MsgTimeoutNow))
        if not self.ri:
            bad |= np.isin(m["type"], (RI.MsgReadIndex, RI.MsgReadIndexResp))
        return looked & bad

    def step(self, m, ri_out=frozenset(), lt_out=frozenset(), pv_out=frozenset()):
        """Step for every record, in order -> raftq_step_out_t[]; a malformed batch raises ValueError and moves nothing.
        An extended case: ref_read_index.step_batch with the switches as they stand (*_out: rules of the three references left out,
        tests only).  Inside the pv_off window the classes are PreVote's with all five of its rules left out -- ref_pre_vote's own
        statement of a Step without the switch, under which a role-3 group is stepped by the follower's arm and keeps role 3 until a
        message gives it another (include/raftq.h "PreVote", Roles); tests/test_interleave_ref.py holds that form to the classes
        without PreVote on every group that is not in role 3."""
        if refuses(m, self.s.G, self.s.N):
            raise ValueError("malformed batch")
        if self.ext:
            if self.unknown(m).any():
                raise ValueError("a kind the switches do not know")
            if self.pv_case and not self.pv:
                pv_out = frozenset(PV_RULES)
            return RI.step_batch(self.s, self.voters, self.extra, m, mode=self.ri, pre_vote=self.pv_case, lead_transfer=self.lt, election_tick=ET,
                                 leave_out=ri_out, lt_leave_out=lt_out, pv_leave_out=pv_out)
        if self.cq:
            return CP.step_batch(self.s, self.voters, self.active, self.le, m, election_tick=ET)
        return P.step_batch(self.s, self.voters, m)

    def same(self, o):
        a, b = self.s, o.s
        if not all(np.array_equal(getattr(a, k), getattr(b, k)) for k, _ in pyoracle.NodeState.FIELDS):
            return False
        if self.ext and not ((self.pv, self.lt, self.ri) == (o.pv, o.lt, o.ri) and np.array_equal(self.transferee, o.transferee)
                             and np.array_equal(self.seq, o.seq) and np.array_equal(self.acked, o.acked)):
            return False
        return (np.array_equal(a.match, b.match) and np.array_equal(a.votes, b.votes) and np.array_equal(self.masks, o.masks)
                and np.array_equal(self.active, o.active) and np.array_equal(self.le, o.le))


def refuses(m, n_groups, n_peers):
    """include/raftq_step.h: a batch with a record whose group or `from` is out of range, or with a malformed MsgProp, applies
    nothing.  RAFTQ_MSGF_SKIP looks at no field, RAFTQ_MSGF_HOLD not at `from`; the local kinds carry no sender."""
    fl = m["_pad"][:, 1]
    seen = (fl & V.MSGF_SKIP) == 0
    local = np.isin(m["type"], (R.MsgHup, R.MsgBeat, Q.MsgCheckQuorum))
    bad_from = seen & ((fl & V.MSGF_HOLD) == 0) & ~local & (m["from"] >= n_peers)
    return bool((seen & (m["group"] >= n_groups)).any() or bad_from.any() or P.malformed(m, n_groups, n_peers).any())


@dataclass
class Move:
    kind: str
    args: dict = field(default_factory=dict)     # the inputs of the call
    want: dict = field(default_factory=dict)     # the outputs it must produce
    changed: np.ndarray = None                   # the groups it changed (at most MAX_CHANGED get a record in the batch behind)
    records: np.ndarray = None                   # records the batch behind must hold as they are (a Tick's MsgHups and checks)
    before: Ref = None                           # the reference in front of the move, behind it and behind the batch(es)
    after: Ref = None
    after_step: Ref = None
    batches: list = field(default_factory=list)  # one batch, or the two of a pipelined pair
    wants: list = field(default_factory=list)


@dataclass
class Schedule:
    case: str
    start: Ref
    moves: list
    ref_seconds: float


# ---- the Step batch behind a move -------------------------------------------------------------------------------------------------
def _others(n, me):
    return np.array([p for p in range(n) if p != me])


def follow_records(ref, groups, rng, timers=False):
    """one record for each of `groups` by what the group is NOW, so that its result reads what the move changed (tests/_refusals.py
    walk_batch is the model): a led group gets an acknowledgement, of its tail or of an index below it; a follower a heartbeat that
    carries a commit index; a candidate a vote response from a slot that has not answered.  timers (the move changed activity or
    elapsed, under CheckQuorum): one led group in three gets a MsgCheckQuorum instead, a follower a MsgVote of the next term."""
    s = ref.s
    n, me = s.N, s.self_peer
    others = _others(n, me)
    m = np.zeros(len(groups), pyoracle.STEP_MSG_DT)
    for i, g in enumerate(np.asarray(groups, np.int64)):
        p = int(rng.choice(others))
        role, term, li, co = int(s.role[g]), int(s.term[g]), int(s.last_index[g]), int(s.committed[g])
        if role == 2:
            if timers and rng.random() < 0.35:  # (a failed check deposes the leader: the others keep theirs for the moves to come)
                Q._rec(m, i, g, Q.MsgCheckQuorum)
            else:
                idx = li if rng.random() < 0.5 else int(rng.integers(min(co, li), li + 1))
                Q._rec(m, i, g, R.MsgAppResp, term=term, frm=p, index=idx)
        elif timers and (role == 0 or int(s.lead[g]) != 0):  # (the lease is whoever's that knows a leader)
            Q._rec(m, i, g, R.MsgVote, term=term + 1, frm=p, index=li + 5, log_term=term + 1)
        elif role == 1:
            free = [q for q in others if int(s.votes[q, g]) == 0]
            Q._rec(m, i, g, R.MsgVoteResp, term=term, frm=int(rng.choice(free)) if free else p, reject=int(rng.random() < 0.2))
        else:
            lead = int(s.lead[g])
            Q._rec(m, i, g, R.MsgHeartbeat, term=term, frm=lead - 1 if lead not in (0, me + 1) else p)
            m["commit"][i] = int(rng.integers(min(co, li), li + 1))
    return m


def random_records(ref, rng, n, keep_off, hot=None):
    """the case's random traffic over N_HOT groups outside `keep_off` (several records a group): tests/_stepgen.random_batch with two
    records in ten turned into MsgProps (ref_step_props.props_batch's way), one in twenty of the rest into a MsgCheckQuorum under
    CheckQuorum, and RAFTQ_MSGF_HOLD / RAFTQ_MSGF_SKIP on a few.  hot: a group that gets K_RUN of the records."""
    s = ref.s
    free = np.setdiff1d(np.arange(s.G), np.asarray(keep_off, np.int64))
    groups = rng.choice(free, min(N_HOT, len(free)), replace=False)
    m = _stepgen.random_batch(rng, s, n, hot_groups=groups)
    for at in np.flatnonzero(rng.random(n) < 0.2):
        g = int(m["group"][at])
        term = max(1, int(s.term[g]) + int(rng.integers(-1, 2))) if rng.random() < 0.125 else 0
        P._prop(m, at, g, int(rng.integers(1, P.MAX_ENTS + 1)) | (int(rng.integers(0, 2**31)) << 32), term=term, frm=int(rng.integers(0, s.N)))
    if ref.cq:
        for at in np.flatnonzero((m["type"] != P.MsgProp) & (rng.random(n) < 1 / 20)):
            Q._rec(m, at, int(m["group"][at]), Q.MsgCheckQuorum, frm=int(rng.integers(0, 256)))  # (`from` is ignored on a local kind)
    m = _stepgen.with_hold_skip(rng, m, 0.03, 0.03)
    if hot is not None:
        m["group"][np.flatnonzero((m["_pad"][:, 1] & V.MSGF_SKIP) == 0)[:K_RUN]] = hot
    return m


def follow_records_x(ref, groups, rng, kind):
    """follow_records for an extended case, with the records that read the new state put over it (the generators'
    shapes are ref_lead_transfer.step_case's, ref_read_index.step_case's and ref_pre_vote.step_case's):
      led, a transferee pending    a MsgProp, which must be dropped, or the transferee's acknowledgement of the tail (MsgTimeoutNow)
      led, ReadIndex               a local MsgReadIndex (numbered behind seq, released at the commit index -- at once under the
                                   lease), or a MsgHeartbeatResp whose context is one of the numbers handed out
      role 3                       a MsgPreVoteResp from a slot that has not answered: a grant at term + 1 or a rejection at the term
      followers, ReadIndex         a MsgReadIndex to forward, a context on the heartbeat to echo
    pv_off / pv_on: what tells the two apart needs no kind the window does not know -- a MsgHup (a pre-election with the switch, a
    campaign without) or a heartbeat of the term before (RAFTQ_OUT_TERM_RESP with the switch, nothing without)."""
    s = ref.s
    n, me = s.N, s.self_peer
    others = _others(n, me)
    m = follow_records(ref, groups, rng, timers=kind in TIMER_KINDS_X)
    window = kind in ("pv_off", "pv_on")
    for i, g in enumerate(np.asarray(groups, np.int64)):
        g = int(g)
        role, term, li = int(s.role[g]), int(s.term[g]), int(s.last_index[g])
        u, p = rng.random(), int(rng.choice(others))
        if role == 2:
            if int(m["type"][i]) == Q.MsgCheckQuorum:
                continue
            t = int(ref.transferee[g]) if ref.lt else 0
            if ref.lt and u < (0.7 if t else 0.35 if kind in TRANSFER_KINDS else 0.0):  # (none pending behind such a move: the MsgProp is taken)
                if u < 0.35 or t - 1 == me:
                    T._prop(m, i, g, 2, frm=p)
                else:
                    Q._rec(m, i, g, R.MsgAppResp, term=term, frm=t - 1, index=li)
            elif u < (0.7 if kind in READ_KINDS else 0.3):
                sq = int(ref.seq[g])
                if ref.ri == SAFE and sq > 0 and rng.random() < 0.5:
                    PV._rec(m, i, g, R.MsgHeartbeatResp, term=term, frm=p, index=int(rng.integers(1, sq + 1)))
                else:
                    PV._rec(m, i, g, RI.MsgReadIndex, frm=me)
        elif window or (role == PV.PRE and not ref.pv):
            if u < 0.5 or term < 2:
                PV._rec(m, i, g, R.MsgHup)
            else:
                PV._rec(m, i, g, R.MsgHeartbeat, term=term - 1, frm=p)
        elif role == PV.PRE:
            free = [q for q in others if int(s.votes[q, g]) == 0]
            grant = rng.random() < 0.7
            PV._rec(m, i, g, PV.MsgPreVoteResp, term=term + 1 if grant else term, frm=int(rng.choice(free)) if free else p, reject=0 if grant else 1)
        elif role == 0 and int(s.lead[g]) != 0 and u < 0.3:
            if int(m["type"][i]) == R.MsgHeartbeat:
                m["index"][i] = int(rng.integers(1, 7))
            else:
                PV._rec(m, i, g, RI.MsgReadIndex, frm=me)
    return m


def random_records_x(ref, rng, n, keep_off, hot=None):
    """random_records, then -- among the records Step looks at -- the kinds of the switches that are on, in the three generators'
    ways: half the MsgVote / MsgVoteResp records turned into their pre-election kinds; a small context on every MsgHeartbeat /
    MsgHeartbeatResp and one record in eight turned into a MsgReadIndex or MsgReadIndexResp; one in twelve into a
    MsgTransferLeader or MsgTimeoutNow (a MsgVote's reject byte, the transfer's mark, is drawn by _stepgen already)."""
    s = ref.s
    m = random_records(ref, rng, n, keep_off, hot=hot)
    plain = np.flatnonzero((m["_pad"][:, 1] & (V.MSGF_SKIP | V.MSGF_HOLD)) == 0)
    if ref.pv:
        turn = plain[rng.random(len(plain)) < 0.5]
        m["type"][turn] = np.where(m["type"][turn] == R.MsgVote, PV.MsgPreVote, np.where(m["type"][turn] == R.MsgVoteResp, PV.MsgPreVoteResp, m["type"][turn]))
    beats = plain[np.isin(m["type"][plain], (R.MsgHeartbeat, R.MsgHeartbeatResp))]
    m["index"][beats] = rng.integers(0, 7, len(beats))
    for i in plain[rng.random(len(plain)) < 1 / 8]:
        grp = int(m["group"][i])
        kind = RI.MsgReadIndex if rng.random() < 0.6 else RI.MsgReadIndexResp
        term = 0 if kind == RI.MsgReadIndex and rng.random() < 0.5 else max(1, int(s.term[grp]) + int(rng.choice([-1, 0, 0, 0, 1])))
        PV._rec(m, i, grp, kind, term=term, frm=int(rng.integers(0, s.N)), index=int(rng.integers(0, 50)))
    if ref.lt:
        for i in plain[rng.random(len(plain)) < 1 / 12]:
            grp = int(m["group"][i])
            kind = T.MsgTransferLeader if rng.random() < 0.5 else T.MsgTimeoutNow
            term = 0 if kind == T.MsgTransferLeader and rng.random() < 0.5 else max(1, int(s.term[grp]) + int(rng.choice([-1, 0, 0, 0, 1])))
            PV._rec(m, i, grp, kind, term=term, frm=int(rng.integers(0, s.N)))
    return m


def make_batch(ref, mv, rng, hot=None):
    """the records of the move's changed groups (the move's own, where it made some), the random traffic, shuffled: at most 1,024"""
    if ref.ext:
        follow, random_part = (lambda groups: follow_records_x(ref, groups, rng, mv.kind)), random_records_x
    else:
        follow, random_part = (lambda groups: follow_records(ref, groups, rng, timers=ref.cq and mv.kind in TIMER_KINDS)), random_records
    changed = np.asarray(mv.changed, np.int64)[:MAX_CHANGED]
    if mv.records is not None:
        forced = np.unique(mv.records["group"].astype(np.int64))
        rest = changed[~np.isin(changed, forced)][: MAX_CHANGED - len(mv.records)]
        own = np.concatenate([mv.records, follow(rest)])
    else:
        own = follow(changed)
    m = np.concatenate([own, random_part(ref, rng, N_RANDOM, own["group"][own["group"] < U(ref.s.G)], hot=hot)])
    assert len(m) <= 1024
    return np.ascontiguousarray(m[rng.permutation(len(m))])


TIMER_KINDS = ("tick", "activity", "cq_toggle", "roles")  # under CheckQuorum: the moves whose change Step reads through the lease or a check
TIMER_KINDS_X = TIMER_KINDS + ("tick_lists", "tick_frames", "tick_elect")
TRANSFER_KINDS = TIMER_KINDS_X + ("transfer", "lt_toggle", "clone")  # ... a transferee may be gone, or have come
# an extended case: the moves behind which a led group's read record, commit index or term gate may stand elsewhere
READ_KINDS = ("reads", "ri_toggle", "clone", "sweep", "cycle", "deltas", "term_deltas", "log_deltas", "log_deltas_nowait", "unmask", "remask", "voter_deltas")


# ---- the moves: each applies itself to `ref` and returns the Move (inputs, expected outputs, changed groups) ----------------------
def _led(ref):
    return np.flatnonzero(ref.s.role == 2)


def _match_deltas(ref, rng, k):
    s = ref.s
    led = _led(ref)
    g = rng.choice(led, min(k, len(led)), replace=False)
    p = _others(s.N, s.self_peer)[rng.integers(0, s.N - 1, len(g))]
    cur = s.match[p, g]
    li = np.maximum(s.last_index[g], cur)
    v = np.where(rng.random(len(g)) < 0.5, li, cur + ((li - cur) * rng.random(len(g))).astype(U)).astype(U)
    return g, p, v, g[v > cur]


def _vote_deltas(ref, rng, k):
    s = ref.s
    others = _others(s.N, s.self_peer)
    gs, ps = [], []
    for g in rng.permutation(np.flatnonzero(s.role == 1)):
        free = [q for q in others if int(s.votes[q, g]) == 0]
        if free and len(gs) < k:
            gs.append(int(g))
            ps.append(int(rng.choice(free)))
    gs, ps = np.array(gs, np.int64), np.array(ps, np.int64)
    return gs, ps, np.where(rng.random(len(gs)) < 0.8, 1, 2).astype(np.uint8)


def _advance(ref):
    """the adopted gated sweep on the reference -> (old, new, n_changed)"""
    s = ref.s
    if ref.voters is None:
        new, n = pyoracle.commit_advance(s.match, s.committed, True, s.first_idx)
    else:
        new, n = RV.commit_advance(s.match, s.committed, ref.voters, gated=True, first_idx=s.first_idx)
    old = s.committed.copy()
    s.committed[:] = new
    return old, new, n


def pending(ref):
    s = ref.s
    if ref.voters is None:
        return pyoracle.commit_advance(s.match, s.committed, True, s.first_idx)[1]
    return RV.commit_advance(s.match, s.committed, ref.voters, gated=True, first_idx=s.first_idx)[1]


def mv_deltas(ref, rng):
    g, p, v, changed = _match_deltas(ref, rng, 200)
    np.maximum.at(ref.s.match, (p, g), v)
    return Move("deltas", dict(group=g.astype(U), peer=p.astype(np.uint32), match=v), {}, changed)


def mv_vote_deltas(ref, rng):
    g, p, v = _vote_deltas(ref, rng, 200)
    ref.s.votes[:] = pyoracle.apply_vote_deltas(ref.s.votes, g.astype(U), p.astype(np.uint32), v)
    return Move("vote_deltas", dict(group=g.astype(U), peer=p.astype(np.uint32), vote=v), {}, g)


def mv_sweep(ref, rng):
    old, new, n = _advance(ref)
    at = np.flatnonzero(new != old)
    return Move("sweep", {}, dict(committed=new.copy(), n_changed=n, group=at.astype(U), old_commit=old[at], new_commit=new[at]), at)


def mv_cycle(ref, rng):
    """one raftq_cycle_packed turn: match deltas, vote deltas, the gated sweep with the tally, the segmented advance list"""
    s = ref.s
    g, p, v, ch = _match_deltas(ref, rng, 120)
    np.maximum.at(s.match, (p, g), v)
    vg, vp, vv = _vote_deltas(ref, rng, 60)
    s.votes[:] = pyoracle.apply_vote_deltas(s.votes, vg.astype(U), vp.astype(np.uint32), vv)
    old, new, n = _advance(ref)
    at = np.flatnonzero(new != old)
    _, won, lost = pyoracle.vote_tally(s.votes) if ref.voters is None else RV.vote_tally(s.votes, ref.voters)
    want = dict(group=at.astype(U), new_commit=new[at], advanced_by=(new[at] - old[at]).astype(np.uint32), total=len(at), counts=(n, won, lost))
    return Move("cycle", dict(group=g.astype(U), peer=p.astype(np.uint32), match=v, vgroup=vg.astype(U), vpeer=vp.astype(np.uint32), vote=vv),
                want, np.unique(np.concatenate([ch, vg, at])))


def mv_roles(ref, rng):
    """raftq_load_roles with about 50 flips, and the timers of 300 groups that are not led drawn anew on both sides of
    election_tick (so that the Ticks behind it have timers to fire); the activity words do not move.  Step reads elapsed under
    CheckQuorum alone (the lease): there the followers whose timer moved count as changed."""
    s = ref.s
    flip = rng.choice(s.G, 50, replace=False)
    old = s.role[flip].copy()
    s.role[flip] = (old + rng.integers(1, 3, len(flip))) % 3
    idle = np.flatnonzero(s.role != 2)
    redraw = rng.choice(idle, min(300, len(idle)), replace=False)
    s.elapsed[redraw] = rng.integers(0, 2 * ET, len(redraw))
    leased = redraw[(s.role[redraw] == 0) & (s.lead[redraw] != 0)] if ref.cq else redraw[:0]
    s.elapsed[leased[:30]] = ET - 1  # the next Tick ends their lease
    return Move("roles", dict(role=s.role.copy(), elapsed=s.elapsed.copy()), {}, np.unique(np.concatenate([flip, leased])))


def mv_campaign(ref, rng):
    s = ref.s
    pool = np.flatnonzero(s.role != 2)
    gs = np.sort(rng.choice(pool, min(60, len(pool)), replace=False)).astype(U)
    s.role[:], s.elapsed[:], s.votes[:] = pyoracle.campaign(s.role, s.elapsed, s.votes, gs, s.self_peer)
    return Move("campaign", dict(groups=gs), {}, gs.astype(np.int64))


def mv_term_deltas(ref, rng):
    s = ref.s
    led = _led(ref)
    g = rng.choice(led, min(150, len(led)), replace=False)
    fi = (1 + (s.last_index[g] * rng.random(len(g))).astype(U)).astype(U)
    old = s.first_idx[g].copy()
    s.first_idx[g] = fi
    return Move("term_deltas", dict(group=g.astype(U), cur_term=np.maximum(s.term[g], U(1)), first_idx=fi), {}, g[fi != old])


def _log_deltas(ref, rng, kind):
    s = ref.s
    g = rng.choice(s.G, 200, replace=False)
    li = s.last_index[g] + rng.integers(0, 3, len(g)).astype(U)
    lt = np.maximum(s.last_term[g], s.term[g] * (s.role[g] == 2))
    ct = np.where(s.role[g] == 2, 0, np.minimum(li, s.committed[g] + rng.integers(0, 3, len(g)).astype(U))).astype(U)
    was = (s.last_index[g].copy(), s.committed[g].copy())
    out = V.apply_log_deltas(s, ref.masks, g.astype(U), li, lt, ct)
    moved = (s.last_index[g] != was[0]) | (s.committed[g] != was[1])
    return Move(kind, dict(group=g.astype(U), last_index=li, last_term=lt, commit_to=ct), dict(committed=out), g[moved])


def mv_log_deltas(ref, rng):
    return _log_deltas(ref, rng, "log_deltas")


def mv_log_deltas_nowait(ref, rng):
    return _log_deltas(ref, rng, "log_deltas_nowait")


def mv_voter_deltas(ref, rng):
    """conf changes with resets: self keeps its vote, a reset names other slots; a few groups are named twice (the last record wins)"""
    s = ref.s
    n, me = s.N, s.self_peer
    g = rng.choice(s.G, 150, replace=False)
    g = np.concatenate([g, g[:20]])[rng.permutation(170)]
    new = (rng.integers(0, 1 << n, len(g)) | (1 << me)).astype(np.uint16)
    reset = np.where(rng.random(len(g)) < 0.4, rng.integers(0, 1 << n, len(g)) & ~(1 << me), 0).astype(np.uint16)
    s.match[:], s.votes[:], ref.voters = RV.apply_voter_deltas(s.match, s.votes, ref.voters, g.astype(U), new, reset)
    return Move("voter_deltas", dict(group=g.astype(U), voters=new, reset=reset), {}, np.unique(g))


def mv_unmask(ref, rng):
    """raftq_load_voters(h, NULL): the batch behind runs on the unmasked kernels"""
    part = np.flatnonzero(ref.voters != (1 << ref.s.N) - 1)
    ref.saved, ref.voters = ref.voters, None
    return Move("unmask", {}, {}, rng.permutation(part))


def mv_remask(ref, rng):
    ref.voters, ref.saved = ref.saved, None
    part = np.flatnonzero(ref.voters != (1 << ref.s.N) - 1)
    return Move("remask", dict(voters=ref.voters.copy()), {}, rng.permutation(part))


def _hup_check_records(hups, checks):
    m = np.zeros(len(hups) + len(checks), pyoracle.STEP_MSG_DT)
    for i, g in enumerate(hups):
        Q._rec(m, i, g, R.MsgHup)
    for i, g in enumerate(checks):
        Q._rec(m, len(hups) + i, g, Q.MsgCheckQuorum)
    return m


def mv_tick(ref, rng):
    """raftq_tick under CheckQuorum, with its three lists; the listed checks and MsgHups are stepped in the batch behind
    (ref_check_quorum_props.lockstep's way).  What Step can read of the move: a follower whose elapsed reached election_tick is out
    of lease now, a leader whose check passed has an empty activity word."""
    s = ref.s
    role0, el0, ac0 = s.role.copy(), s.elapsed.copy(), ref.active.copy()
    el, act, ac, le, nh, nb = Q.tick_array(pyoracle, s.role, s.elapsed, ref.active, ref.le, ref.voters, s.self_peer, s.N, ET, HB, SEED, ref.tick_no)
    s.elapsed[:], ref.active[:], ref.le[:] = el, ac, le
    ref.tick_no += 1
    hups, beats, checks = (np.flatnonzero(act == k) for k in (1, 2, 3))
    crossed = np.flatnonzero((role0 != 2) & (s.lead != 0) & (el0 < ET) & (el >= ET))
    cleared = np.flatnonzero((role0 == 2) & (ac0 != 0) & (ac == 0))
    want = dict(n_hup=nh, n_beat=nb, action=act, hups=hups.astype(U), beats=beats.astype(U), checks=checks.astype(U), crossed=len(crossed))
    return Move("tick", {}, want, np.concatenate([crossed, cleared, checks, hups]), records=_hup_check_records(hups[:200], checks[:200]))


def _tick_plain(ref):
    s = ref.s
    if ref.voters is None:
        el, act, nh, nb = pyoracle.tick(s.role, s.elapsed, ET, HB, SEED, ref.tick_no)
    else:
        el, act, nh, nb = TM.tick_array(pyoracle, s.role, s.elapsed, ref.voters, s.self_peer, ET, HB, SEED, ref.tick_no)
    s.elapsed[:] = el
    ref.tick_no += 1
    return act, np.flatnonzero(act == 1).astype(np.uint32), np.flatnonzero(act == 2).astype(np.uint32), nh, nb


def mv_tick_lists(ref, rng):
    act, hups, beats, nh, nb = _tick_plain(ref)
    return Move("tick_lists", {}, dict(n_hup=nh, n_beat=nb, action=act, hups=hups, beats=beats), hups.astype(np.int64),
                records=_hup_check_records(hups[:MAX_CHANGED], []))


def _positional(w, keep, n_max):
    if keep is None:
        stream, off = W.wire_encode(w) if len(w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        full = np.full(n_max + 1, len(stream), np.uint64)  # entries past the last frame all hold the total
        full[: len(off)] = off
        return np.asarray(stream), full, len(w)
    stream, full = TM.encode_members(w, keep, n_max)
    return np.asarray(stream), full, int(np.asarray(keep).sum())


def mv_tick_frames(ref, rng):
    """raftq_tick_frames: the Tick, its lists and every MsgBeat group's heartbeats (test_tick_frames_gpu.want_frames; over masks
    ref_tick_members.member_beats)"""
    from tests import test_tick_frames_gpu as TF

    s = ref.s
    act, hups, beats, nh, nb = _tick_plain(ref)
    if ref.voters is None:
        w, po = TF.want_frames(s, beats, s.G)
        keep = None
    else:
        w, keep, po = TM.member_beats(s, ref.voters, beats, s.G)
    stream, off, n_frames = _positional(w, keep, s.G * (s.N - 1))
    want = dict(n_hup=nh, n_beat=nb, action=act, hups=hups, beats=beats, stream=stream, off=off, peer_off=np.asarray(po, U), n_frames=n_frames)
    return Move("tick_frames", {}, want, hups.astype(np.int64), records=_hup_check_records(hups[:MAX_CHANGED], []))


def mv_tick_elect(ref, rng):
    """raftq_tick_elect_frames: the device campaigns for every MsgHup group (test_tick_elect_gpu.want_round; over masks
    ref_tick_members.member_beats and member_campaigns)"""
    from tests import test_tick_elect_gpu as TE

    s = ref.s
    n, me = s.N, s.self_peer
    act, hups, beats, nh, nb = _tick_plain(ref)
    if ref.voters is None:
        w, po, camp, built, _ = TE.want_round(s, hups, beats, s.G, s.G)
        keep = None
    else:
        bw, bkeep, bpo = TM.member_beats(s, ref.voters, beats, s.G)
        vw, vkeep, camp, built, _ = TM.member_campaigns(s, ref.voters, hups, s.G)
        w, keep = np.concatenate([bw, vw]), np.concatenate([bkeep, vkeep])
        po = np.zeros(2 * (n + 1), U)
        po[: n + 1] = bpo
        po[n + 1] = bpo[n]
        po[n + 2:] = bpo[n] + np.cumsum([0 if p == me else len(built) for p in range(n)]).astype(U)
    stream, off, n_frames = _positional(w, keep, 2 * s.G * (n - 1))
    want = dict(n_hup=nh, n_beat=nb, action=act, hups=hups, beats=beats, stream=stream, off=off, peer_off=np.asarray(po, U), n_frames=n_frames, camp=camp)
    return Move("tick_elect", {}, want, np.asarray(built, np.int64))


def mv_propose(ref, rng):
    """raftq_propose_frames under raftq_propose_set_forward: sound proposals on led groups (an append that moves no commit index),
    proposals on followed groups, which leave as MsgProp, and on groups that know no leader, which are dropped"""
    s = ref.s
    me = s.self_peer
    led = np.flatnonzero((s.role == 2) & (s.lead == me + 1))
    probe = np.zeros(len(led), RF.PROP_DT)
    probe["group"], probe["n_ents"] = led, 3
    led = led[B.propose_verdict(s, ref.masks, probe) == 0]
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0) & (s.lead != me + 1))
    lost = np.flatnonzero((s.role == 1) | ((s.role == 0) & (s.lead == 0)))
    pick = lambda a, k: rng.choice(a, min(k, len(a)), replace=False)  # noqa: E731
    groups = rng.permutation(np.concatenate([pick(led, 120), pick(fol, 60), pick(lost, 20)]))
    n = len(groups)
    props, pe_n = np.zeros(n, RF.PROP_DT), rng.integers(1, 4, n).astype(np.uint32)
    props["group"], props["n_ents"], props["ent_first"] = groups, pe_n, np.cumsum(pe_n) - pe_n
    pe = np.zeros(int(pe_n.sum()), RF.PROP_ENT_DT)
    pe["data_len"] = rng.integers(0, 90, len(pe))
    pe["type"][rng.random(len(pe)) < 0.15] = 1
    hm, he, hpool = _wiregen.random_msgs(rng, 30, big_every=0, ent_frac=0.2)
    hpool = np.frombuffer(bytes(hpool), np.uint8)
    pe["data_off"] = len(hpool) + np.cumsum(pe["data_len"]) - pe["data_len"]
    pool = np.concatenate([hpool, rng.integers(0, 256, int(pe["data_len"].sum()) + 1, dtype=np.uint8)])
    w = RF.want(s, ref.voters, props, pe, pool, hm, he)
    want = dict(stream=w["stream"], off=w["off"], n_msgs=len(hm) + w["n_frames"], n_ents=len(he) + len(pe), bytes=len(w["stream"]), outcomes=w["what"])
    return Move("propose", dict(props=props, pe=pe, pool=pool, hm=hm, he=he), want, groups[w["what"] == RF.APPENDED].astype(np.int64))


def mv_respond(ref, rng):
    """raftq_campaign on 20 followers, then raftq_step_frames_respond with an at-tail bitmap: candidates (the new ones among them) get
    the grants that their quorum lacks (the last one wins, the
    device answers with becomeLeader's broadcast), led groups at the tail a MsgProp frame and the acknowledgements that commit it,
    followers a MsgProp frame (forwarded: the host's) and a heartbeat"""
    s = ref.s
    n, me = s.N, s.self_peer
    others = [int(p) for p in _others(n, me)]
    masks = ref.masks
    rows = []
    # raftq_campaign right in front of the call: the lead walk then runs behind a writer that is not Step, and the wins of these
    # groups are wins only if it read their new role
    fresh = np.sort(rng.permutation(np.flatnonzero(s.role == 0))[:20]).astype(U)
    s.role[:], s.elapsed[:], s.votes[:] = pyoracle.campaign(s.role, s.elapsed, s.votes, fresh, me)
    for g in np.concatenate([fresh.astype(np.int64), rng.permutation(np.setdiff1d(np.flatnonzero(s.role == 1), fresh.astype(np.int64)))[:20]]):
        vot = [p for p in others if (int(masks[g]) >> p) & 1 and int(s.votes[p, g]) == 0]
        have = sum(1 for p in range(n) if (int(masks[g]) >> p) & 1 and int(s.votes[p, g]) == 1)
        need = bin(int(masks[g])).count("1") // 2 + 1 - have
        if 0 < need <= len(vot):
            rows += [dict(group=int(g), type=RP.MSG_VOTE_RESP, term=int(s.term[g]), **{"from": p}) for p in vot[:need]]
            rows.append(RP.ack(int(g), others[-1], int(s.term[g]), int(s.last_index[g]) + 1))
    led = rng.permutation(np.flatnonzero((s.role == 2) & (s.lead == me + 1)))
    tail = led[:40]
    for g in tail:
        t, li = int(s.term[g]), int(s.last_index[g])
        rows.append(RP.prop(int(g), others[0], [(0, b"abc"), (1, b"")]))
        rows += [RP.ack(int(g), p, t, li + 2) for p in others]
    for g in led[40:60]:  # not at the tail: the proposal is the host's
        rows.append(RP.prop(int(g), others[-1], [(0, b"z" * 70)]))
    for g in rng.permutation(np.flatnonzero((s.role == 0) & (s.lead != 0) & (s.lead != me + 1)))[:40]:
        rows.append(RP.prop(int(g), others[0], [(0, bytes(range(17)))]))
        rows.append(dict(group=int(g), type=RP.MSG_HB, term=int(s.term[g]), commit=int(s.last_index[g]), **{"from": int(s.lead[g]) - 1}))
    # the groups keep the order of their own frames; the groups are interleaved
    by_group = {}
    for r in rows:
        by_group.setdefault(r["group"], []).append(r)
    order = rng.permutation(np.repeat(list(by_group), [len(v) for v in by_group.values()]))
    rows = [by_group[int(g)].pop(0) for g in order]
    stream, off = RP.frames(rows, me, pad=5)
    at = B.leaders_bitmap(rng, s, 0.5) | RP.bitmap(s.G, tail)
    for g in led[40:60]:
        at[g >> 6] &= ~(U(1) << U(g & 63))
    if ref.cq:
        w = CP.want(s, ref.active, ref.le, stream, off, at, ref.voters, election_tick=ET)
    else:
        w = RP.want(s, stream, off, at, ref.voters)
    return Move("respond", dict(campaign=fresh, stream=stream, off=off, at_tail=at), w, np.array(sorted(by_group), np.int64))


def _sample(ref, rng):
    return rng.choice(ref.s.G, 200, replace=False)


def mv_clone(ref, rng):
    """raftq_clone_state into a second handle with the same switches, then raftq_load_roles, raftq_load_node and (CheckQuorum)
    raftq_load_activity; the run continues on the clone, whose tick number starts at 0"""
    ref.tick_no = 0
    return Move("clone", {}, {}, _sample(ref, rng))


def mv_narrow_rebuild(ref, rng):
    return Move("narrow_rebuild", {}, {}, _sample(ref, rng))


def mv_refused(ref, rng):
    """a Step batch with one record whose `from` is N or more: RAFTQ_EINVAL and nothing moved.  The record is an acknowledgement in
    one refused move of a schedule and a MsgProp in the other."""
    mv = Move("refused", {}, {}, _sample(ref, rng))
    bad = make_batch(ref, mv, rng)
    at = int(rng.integers(0, len(bad)))
    g = int(rng.choice(_led(ref)))
    if rng.random() < 0.5:
        Q._rec(bad, at, g, R.MsgAppResp, term=int(ref.s.term[g]), frm=ref.s.N, index=int(ref.s.last_index[g]))
    else:
        P._prop(bad, at, g, 2, frm=ref.s.N + 3)
    mv.args = dict(bad=bad, at=at)
    return mv


def mv_activity(ref, rng):
    """raftq_load_activity: other activity words and lead_elapsed in led groups"""
    full = (1 << ref.s.N) - 1
    led = _led(ref)
    g = rng.choice(led, min(200, len(led)), replace=False)
    old = ref.active[g].copy()
    ref.active[g] = np.where(rng.random(len(g)) < 0.5, full - old, rng.integers(0, full + 1, len(g))).astype(np.uint16)
    ref.le[g] = rng.integers(0, ET, len(g))
    return Move("activity", dict(active=ref.active.copy(), lead_elapsed=ref.le.copy()), {}, g[ref.active[g] != old])


def mv_cq_toggle(ref, rng):
    """raftq_set_check_quorum(h, 0) then (h, 1): both activity arrays come back zeroed"""
    ch = np.flatnonzero((ref.s.role == 2) & (ref.active != 0))
    ref.active[:], ref.le[:] = 0, 0
    return Move("cq_toggle", {}, {}, rng.permutation(ch))


# ---- the moves of an extended case -------------------------------------------------------------------------------------------------
def _holds_more(ref):
    """[G] bool: a transferee or a read record stands in the group"""
    return (ref.transferee != 0) | (ref.seq != 0) | (ref.acked != 0).any(axis=0)


def mv_roles_x(ref, rng):
    """mv_roles; under PreVote some of the groups that become candidates and know no leader become pre-candidates (role 3, what
    becomePreCandidate leaves).  A led group that holds a transferee or a read record keeps its role: only a leader holds either
    (ref_lead_transfer.tick_input, ref_read_index.step_case), and raftq_load_roles is no reset()."""
    s = ref.s
    pool = np.flatnonzero(~((s.role == 2) & _holds_more(ref)))
    flip = rng.choice(pool, 50, replace=False)
    new = ((s.role[flip] % 3) + rng.integers(1, 3, len(flip))) % 3
    if ref.pv:
        new[(new == 1) & (s.lead[flip] == 0) & (rng.random(len(flip)) < 0.6)] = PV.PRE
    s.role[flip] = new
    idle = np.flatnonzero(s.role != 2)
    redraw = rng.choice(idle, min(300, len(idle)), replace=False)
    s.elapsed[redraw] = rng.integers(0, 2 * ET, len(redraw))
    leased = redraw[(s.role[redraw] == 0) & (s.lead[redraw] != 0)]
    s.elapsed[leased[:30]] = ET - 1  # the next Tick ends their lease
    return Move("roles", dict(role=s.role.copy(), elapsed=s.elapsed.copy()), {}, np.unique(np.concatenate([flip, leased])))


def _tick_x(ref):
    """ref_lead_transfer.tick on the reference (ref_check_quorum.tick_array over the word's low half: a check that passes clears
    the transferee with the bits) -> (want, the groups whose change Step can read)"""
    s = ref.s
    role0, el0, ac0, tr0 = s.role.copy(), s.elapsed.copy(), ref.active.copy(), ref.transferee.copy()
    el, act, ac, le, tr, nh, nb = T.tick(pyoracle, s.role, s.elapsed, ref.active, ref.le, ref.transferee, ref.voters, s.self_peer, s.N, ET, HB, SEED,
                                         ref.tick_no)
    s.elapsed[:], ref.active[:], ref.le[:], ref.transferee[:] = el, ac, le, tr
    ref.tick_no += 1
    hups, beats, checks = (np.flatnonzero(act == k) for k in (1, 2, 3))
    crossed = np.flatnonzero((role0 != 2) & (s.lead != 0) & (el0 < ET) & (el >= ET))
    cleared = np.flatnonzero((role0 == 2) & (((ac0 != 0) & (ac == 0)) | ((tr0 != 0) & (tr == 0))))
    want = dict(n_hup=nh, n_beat=nb, action=act, hups=hups, beats=beats, checks=checks, crossed=len(crossed), aborted=int(((tr0 != 0) & (tr == 0)).sum()))
    return want, np.concatenate([crossed, cleared, checks])


def mv_tick_x(ref, rng):
    """mv_tick with the transferee in the word"""
    want, read = _tick_x(ref)
    hups, checks = want["hups"], want["checks"]
    want.update(hups=hups.astype(U), beats=want["beats"].astype(U), checks=checks.astype(U))
    return Move("tick", {}, want, np.concatenate([read, hups]), records=_hup_check_records(hups[:200], checks[:200]))


def _lists32(want):
    want.update({k: want[k].astype(np.uint32) for k in ("hups", "beats", "checks")})
    return want


def mv_tick_lists_x(ref, rng):
    """raftq_tick_collect_lists under raftq_tick_set_checks: the Tick and its three lists"""
    want, read = _tick_x(ref)
    hups, checks = want["hups"], want["checks"]
    return Move("tick_lists", {}, _lists32(want), np.concatenate([read, hups]), records=_hup_check_records(hups[:200], checks[:200]))


def mv_tick_frames_x(ref, rng):
    """raftq_tick_frames under raftq_tick_set_checks: the Tick, its three lists and the heartbeats of the MsgBeat groups, none of them
    a group whose check failed (ref_tick_checks.beats_round, as tests/test_tick_checks_gpu.py composes it)"""
    s = ref.s
    want, read = _tick_x(ref)
    hups, checks = want["hups"], want["checks"]
    w, keep, po = RC.beats_round(s, ref.voters, want["beats"].astype(np.uint32), s.G)
    stream, off = TM.encode_members(w, keep, s.G * (s.N - 1))
    want.update(stream=np.asarray(stream), off=off, peer_off=np.asarray(po, U), n_frames=int(np.asarray(keep).sum()))
    return Move("tick_frames", {}, _lists32(want), np.concatenate([read, hups]), records=_hup_check_records(hups[:200], checks[:200]))


def mv_tick_elect_x(ref, rng):
    """raftq_tick_elect_frames under raftq_tick_set_checks: ref_tick_checks.round_'s composition with the Tick above and the election
    round stepped by this case's Step -- MsgHup records of every MsgHup group: a campaign, whose reset() clears the activity word, or
    under PreVote a pre-election that moves no term"""
    s = ref.s
    n, me = s.N, s.self_peer
    want, read = _tick_x(ref)
    bw, bkeep, bpo = RC.beats_round(s, ref.voters, want["beats"].astype(np.uint32), s.G)
    vw, vkeep, camp, built, outs = RC.campaigns(s, ref.active, ref.le, ref.voters, want["hups"].astype(np.uint32), s.G, ref.pv, ET, step=ref.step)
    po = np.zeros(2 * (n + 1), U)
    po[: n + 1] = bpo
    po[n + 1] = bpo[n]
    po[n + 2:] = bpo[n] + np.cumsum([0 if p == me else len(built) for p in range(n)]).astype(U)
    keep = np.concatenate([bkeep, vkeep])
    stream, off = TM.encode_members(np.concatenate([bw, vw]), keep, 2 * s.G * (n - 1))
    want.update(stream=np.asarray(stream), off=off, peer_off=po, n_frames=int(keep.sum()), camp=camp, built=built, outs=outs)
    return Move("tick_elect", {}, _lists32(want), np.concatenate([read, built]), records=_hup_check_records([], want["checks"][:200]))


def mv_activity_x(ref, rng):
    """mv_activity; of the groups it rewrites, up to 12 that hold a transferee get every activity bit and lead_elapsed one short of
    the timeout: the next Tick's check falls due, passes and aborts their transfer.  The transferees themselves stand."""
    mv = mv_activity(ref, rng)
    due = mv.changed[ref.transferee[mv.changed] != 0][:12]
    ref.active[due], ref.le[due] = (1 << ref.s.N) - 1, ET - 1
    mv.args = dict(active=ref.active.copy(), lead_elapsed=ref.le.copy())
    return mv


def mv_transfer(ref, rng):
    """raftq_load_transfer: other transferees in about 150 led groups -- mostly another slot, sometimes none, seldom self"""
    s = ref.s
    n, me = s.N, s.self_peer
    led = _led(ref)
    g = rng.choice(led, min(150, len(led)), replace=False)
    old = ref.transferee[g].copy()
    u = rng.random(len(g))
    new = np.where(u < 0.2, 0, np.where(u < 0.25, me + 1, 1 + _others(n, me)[rng.integers(0, n - 1, len(g))])).astype(np.uint8)
    ref.transferee[g] = new
    return Move("transfer", dict(transferee=ref.transferee.copy()), {}, g[new != old])


def mv_reads(ref, rng):
    """raftq_load_reads: other read records in about 150 led groups, every acked word at most its group's seq"""
    n = ref.s.N
    led = _led(ref)
    g = rng.choice(led, min(150, len(led)), replace=False)
    old = (ref.seq[g].copy(), ref.acked[:, g].copy())
    ref.seq[g] = rng.integers(0, 7, len(g))
    ref.acked[:, g] = (rng.random((n, len(g))) * (ref.seq[g] + 1)[None, :]).astype(np.uint32)
    moved = (ref.seq[g] != old[0]) | (ref.acked[:, g] != old[1]).any(axis=0)
    return Move("reads", dict(seq=ref.seq.copy(), acked=ref.acked.copy()), {}, g[moved])


def mv_lt_toggle(ref, rng):
    """raftq_set_lead_transfer(h, 0) then (h, 1): every transferee is 0, the activity bits and lead_elapsed stand"""
    ch = np.flatnonzero(ref.transferee != 0)
    ref.transferee[:] = 0
    return Move("lt_toggle", {}, {}, rng.permutation(ch))


def mv_ri_toggle(ref, rng):
    """raftq_set_read_index to the other mode and back: the safe mode's records come back zeroed, everything else stands"""
    other = LEASE if ref.ri == SAFE else SAFE
    if ref.ri == LEASE:
        return Move("ri_toggle", dict(other=other), {}, _sample(ref, rng))
    ch = np.flatnonzero((ref.seq != 0) | (ref.acked != 0).any(axis=0))
    ref.seq[:], ref.acked[:] = 0, 0
    return Move("ri_toggle", dict(other=other), {}, rng.permutation(ch))


def _window_groups(ref, rng):
    pre = np.flatnonzero(ref.s.role == PV.PRE)
    rest = np.flatnonzero((ref.s.role != PV.PRE) & (ref.s.role != 2))
    return np.concatenate([rng.permutation(pre), rng.choice(rest, min(150, len(rest)), replace=False)])


def mv_pv_off(ref, rng):
    """raftq_set_pre_vote(h, 0): the batch behind runs without PreVote"""
    ref.pv = False
    return Move("pv_off", {}, {}, _window_groups(ref, rng))


def mv_pv_on(ref, rng):
    ref.pv = True
    return Move("pv_on", {}, {}, _window_groups(ref, rng))


def mv_tally_rebuild(ref, rng):
    return Move("tally_rebuild", {}, {}, _sample(ref, rng))


def mv_closed(ref, rng):
    """every call the case's switches close, tried once: each is refused with its word and moves nothing.  The raftq_propose_frames
    that a transfer closes gets sound proposals on three led groups."""
    led = _led(ref)[:3]
    props, pe = np.zeros(len(led), RF.PROP_DT), np.zeros(len(led), RF.PROP_ENT_DT)
    props["group"], props["n_ents"], props["ent_first"] = led, 1, np.arange(len(led))
    pe["data_len"], pe["data_off"] = 4, 4 * np.arange(len(led))
    args = dict(calls=closed_calls(ref.case), props=props, pe=pe, pool=np.arange(4 * len(led) + 1, dtype=np.uint8),
                hm=np.zeros(0, W.WIRE_MSG_DT), he=np.zeros(0, W.WIRE_ENT_DT))
    return Move("closed", args, {}, _sample(ref, rng))


MOVES_X = {"roles": mv_roles_x, "tick": mv_tick_x, "tick_lists": mv_tick_lists_x, "tick_frames": mv_tick_frames_x, "tick_elect": mv_tick_elect_x,
           "transfer": mv_transfer, "reads": mv_reads, "lt_toggle": mv_lt_toggle, "ri_toggle": mv_ri_toggle, "pv_off": mv_pv_off, "pv_on": mv_pv_on,
           "tally_rebuild": mv_tally_rebuild, "closed": mv_closed, "activity": mv_activity_x}


def move_fn(ref, kind):
    return MOVES_X[kind] if ref.ext and kind in MOVES_X else MOVES[kind]


MOVES = {f.__name__[3:]: f for f in (mv_deltas, mv_vote_deltas, mv_sweep, mv_cycle, mv_roles, mv_campaign, mv_term_deltas, mv_log_deltas,
                                     mv_log_deltas_nowait, mv_voter_deltas, mv_unmask, mv_remask, mv_tick, mv_tick_lists, mv_tick_frames,
                                     mv_tick_elect, mv_propose, mv_respond, mv_clone, mv_narrow_rebuild, mv_refused, mv_activity, mv_cq_toggle)}


def admissible(ref, kind):
    """the state holds what the move needs to change something"""
    s = ref.s
    if ref.ext:
        if kind in TICKS:  # a dry run: Step can read what the Tick moved, and the device's round has campaigns to build
            w = move_fn(ref, kind)(ref.copy(), np.random.default_rng(0)).want
            return w["crossed"] >= 3 and (kind != "tick_elect" or len(w["built"]) >= 4)
        if kind in ("transfer", "reads"):
            return int((s.role == 2).sum()) >= 32
        if kind == "lt_toggle":
            return int(((s.role == 2) & (ref.transferee != 0)).sum()) >= 16
        if kind == "ri_toggle":
            return ref.ri == LEASE or int(((s.role == 2) & (ref.seq != 0)).sum()) >= 16
        if kind == "pv_off":
            return int((s.role == PV.PRE).sum()) >= 8
        if kind == "pv_on":
            return False  # only right behind "pv_off"
    if kind in ("deltas", "cycle", "term_deltas", "activity"):
        return int((s.role == 2).sum()) >= 32
    if kind == "vote_deltas":
        return int((s.role == 1).sum()) >= 32
    if kind == "sweep":
        return pending(ref) >= 4
    if kind == "cq_toggle":
        return int(((s.role == 2) & (ref.active != 0)).sum()) >= 16
    if kind in TICKS:  # a dry run: timers fire (and, under CheckQuorum, Step can read what the Tick moved)
        if kind == "tick":  # (the followers that leave their lease are what a record reads for certain)
            return MOVES[kind](ref.copy(), np.random.default_rng(0)).want["crossed"] >= 3
        return len(_tick_plain(ref.copy())[1]) >= 8
    if kind == "remask":
        return False  # only right behind "unmask"
    return True


# what makes a kind admissible again when nothing that is left is: one more move of the feeding kind is put in front of it
FEEDER = {"sweep": "deltas", "vote_deltas": "campaign", "cq_toggle": "activity", "tick": "roles", "tick_lists": "roles", "tick_frames": "roles",
          "tick_elect": "roles", "deltas": "roles", "cycle": "roles", "term_deltas": "roles", "activity": "roles",
          "lt_toggle": "transfer", "ri_toggle": "reads", "transfer": "roles", "reads": "roles", "pv_off": "roles"}


# ---- a case's start and its schedule ----------------------------------------------------------------------------------------------
def start_of(case):
    c = CASES[case]
    n, me = c["n"], c["me"]
    rng = np.random.default_rng(SEEDS[c["schedule"]])
    s = P.props_state(rng, n, me, G)
    s.elapsed[:] = np.where(s.role == 2, 0, rng.integers(0, 2 * ET, G))
    full = (1 << n) - 1
    active = rng.integers(0, full + 1, G).astype(np.uint16) if c["cq"] else np.zeros(G, np.uint16)
    le = rng.integers(0, ET, G).astype(np.uint32) if c["cq"] else np.zeros(G, np.uint32)
    voters = B.propose_masks(rng, n, G, me, np.arange(G)) if c["masks"] else None  # self and one other slot vote everywhere
    ref = Ref(s, voters, c["cq"], active, le)
    if "pv" in c:
        _extend_start(ref, case, rng)
    return ref, rng


def _extend_start(ref, case, rng):
    """the three generators' starts: under PreVote every third candidate a pre-candidate; under transfer a transferee in one led
    group of three; in the safe mode a read record (seq up to 5, every acked word at most seq) in every led group"""
    c, s = CASES[case], ref.s
    n = s.N
    if c["pv"]:
        s.role[np.flatnonzero(s.role == 1)[::3]] = PV.PRE
    led = np.flatnonzero(s.role == 2)
    x = RI.zero_extra(G, n)
    if c["lt"]:
        x.transferee[led] = np.where(rng.random(len(led)) < 1 / 3, 1 + rng.integers(0, n, len(led)), 0)
    if c["ri"] == SAFE:
        x.seq[led] = rng.integers(0, 6, len(led))
        x.acked[:, led] = (rng.random((n, len(led))) * (x.seq[led] + 1)[None, :]).astype(np.uint32)
    ref.extend(case, x.transferee, x.seq, x.acked)


@functools.lru_cache(maxsize=None)
def _schedule(key):
    import time

    t0 = time.perf_counter()
    case = next(k for k, c in CASES.items() if c["schedule"] == key)
    ref, rng = start_of(case)
    start = ref.copy()
    left = kinds_of(case)
    total = sum(left.values())
    pairs = set(int(x) for x in rng.choice(total, 2, replace=False))  # the moves whose batch is a pipelined pair
    moves, force = [], None
    while sum(left.values()):
        can = [k for k, c in left.items() if c and admissible(ref, k)]
        if force or can:
            kind = force or can[int(rng.integers(0, len(can)))]
            left[kind] -= 1
        else:
            kind = FEEDER[next(k for k, c in left.items() if c)]
            if not admissible(ref, kind):
                kind = FEEDER.get(kind, "roles")
            assert len(moves) < 3 * total, ("the feeders do not help", left)
        force = FORCED.get(kind)
        before = ref.copy()
        mv = move_fn(ref, kind)(ref, rng)
        mv.before, mv.after = before, ref.copy()
        mv.changed = np.asarray(mv.changed, np.int64)
        if len(moves) in pairs:
            hot = int(rng.integers(0, G))
            plain = Move(mv.kind, changed=np.zeros(0, np.int64))
            which = int(rng.integers(0, 2))  # the long run in the first or in the second of the two
            mv.batches = [make_batch(ref, mv, rng, hot=hot if which == 0 else None), None]
            mv.wants = [ref.step(mv.batches[0])]
            mv.batches[1] = make_batch(ref, plain, rng, hot=hot if which == 1 else None)
            mv.wants.append(ref.step(mv.batches[1]))
        else:
            mv.batches = [make_batch(ref, mv, rng)]
            mv.wants = [ref.step(mv.batches[0])]
        mv.after_step = ref.copy()
        moves.append(mv)
    return Schedule(case, start, moves, time.perf_counter() - t0)


def schedule(case):
    return _schedule(CASES[case]["schedule"])


# ---- what the tests ask of a schedule ---------------------------------------------------------------------------------------------
def what_if(ref):
    """the RAFTQ_SWEEP_NO_ADOPT sweeps on a handle that stands where `ref` stands -> {gated: (committed', n_changed, changed ids)},
    and the tally's outcome"""
    s = ref.s
    out = {}
    for gated in (False, True):
        if ref.voters is None:
            new, n = pyoracle.commit_advance(s.match, s.committed, gated, s.first_idx if gated else None)
        else:
            new, n = RV.commit_advance(s.match, s.committed, ref.voters, gated=gated, first_idx=s.first_idx)
        out[gated] = (new, n, np.flatnonzero(new != s.committed))
    out["outcome"] = (pyoracle.vote_tally(s.votes) if ref.voters is None else RV.vote_tally(s.votes, ref.voters))
    return out


def discriminates(mv):
    """the records of the move's changed groups in the batch behind it, stepped on the state in FRONT of the move (groups are
    independent in Step: the records of other groups are left out) -> the changed groups in which a record differs"""
    m, want = mv.batches[0], mv.wants[0]
    mine = ((m["_pad"][:, 1] & V.MSGF_SKIP) == 0) & np.isin(m["group"], mv.changed.astype(U))
    if mv.before.ext:  # (pv_on: a kind the handle in front of the move would refuse the batch for tells nothing apart by its record)
        mine &= ~mv.before.unknown(m)
    got = mv.before.copy().step(np.ascontiguousarray(m[mine]))
    k = got.dtype.itemsize
    differs = (got.view(np.uint8).reshape(-1, k) != np.ascontiguousarray(want[mine]).view(np.uint8).reshape(-1, k)).any(axis=1)
    return np.unique(m["group"][mine][differs])


def case_rules(case):
    """-> [(reference, rule)] every Step rule the switches of an extended case enable: "ri" ref_read_index's (the lease mode keeps no
    record: 2 and 6 alone, ref_read_index.case_rules), "lt" ref_lead_transfer's, "pv" ref_pre_vote's"""
    c = CASES[case]
    rules = [("ri", r) for r in ((2, 6) if c["ri"] == LEASE else RI.RULES)]
    rules += [("lt", r) for r in T.RULES] if c["lt"] else []
    return rules + ([("pv", r) for r in PV_RULES] if c["pv"] else [])


def batches_changed_without(sch, which, rule, stop_at=None):
    """the schedule's batches stepped again, each from the state it was made for, with one rule left out -> how many of them give
    another record or leave another word of state (the per-rule floor of the features' own suites, applied to the schedules).
    stop_at: stop counting there.  The batch inside the pv_off window has no PreVote rule to leave out."""
    n = 0
    for mv in sch.moves:
        for j, (m, w) in enumerate(zip(mv.batches, mv.wants)):
            st = mv.after.copy()
            if j:
                st.step(mv.batches[0])
            if which == "pv" and not st.pv:
                continue
            if len(mv.batches) == 1:
                full = mv.after_step
            else:
                full = st.copy()
                full.step(m)
            got = st.step(m, **{which + "_out": frozenset({rule})})
            n += got.tobytes() != w.tobytes() or not st.same(full)
            if stop_at is not None and n >= stop_at:
                return n
    return n


def counts(sch):
    out = {}
    for mv in sch.moves:
        out[mv.kind] = out.get(mv.kind, 0) + 1
    return out
