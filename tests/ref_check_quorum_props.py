"""CheckQuorum beside the other Step switches (include/raftq_step.h "CheckQuorum" with raftq_step_set_props; include/raftq_wire.h
raftq_respond_set_lead / raftq_respond_set_props): ONE Step reference with both sets of arms -- tests/ref_check_quorum._CheckArms and
tests/ref_step_props._PropArms are cooperative mixins and compose as they stand, nothing is overridden here -- a batch driver in
the shape of ref_step_props.step_batch that carries the activity words, the reference of raftq_step_frames_respond over it
(ref_respond_props.expected run over this Step's results), and the generators of the inputs the GPU tests hand to the device:

  respond_case    ref_respond_props.random_case with elapsed on both sides of election_tick, random activity words and, planted in
                  front, what a random case rarely draws (a candidate's last grant, a higher-term MsgVote to a leader at the tail,
                  the same vote to a follower in and out of lease)
  props_case      ref_check_quorum.step_case's state under ref_step_props.props_batch's traffic: MsgProp and type 12 in one batch
  lockstep        Tick and Step alternating over one state, the checks and MsgHups the Tick raised stepped in the next batch
  lease_case      a heartbeat and a higher-term vote to one out-of-lease follower, in one batch and in two

Nothing in here runs the code under test.  TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_raft_py as R
from tests import ref_respond_props as RP
from tests import ref_step_props as P
from tests import ref_step_voters as V

MsgCheckQuorum = Q.MsgCheckQuorum
ELECTION_TICK = Q.ELECTION_TICK
TICK_SEED = 0x5EED  # raftq_set_timers' seed in every handle of the GPU tests, and the lockstep reference's


@dataclass
class CPRaft(Q._CheckArms, P._PropArms, R.Raft):
    pass


@dataclass
class CPVRaft(Q._CheckArms, P._PropArms, V.VRaft):
    pass


def from_node_state(s, g, mask, active, lead_elapsed, election_tick, leave_out=frozenset()):
    return Q.from_node_state(s, g, mask, active, lead_elapsed, election_tick, leave_out, classes=(CPRaft, CPVRaft))


def _word(r):
    return sum(1 << (p - 1) for p in r.active)


def step_batch(s, voters, active, lead_elapsed, msgs, frames=False, election_tick=ELECTION_TICK, leave_out=frozenset(), trace=None):
    """Step for every message, in order, with raftq_step_set_props and raftq_set_check_quorum on -> raftq_step_out_t[]; `s`,
    `active` and `lead_elapsed` move.  voters: the masks, or None for a handle without them.  A malformed batch raises ValueError
    and moves nothing.  trace (tests only): a uint16[n] that receives the group's activity word behind every record."""
    if P.malformed(msgs, s.G, s.N, frames).any() or (msgs["group"][(msgs["_pad"][:, 1] & V.MSGF_SKIP) == 0] >= s.G).any():
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
            r = rafts[g] = from_node_state(s, g, None if voters is None else voters[g], active[g], lead_elapsed[g], election_tick, leave_out)
            r.held = False
        if fl & V.MSGF_HOLD:
            r.held = True
            V._common(out[i], r, m)
            out[i]["type"] = V.OutHeld
        else:
            t = int(m["type"])
            local = t in (R.MsgHup, R.MsgBeat, MsgCheckQuorum)
            k = P.entry_count(m, frames)
            ent_term = 0 if t == P.MsgProp else int(m["reject_hint"])  # (a proposal's entries: their Term is not looked at)
            res = r.step(R.Message(type=t, frm=0 if local else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
                                   index=int(m["index"]), commit=int(m["commit"]), reject=bool(m["reject"]),
                                   entries=(ent_term,) * k if fl & V.MSGF_ENTRIES else None, barrier=bool(fl & V.MSGF_BARRIER)))
            V._common(out[i], r, m)
            if res.type == P.OutForward:
                out[i]["to"] = r.lead - 1  # the one result whose addressee is not the sender
            out[i]["type"], out[i]["index"], out[i]["log_term"], out[i]["reject"], out[i]["flags"] = res.type, res.index, res.log_term, res.reject, res.flags
        if trace is not None:
            trace[i] = _word(r)
    for g, r in rafts.items():
        V.to_node_state(r, s, g)
        active[g] = _word(r)
        lead_elapsed[g] = r.lead_elapsed
    return out


def want(st, active, lead_elapsed, s, off, at_tail, voters=None, tail_appends=True, lead=True, props=True, ents_cap=None,
         election_tick=ELECTION_TICK, leave_out=frozenset(), trace=False):
    """ref_respond_props.want over this module's Step: st, active and lead_elapsed MOVE.  -> its dict (+ "trace": the activity word
    behind every record, when asked for)"""
    tr = []

    def step(st, voters, rec):
        tr.append(np.zeros(len(rec), np.uint16) if trace else None)
        return step_batch(st, voters, active, lead_elapsed, rec, election_tick=election_tick, leave_out=leave_out, trace=tr[0])

    w = RP.want(st, s, off, at_tail, voters, tail_appends, lead, props, ents_cap, step=step)
    w["trace"] = tr[0]
    return w


def copy_triple(t):
    return V.copy_state(t[0]), t[1].copy(), t[2].copy()


# ---- raftq_step_frames_respond under the switch ---------------------------------------------------------------------------------
N_WINS, N_TAIL, N_LEASE = 6, 4, 4  # planted groups per kind


def respond_case(seed, N, me, n_frames, band=None, masked=False, hot=False, G=97):
    """ref_respond_props.random_case(...) with elapsed drawn from [0, 2 * ELECTION_TICK), random activity words and lead_elapsed
    below ELECTION_TICK; planted in front of its frames, in this order:
      N_WINS candidates one grant short of their quorum, activity word non-zero: the grant, then an MsgAppResp of the empty entry
      N_TAIL led groups with their at-tail bit set: a MsgVote of the next term (random_case's proposal and committing acks follow)
      N_LEASE followers of a peer with elapsed 0 and N_LEASE with elapsed past ELECTION_TICK: the same MsgVote of the next term
    -> ((state, active, lead_elapsed), voters | None, stream, frame_off, at_tail, plan): plan holds the planted frames' positions"""
    start, voters, stream, off, at = RP.random_case(seed, N, me, G=G, n_frames=n_frames, band=band, masked=masked, hot=hot)
    rng = np.random.default_rng(seed + 50000)
    s = start
    full = (1 << N) - 1
    s.elapsed[:] = rng.integers(0, 2 * ELECTION_TICK, G)
    active = rng.integers(0, full + 1, G).astype(np.uint16)
    lead_elapsed = rng.integers(0, ELECTION_TICK, G).astype(np.uint32)
    others = [p for p in range(N) if p != me]
    cands = np.flatnonzero(s.role == 1)[:N_WINS]
    led = np.flatnonzero(s.role == 2)
    tail = led[:N_TAIL]  # (random_case sets the at-tail bit of its first PLANT led groups and plants a proposal in them)
    fol = np.flatnonzero((s.role == 0) & (s.lead != 0))
    in_lease, out_lease = fol[:N_LEASE], fol[N_LEASE:2 * N_LEASE]
    assert len(cands) == N_WINS and len(fol) >= 2 * N_LEASE and all((int(at[g >> 6]) >> (g & 63)) & 1 for g in tail)
    if voters is not None:
        voters[np.concatenate([cands, tail])] = full
    s.elapsed[in_lease], s.elapsed[out_lease] = 0, ELECTION_TICK + 3
    rows, plan = [], {"grant": [], "ack": [], "tail_vote": [], "in_lease": [], "out_lease": []}
    q = N // 2 + 1
    for g in cands:
        order = [int(p) for p in rng.permutation(others)]
        s.votes[:, g] = 0
        s.votes[me, g] = 1
        s.votes[order[:q - 2], g] = 1
        active[g] = rng.integers(1, full + 1)
        granter, acker = order[q - 2], order[-1]
        plan["grant"].append(len(rows))
        rows.append(dict(group=int(g), type=RP.MSG_VOTE_RESP, term=int(s.term[g]), **{"from": granter}))
        plan["ack"].append((len(rows), acker))
        rows.append(RP.ack(int(g), acker, int(s.term[g]), int(s.last_index[g]) + 1))
    for key, groups in (("tail_vote", tail), ("in_lease", in_lease), ("out_lease", out_lease)):
        for g in groups:
            plan[key].append(len(rows))
            rows.append(dict(group=int(g), type=R.MsgVote, term=int(s.term[g]) + 1, index=int(s.last_index[g]) + 5, log_term=int(s.term[g]) + 1,
                             **{"from": others[-1]}))
    ps, poff = RP.frames(rows, me)
    stream2 = np.concatenate([ps, np.asarray(stream, np.uint8)])
    off2 = np.concatenate([poff[:-1], np.asarray(off, np.uint64) + np.uint64(len(ps))])
    return (s, active, lead_elapsed), voters, stream2, off2, at, plan


def lease_ignored(rec, outs):
    """the MsgVotes of a higher term that the lease swallowed: the term did not become the group's, nothing came back"""
    looked_at = (rec["_pad"][:, 1] & (V.MSGF_HOLD | V.MSGF_SKIP)) == 0
    return looked_at & (rec["type"] == R.MsgVote) & (rec["term"] > outs["term"]) & (outs["type"] == R.OutNone)


def respond_shows(start, w):
    """what a respond_case shows of the switch in the lead forms, read off the reference's own output -> dict of counts"""
    rec, o, ans, tr = w["rec"], w["outs"], w["answered"], w["trace"]
    ign = lease_ignored(rec, o)
    word = {}
    cleared = 0
    wins = set(w["wins"])
    for i in range(len(rec)):
        if int(o["type"][i]) == V.OutSkipped:
            continue
        g = int(rec["group"][i])
        before = word.get(g, int(start[1][g]))
        cleared += i in wins and before != 0 and int(tr[i]) == 0
        word[g] = int(tr[i])
    goes_on = 0
    for i in np.flatnonzero(ign):
        behind = np.flatnonzero(rec["group"][i + 1:] == rec["group"][i]) + i + 1
        goes_on += bool(ans[behind].any())
    return {"lease-ignored votes": int(ign.sum()), "answered wins that clear a non-zero word": int(cleared),
            "answered proposals": len(w["taken"]), "ignored votes inside a prefix that goes on": int(goes_on)}


RESPOND_FLOORS = {"lease-ignored votes": 5, "answered wins that clear a non-zero word": 4, "answered proposals": 8,
                  "ignored votes inside a prefix that goes on": 2}


def assert_planted(start, w, plan):
    """the planted exchanges, on the reference's own output: a planted win is answered on the device and leaves the activity word
    0, the acknowledgement behind it sets its sender's bit alone; the MsgVote to a leader at the tail is ignored (no frame, the term
    stays) and the proposal and a committing acknowledgement behind it are still answered; the same vote to a follower in lease is
    ignored, out of lease it is answered with a MsgVoteResp frame at the new term"""
    rec, o, ans, tr = w["rec"], w["outs"], w["answered"], w["trace"]
    won = np.zeros(len(rec), bool)
    won[w["wins"]] = True
    took = np.zeros(len(rec), bool)
    took[w["taken"]] = True
    for i, (j, p) in zip(plan["grant"], plan["ack"]):
        assert int(o["type"][i]) == R.OutBecameLeader and won[i] and ans[i] and int(tr[i]) == 0, ("a planted win", i, o[i])
        assert int(start[1][int(rec["group"][i])]) != 0
        assert int(o["type"][j]) == R.OutProgress and int(tr[j]) == 1 << p, ("the ack behind the win", j, int(tr[j]), p)
    for i in plan["tail_vote"]:
        g = rec["group"][i]
        assert int(o["type"][i]) == R.OutNone and not ans[i] and int(o["term"][i]) == int(start[0].term[g]) and int(o["role"][i]) == 2
        behind = np.flatnonzero(rec["group"] == g)
        behind = behind[behind > i]
        assert took[behind].any(), ("no answered proposal behind the ignored vote", i)
        assert (ans[behind] & (rec["type"][behind] == RP.MSG_APP_RESP) & ((o["flags"][behind] & R.FlagCommitted) != 0)).any(), ("no commit broadcast", i)
    for i in plan["in_lease"]:
        assert int(o["type"][i]) == R.OutNone and not ans[i] and int(o["term"][i]) == int(start[0].term[rec["group"][i]])
    for i in plan["out_lease"]:
        assert int(o["type"][i]) == R.OutVoteResp and ans[i] and int(o["term"][i]) == int(start[0].term[rec["group"][i]]) + 1


def respond_case_list():
    """the arguments of every respond_case the GPU tests run: N = 3, 5 (over masks) and 9, a case with more than kMaxRun = 32 frames
    of one group in plain and masked form, one case lifted into the top band and one into b32"""
    return {"n3": dict(seed=10100, N=3, me=1, n_frames=400), "n5-masked": dict(seed=10101, N=5, me=4, n_frames=600, masked=True),
            "n9": dict(seed=10102, N=9, me=0, n_frames=600), "hot": dict(seed=10103, N=3, me=1, n_frames=400, hot=True),
            "hot-masked": dict(seed=10104, N=5, me=4, n_frames=600, masked=True, hot=True),
            "top": dict(seed=10105, N=3, me=1, n_frames=400, band="top"), "b32": dict(seed=10106, N=5, me=4, n_frames=600, band="b32", masked=True)}


# ---- proposals through raftq_step_batch under the switch ------------------------------------------------------------------------
G, N_MSGS, PLANT = Q.G, Q.N_MSGS, Q.PLANT


def props_case(n, self_peer, seed, masks=False, hot=False, g=G, n_msgs=N_MSGS):
    """ref_check_quorum.step_case's state (ref_step_props.props_state's dealt roles, elapsed on both sides of election_tick, random
    activity words) under ref_step_props.props_batch's traffic with one record in seven of its random part turned into a
    MsgCheckQuorum; in front, PLANT groups of each kind:
      led, no bit set      a check (fails for N > 1), a MsgProp from a peer, a MsgProp from self: neither is taken
      led, every bit set   a check (passes), a MsgProp (taken: no activity), a second check (fails for N > 1)
    `hot`: a led group gets 40 records of the random part (a run longer than the list walk takes).
    -> ((state, active, lead_elapsed) at the start, voters | None, batch, the reference's records, the triple after, plan)"""
    rng = np.random.default_rng(seed)
    s = P.props_state(rng, n, self_peer, g)
    s.elapsed[:] = rng.integers(0, 2 * ELECTION_TICK, g)
    full = (1 << n) - 1
    active = rng.integers(0, full + 1, g).astype(np.uint16)
    lead_elapsed = rng.integers(0, ELECTION_TICK, g).astype(np.uint32)
    voters = None
    if masks:
        voters = rng.integers(0, full + 1, g).astype(np.uint16) | np.uint16(1 << self_peer)
    led = np.flatnonzero(s.role == 2)
    pending = led[(s.committed[led] == 0) & (s.match[:, led] == s.last_index[led][None, :]).all(axis=0)]
    free = np.setdiff1d(led, pending)[P.PLANT:]  # (props_batch plants in the pending ones and in the first PLANT of the others)
    assert len(free) >= 2 * PLANT + 1, len(free)
    empty, fullset, hot_group = free[:PLANT], free[PLANT:2 * PLANT], int(free[2 * PLANT])
    active[empty], active[fullset] = 0, full
    if masks:
        voters[np.concatenate([empty, fullset])] = full
    other = (self_peer + 1) % n
    front = np.zeros(6 * PLANT, pyoracle.STEP_MSG_DT)
    plan = {"empty": [], "full": []}
    at = 0
    for grp in empty:
        plan["empty"].append(at)
        Q._rec(front, at, grp, MsgCheckQuorum)
        P._prop(front, at + 1, grp, 2, frm=other)
        P._prop(front, at + 2, grp, 1, frm=self_peer)
        at += 3
    for grp in fullset:
        plan["full"].append(at)
        Q._rec(front, at, grp, MsgCheckQuorum)
        P._prop(front, at + 1, grp, 3, frm=other)
        Q._rec(front, at + 2, grp, MsgCheckQuorum)
        at += 3
    body = P.props_batch(rng, s, n_msgs - len(front), hot=hot_group if hot else None)
    m = np.concatenate([front, body])
    rest = np.arange(len(front) + P.N_FRONT, n_msgs)  # behind props_batch's own planted records
    for i in rest[rng.random(len(rest)) < 1 / 7]:
        Q._rec(m, i, int(m["group"][i]), MsgCheckQuorum, frm=int(rng.integers(0, 256)))  # (`from` is ignored on a local kind)
    start = (V.copy_state(s), active.copy(), lead_elapsed.copy())
    want_o = step_batch(s, voters, active, lead_elapsed, m)
    for a in (m, want_o):
        a.setflags(write=False)
    return start, voters, m, want_o, (s, active, lead_elapsed), plan


def assert_props_planted(start, m, o, plan, n):
    for i in plan["empty"]:
        g = int(m["group"][i])
        down = n > 1
        assert bool(int(o["flags"][i]) & R.FlagSteppedDown) == down and int(o["role"][i]) == (0 if down else 2), ("the failing check", i, o[i])
        if down:
            assert (o["type"][i + 1:i + 3] == R.OutNone).all() and (o["last_index"][i + 1:i + 3] == start[0].last_index[g]).all(), ("a deposed leader took a proposal", i)
        assert (m["type"][i + 1:i + 3] == P.MsgProp).all() and int(m["from"][i + 2]) == start[0].self_peer
    for i in plan["full"]:
        g = int(m["group"][i])
        assert int(o["flags"][i]) == 0 and int(o["role"][i]) == 2, ("the passing check", i, o[i])
        assert int(o["type"][i + 1]) == P.OutProposed and int(o["last_index"][i + 1]) == int(start[0].last_index[g]) + 3, ("the proposal behind it", i)
        assert bool(int(o["flags"][i + 2]) & R.FlagSteppedDown) == (n > 1), ("the second check", i, o[i + 2])


def props_case_list():
    cases = []
    for n, me in ((3, 0), (5, 4)):
        cases.append(dict(n=n, self_peer=me, seed=10200 + n))
        cases.append(dict(n=n, self_peer=me, seed=10210 + n, masks=True))
    cases.append(dict(n=3, self_peer=1, seed=10220, hot=True))
    return cases


def malformed_beside_a_check(m):
    """a copy of the batch in which the LAST MsgProp carries no entries: it fails the batch; the type-12 records in front stay valid"""
    m = np.array(m)
    i = int(np.flatnonzero((m["type"] == P.MsgProp) & ((m["_pad"][:, 1] & V.MSGF_ENTRIES) != 0))[-1])
    assert (m["type"][:i] == MsgCheckQuorum).any()
    m["_resv"][i] = 0
    return m


# ---- Tick and Step in lockstep --------------------------------------------------------------------------------------------------
LOCK_G, LOCK_ET, LOCK_HT, LOCK_MSGS = 300, 3, 1, 512
LOCK_SHAPES = {"n3": dict(n=3, self_peer=0, masks=False, seed=10300), "n5-masked": dict(n=5, self_peer=4, masks=True, seed=10301)}
LOCK_FLOORS = {"step-downs by a check": 3, "lease-ignored votes": 20, "wins": 5}


def lockstep(n, self_peer, masks, seed, tick_seed=TICK_SEED, g=LOCK_G, et=LOCK_ET, ht=LOCK_HT, n_msgs=LOCK_MSGS, rounds=None):
    """4 * et rounds of raftq_tick then raftq_step_batch over ONE state: the reference's elapsed after the Tick is what its Step
    reads, its elapsed after Step what the next Tick reads.  A round's batch is tests/_stepgen.random_batch on the state behind its
    Tick with one MsgCheckQuorum for every group the Tick marked 3 and one MsgHup for every group it marked 1, at random positions.
    -> ((state, active, lead_elapsed) at the start, voters | None, [per round: dict(tick=(elapsed, action, active, lead_elapsed,
    n_hup, n_beat) behind the Tick, before=the triple the Step starts from, m, want, after=the triple behind the Step)])"""
    rng = np.random.default_rng(seed)
    s = _stepgen.random_state(rng, g, n, self_peer)
    full = (1 << n) - 1
    active = rng.integers(0, full + 1, g).astype(np.uint16)
    lead_elapsed = rng.integers(0, et, g).astype(np.uint32)
    voters = (rng.integers(0, full + 1, g).astype(np.uint16) | np.uint16(1 << self_peer)) if masks else None  # self votes everywhere
    start = (V.copy_state(s), active.copy(), lead_elapsed.copy())
    out = []
    for t in range(4 * et if rounds is None else rounds):
        el, act, ac, le, n_hup, n_beat = Q.tick_array(pyoracle, s.role, s.elapsed, active, lead_elapsed, voters, self_peer, n, et, ht, tick_seed, t)
        s.elapsed[:], active[:], lead_elapsed[:] = el, ac, le
        m = _stepgen.random_batch(rng, s, n_msgs)
        chk, hup = np.flatnonzero(act == 3), np.flatnonzero(act == 1)
        assert len(chk) + len(hup) <= n_msgs // 2
        pos = rng.choice(n_msgs, len(chk) + len(hup), replace=False)
        for i, grp in zip(pos[:len(chk)], chk):
            Q._rec(m, i, grp, MsgCheckQuorum)
        for i, grp in zip(pos[len(chk):], hup):
            Q._rec(m, i, grp, R.MsgHup)
        before = (V.copy_state(s), active.copy(), lead_elapsed.copy())
        want_o = step_batch(s, voters, active, lead_elapsed, m, election_tick=et)
        out.append(dict(tick=(el, act, ac, le, n_hup, n_beat), before=before, m=m, want=want_o, after=(V.copy_state(s), active.copy(), lead_elapsed.copy())))
    return start, voters, out


def lockstep_shows(rounds):
    """counted over the second half of the rounds, on the reference's own output"""
    got = dict.fromkeys(LOCK_FLOORS, 0)
    for r in rounds[len(rounds) // 2:]:
        m, o = r["m"], r["want"]
        got["step-downs by a check"] += int(((m["type"] == MsgCheckQuorum) & ((o["flags"] & R.FlagSteppedDown) != 0)).sum())
        got["lease-ignored votes"] += int(lease_ignored(m, o).sum())
        got["wins"] += int((o["type"] == R.OutBecameLeader).sum())
    return got


# ---- the lease behind a reset of the same batch ---------------------------------------------------------------------------------
def lease_case(long_runs, n=3, self_peer=0, k=8):
    """Followers of slot 1 at term 4 with elapsed past ELECTION_TICK (out of lease), in three sets of k groups:
      one batch     MsgHeartbeat of the term (elapsed = 0), then a MsgVote of term 5: in lease by the reset of this batch, ignored
      two batches   the heartbeat in the first, the vote in the second, submitted back to back: ignored
      control       the vote alone: answered
    and two groups that are never in lease, elapsed 0: a follower without a leader and a candidate -- the vote is answered.
    long_runs: the first group of each set gets 33 more heartbeats in the batch that holds its vote.  A run longer than kMaxRun = 32
    stalls the list walk, which then applies nothing of its batch: that batch and every batch in flight behind it are replayed
    through the sorted walk, one after the other.  Without the long runs no group has more than two records in a batch: both
    batches go through the list walk, and two submitted back to back are two list walks in flight.
    -> ((state, active, lead_elapsed), [batch 1, batch 2], sets: dict of group arrays)"""
    g = 3 * k + 2
    s = pyoracle.NodeState(g, n, self_peer)
    s.term[:], s.lead[:], s.last_index[:], s.last_term[:], s.elapsed[:] = 4, 2, 6, 4, ELECTION_TICK + 2
    s.match[self_peer] = 6
    sets = {"one batch": np.arange(k), "two batches": np.arange(k, 2 * k), "control": np.arange(2 * k, 3 * k), "no leader": np.array([3 * k]),
            "candidate": np.array([3 * k + 1])}
    s.lead[3 * k], s.elapsed[3 * k] = 0, 0
    s.role[3 * k + 1], s.lead[3 * k + 1], s.vote[3 * k + 1], s.votes[self_peer, 3 * k + 1], s.elapsed[3 * k + 1] = 1, 0, self_peer + 1, 1, 0
    from raftsql_amd import step as S

    def hb(groups):
        return S.pack_msgs(np.asarray(groups, np.uint64), R.MsgHeartbeat, term=4, frm=1)

    def vote(groups):
        return S.pack_msgs(np.asarray(groups, np.uint64), R.MsgVote, term=5, frm=2, index=9, log_term=5)

    long_ = lambda grp: hb(np.full(33 if long_runs else 0, grp))  # noqa: E731
    a, b, c = sets["one batch"], sets["two batches"], sets["control"]
    b1 = np.concatenate([hb(a), long_(a[0]), hb(b), vote(a), vote(c[:1]), long_(c[0]), vote(c[1:]), vote(sets["no leader"]), vote(sets["candidate"])])
    b2 = np.concatenate([vote(b), long_(b[0])])  # (the vote in front: nothing of ITS batch has reset elapsed)
    return (s, np.zeros(g, np.uint16), np.zeros(g, np.uint32)), [b1, b2], sets
