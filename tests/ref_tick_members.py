"""The reference of Tick and its two device-built rounds over each group's own members (raftq_tick_set_voters, include/raftq.h
"batched Tick", include/raftq_wire.h): upstream's promotable() in tickElection, bcastHeartbeat and campaign ranging over r.prs.

The Tick is stated twice -- array-shaped on top of oracle.pyoracle.tick, and as a per-group loop that restates tickElection /
tickHeartbeat with the oracle's draw -- and tests/test_tick_members_ref.py holds the two against each other.  The rounds are
built from what the suite already trusts: test_tick_frames_gpu.want_frames filtered by mask, ref_step_voters.step_batch on the
MsgHup messages, oracle.pywire.wire_encode's offsets spread over the positional slots.
TEST INFRASTRUCTURE: nothing in the product imports it."""
import numpy as np

from oracle import pywire as W
from tests import ref_step_voters as V

MSG_HUP, MSG_VOTE = 0, 5
OUT_CAMPAIGN, OUT_BECAME_LEADER = 3, 4
OUTF_HARDSTATE, OUTF_COMMITTED, OUTF_ANSWERED = 0x01, 0x02, 0x10
LEADER = 2


def mine_of(voters, self_peer: int) -> np.ndarray:
    """-> bool [G]: this node votes in group g (promotable(): `_, ok := r.prs[r.id]`)"""
    return ((np.asarray(voters, np.uint16).astype(np.uint32) >> np.uint32(self_peer)) & 1).astype(bool)


def tick_array(oracle, role, elapsed, voters, self_peer, election_tick, heartbeat_tick, seed, tick_no):
    """oracle.tick, then action 0 and elapsed 0 wherever the group is not led and self's bit is clear.  Exact: groups are
    independent and the draw is a function of (seed, tick, group) -> (elapsed' u32, action u8, n_hup, n_beat)"""
    el, act, _, _ = oracle.tick(role, elapsed, election_tick, heartbeat_tick, seed, tick_no)
    idle = (np.asarray(role) != LEADER) & ~mine_of(voters, self_peer)
    act = np.where(idle, 0, act).astype(np.uint8)
    el = np.where(idle, 0, el).astype(np.uint32)
    return el, act, int((act == 1).sum()), int((act == 2).sum())


def tick_scalar(oracle, role, elapsed, voters, self_peer, election_tick, heartbeat_tick, seed, tick_no):
    """upstream, group by group:
        tickElection:  if !r.promotable() { r.elapsed = 0; return }
                       r.elapsed++; if r.isElectionTimeout() { r.elapsed = 0; r.Step(MsgHup) }
        isElectionTimeout: d := r.elapsed - r.electionTimeout; if d < 0 { return false }; return d > rand % electionTimeout
        tickHeartbeat: r.elapsed++; if r.elapsed >= r.heartbeatTimeout { r.elapsed = 0; r.Step(MsgBeat) }
    with rand = the oracle's draw for (seed, tick, group)"""
    G = len(role)
    el = np.asarray(elapsed, np.uint32).copy()
    act = np.zeros(G, np.uint8)
    for g in range(G):
        if int(role[g]) == LEADER:
            e = int(el[g]) + 1
            if e >= heartbeat_tick:
                e, act[g] = 0, 2
            el[g] = e
            continue
        if not (int(voters[g]) >> self_peer) & 1:
            el[g] = 0
            continue
        e = int(el[g]) + 1
        d = e - election_tick
        if d >= 0 and d > oracle.tick_rand(seed, tick_no, g) % election_tick:
            e, act[g] = 0, 1
        el[g] = e
    return el, act, int((act == 1).sum()), int((act == 2).sum())


def _slots(voters, built, n_peers, self_peer, allowed=None):
    """-> bool [(N - 1) * len(built)], peer-major: the slot's peer is a member of its group (and the group is in `allowed`)"""
    v = np.asarray(voters, np.uint16).astype(np.uint32)[np.asarray(built, np.int64)]
    rows = [((v >> np.uint32(p)) & 1).astype(bool) & (True if allowed is None else allowed) for p in range(n_peers) if p != self_peer]
    return np.concatenate(rows) if rows else np.zeros(0, bool)


def member_beats(st, voters, beats, beat_cap):
    """the heartbeat round over members -> (every positional record, keep [slots] bool, peer_off): want_frames' records, of which
    only those to a member of their group are sent"""
    from tests import test_tick_frames_gpu as TF

    w, po = TF.want_frames(st, beats, beat_cap)
    built = np.asarray(beats[:beat_cap], np.int64)
    return w, _slots(voters, built, st.N, st.self_peer), po


def member_campaigns(st, voters, hups, hup_cap):
    """the election round over voters (st MOVES: the campaigns are stepped by the masked statement of Step) ->
    (every positional vote record, keep [slots] bool, camp records, campaigned ids, the raw 64-byte results)"""
    from raftsql_amd import step as S

    N, me = st.N, st.self_peer
    built = np.asarray(hups[:hup_cap], np.int64)
    outs = V.step_batch(st, voters, S.pack_msgs(built.astype(np.uint64), MSG_HUP)) if len(built) else np.zeros(0, S.OUT_DT)
    assert np.isin(outs["type"], (OUT_CAMPAIGN, OUT_BECAME_LEADER)).all(), "Step(MsgHup) of a non-leader campaigns"
    camp = np.zeros(len(built), S.OUT_S_DT)
    for k in ("term", "index", "vote", "lead", "type", "reject", "role"):
        camp[k] = outs[k]
    is_camp = outs["type"] == OUT_CAMPAIGN
    camp["commit"] = np.where(is_camp, outs["log_term"], outs["commit"])  # the 32-byte record carries a campaign's lastTerm there
    camp["flags"] = outs["flags"] | np.where(is_camp, OUTF_ANSWERED, 0).astype(np.uint8)  # ANSWERED for CAMPAIGN records only
    recs = []
    for p in range(N):
        if p == me:
            continue
        w = np.zeros(len(built), W.WIRE_MSG_DT)
        w["group"], w["type"], w["to"], w["from"] = built, MSG_VOTE, p, me
        w["term"], w["index"], w["log_term"] = outs["term"], outs["index"], outs["log_term"]
        recs.append(w)
    w = np.concatenate(recs) if recs else np.zeros(0, W.WIRE_MSG_DT)
    return w, _slots(voters, built, N, me, allowed=is_camp), camp, built, outs


def encode_members(w, keep, n_max):
    """the member records alone through the wire oracle, their offsets spread over the positional slots ->
    (stream u8, frame_off u64 [n_max + 1]: a non-member's slot has zero length, the entries past the last slot hold the total)"""
    keep = np.asarray(keep, bool)
    sent = w[keep]
    stream, dense = W.wire_encode(sent) if len(sent) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    at = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)  # member records in front of slot k
    full = np.full(n_max + 1, dense[-1], np.uint64)
    full[: len(at)] = np.asarray(dense, np.uint64)[at]
    return stream, full


def peer_bytes(stream, full_off, peer_off, p):
    """peer p's bytes: out[frame_off[peer_off[p]] .. frame_off[peer_off[p + 1]])"""
    return bytes(stream[int(full_off[int(peer_off[p])]): int(full_off[int(peer_off[p + 1])])])


def hand_masks(n: int, self_peer: int) -> np.ndarray:
    """the masks added by hand: empty, full, {self} alone, self absent"""
    full = (1 << n) - 1
    return np.array([0, full, 1 << self_peer, full & ~(1 << self_peer)], np.uint16)
