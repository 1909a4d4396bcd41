"""The masked statement of Step (include/raftq_step.h raftq_step_set_voters): tests/ref_raft_py.Raft with a voter set.  Upstream's
`prs` map IS the membership; here the map keeps all N slots (a non-voter's Match and vote are stored and read as always) and a
separate set says who counts.  Overridden: q, maybe_commit, poll and the candidate's rejection count -- nothing else.

Also: a batch driver over an oracle.pyoracle.NodeState plus masks (messages in order, `held` cleared per batch, 64-byte result
records and the state written back), the tail reports (raftq_apply_log_deltas), and the two directed inputs whose outcome
depends on the masks.  TEST INFRASTRUCTURE: nothing in the product imports it."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle
from tests import ref_raft_py as R

OutSkipped, OutHeld = 10, 11
MSGF_ENTRIES, MSGF_BARRIER, MSGF_HOLD, MSGF_SKIP = 0x80, 0x40, 0x20, 0x10


@dataclass
class VRaft(R.Raft):
    voters: frozenset = frozenset()  # raft IDs (1-based) that vote in this group

    def q(self) -> int:
        return len(self.voters) // 2 + 1

    def maybe_commit(self) -> bool:
        mis = sorted((pr.match for p, pr in self.prs.items() if p in self.voters), reverse=True)
        mci = mis[self.q() - 1] if mis else 0  # an empty mask: candidate 0, nothing commits
        term_ok = self.first_index_of_term != 0 and mci >= self.first_index_of_term
        if mci > self.committed and term_ok:
            self.committed = mci
            return True
        return False

    def poll(self, frm: int, v: bool) -> int:
        if frm not in self.votes:  # every sender's first response is recorded, voter or not
            self.votes[frm] = v
        return sum(1 for p, g in self.votes.items() if g and p in self.voters)

    def step_candidate(self, m: R.Message) -> R.Result:
        if m.type != R.MsgVoteResp:
            return super().step_candidate(m)
        gr = self.poll(m.frm, not m.reject)
        if self.q() == gr:
            self.become_leader()
            return R.Result(R.OutBecameLeader, self.last_index, self.last_term)
        if self.q() == sum(1 for p in self.votes if p in self.voters) - gr:  # the voters' rejections
            self.become_follower(self.term, R.NONE)
        return R.Result()


def from_node_state(s, g: int, mask: int) -> VRaft:
    n = s.N
    r = VRaft(id=s.self_peer + 1, peers=list(range(1, n + 1)), term=int(s.term[g]), vote=int(s.vote[g]), lead=int(s.lead[g]),
              state=int(s.role[g]), elapsed=int(s.elapsed[g]), committed=int(s.committed[g]), last_index=int(s.last_index[g]),
              last_term=int(s.last_term[g]), first_index_of_term=int(s.first_idx[g]),
              voters=frozenset(p + 1 for p in range(n) if (int(mask) >> p) & 1))
    r.prs = {p + 1: R.Progress(int(s.match[p, g])) for p in range(n)}
    r.votes = {p + 1: (int(s.votes[p, g]) == 1) for p in range(n) if int(s.votes[p, g]) in (1, 2)}
    return r


def to_node_state(r: VRaft, s, g: int) -> None:
    s.term[g], s.vote[g], s.lead[g], s.role[g], s.elapsed[g] = r.term, r.vote, r.lead, r.state, r.elapsed
    s.committed[g], s.last_index[g], s.last_term[g], s.first_idx[g] = r.committed, r.last_index, r.last_term, r.first_index_of_term
    for p in range(s.N):
        s.match[p, g] = r.prs[p + 1].match
        s.votes[p, g] = 1 if r.votes.get(p + 1) is True else 2 if r.votes.get(p + 1) is False else 0


def _common(o, r, m):
    o["group"], o["term"], o["commit"], o["last_index"] = m["group"], r.term, r.committed, r.last_index
    o["to"], o["vote"], o["lead"], o["role"] = m["from"], r.vote, r.lead, r.state


def step_batch(s, voters, msgs) -> np.ndarray:
    """Step for every message, in order, over each group's own voters -> raftq_step_out_t[]; `s` moves."""
    out = np.zeros(len(msgs), dtype=pyoracle.STEP_OUT_DT)
    rafts = {}
    for i in range(len(msgs)):
        m = msgs[i]
        fl = int(m["_pad"][1])
        if fl & MSGF_SKIP:
            out[i]["type"] = OutSkipped
            continue
        g = int(m["group"])
        r = rafts.get(g)
        if r is None:
            r = rafts[g] = from_node_state(s, g, voters[g])
            r.held = False
        if fl & MSGF_HOLD:
            r.held = True
            _common(out[i], r, m)
            out[i]["type"] = OutHeld
            continue
        t = int(m["type"])
        local = t in (R.MsgHup, R.MsgBeat)
        res = r.step(R.Message(type=t, frm=0 if local else int(m["from"]) + 1, term=int(m["term"]), log_term=int(m["log_term"]),
                               index=int(m["index"]), commit=int(m["commit"]), reject=bool(m["reject"]),
                               entries=(int(m["reject_hint"]),) * (int(m["_resv"]) & 0xFFFFFFFF) if fl & MSGF_ENTRIES else None,
                               barrier=bool(fl & MSGF_BARRIER)))
        _common(out[i], r, m)
        out[i]["type"], out[i]["index"], out[i]["log_term"], out[i]["reject"], out[i]["flags"] = res.type, res.index, res.log_term, res.reject, res.flags
    for g, r in rafts.items():
        to_node_state(r, s, g)
    return out


def apply_log_deltas(s, voters, group, last_index, last_term, commit_to=0) -> np.ndarray:
    """the log owner's tail reports, in order -> committed after each record; `s` moves"""
    group = np.atleast_1d(np.asarray(group, dtype=np.uint64))
    li, lt, ct = (np.broadcast_to(np.asarray(x, dtype=np.uint64), group.shape) for x in (last_index, last_term, commit_to))
    out = np.zeros(len(group), dtype=np.uint64)
    for i, g in enumerate(group.tolist()):
        r = from_node_state(s, g, voters[g])
        r.last_index, r.last_term = int(li[i]), int(lt[i])
        if r.state == R.StateLeader:
            r.prs[r.id].maybe_update(r.last_index)
            r.maybe_commit()
        elif int(ct[i]) != 0:
            r.commit_to(int(ct[i]))
        to_node_state(r, s, g)
        out[i] = r.committed
    return out


def full_masks(n: int, g: int) -> np.ndarray:
    return np.full(g, (1 << n) - 1, np.uint16)


def random_masks(rng, n: int, g: int) -> np.ndarray:
    """uniform in [1, 2^N); in [0, 2) for N = 1"""
    return (rng.integers(0, 2, g) if n == 1 else rng.integers(1, 1 << n, g)).astype(np.uint16)


# ---- the directed inputs: one message per group, an outcome that depends on who votes ------------------------------------
L = 20  # the led groups' lastIndex


def commit_input(n: int, self_peer: int, g: int, seed: int):
    """Every group is led (term 3, the log ends at (L, 3), first_idx 1, committed 0..3).  A voter's Match is 0..10; a non-voter's
    is L in the even groups and 0 in the odd ones; self holds L.  One MsgAppResp per group at term 3 from a uniform slot, index
    10..L, not rejecting.  -> (NodeState, voters, msgs)"""
    rng = np.random.default_rng(seed)
    voters = random_masks(rng, n, g)
    bits = ((voters[None, :].astype(np.uint32) >> np.arange(n, dtype=np.uint32)[:, None]) & 1).astype(bool)
    s = pyoracle.NodeState(g, n, self_peer)
    s.role[:], s.term[:], s.last_index[:], s.last_term[:], s.first_idx[:] = 2, 3, L, 3, 1
    s.vote[:] = s.lead[:] = self_peer + 1
    s.committed[:] = rng.integers(0, 4, g)
    even = np.arange(g) % 2 == 0
    s.match[:] = np.where(bits, rng.integers(0, 11, (n, g)), np.where(even, L, 0)[None, :]).astype(np.uint64)
    s.match[self_peer] = L
    m = np.zeros(g, dtype=pyoracle.STEP_MSG_DT)
    m["group"], m["type"], m["term"] = np.arange(g), R.MsgAppResp, 3
    m["from"], m["index"] = rng.integers(0, n, g), rng.integers(10, L + 1, g)
    return s, voters, m


def election_input(n: int, self_peer: int, g: int, seed: int):
    """Every group is a candidate (term 3, vote = self, the log ends at (5, 2)).  Self has granted; every other voter is drawn
    from {none, none, granted, rejected}; a non-voter has granted in the even groups and rejected in the odd ones.  One
    MsgVoteResp per group at term 3: with probability 0.8 from a slot with nothing recorded (if there is one), otherwise from a
    uniform slot; it rejects with probability 0.4.  -> (NodeState, voters, msgs)"""
    rng = np.random.default_rng(seed)
    voters = random_masks(rng, n, g)
    bits = ((voters[None, :].astype(np.uint32) >> np.arange(n, dtype=np.uint32)[:, None]) & 1).astype(bool)
    s = pyoracle.NodeState(g, n, self_peer)
    s.role[:], s.term[:], s.last_index[:], s.last_term[:] = 1, 3, 5, 2
    s.vote[:] = self_peer + 1
    s.match[self_peer] = 5
    even = np.arange(g) % 2 == 0
    drawn = rng.choice(np.array([0, 0, 1, 2], np.uint8), (n, g))
    s.votes[:] = np.where(bits, drawn, np.where(even, 1, 2)[None, :]).astype(np.uint8)
    s.votes[self_peer] = 1
    frm = rng.integers(0, n, g)
    fresh = rng.random(g) < 0.8
    pick = rng.random((n, g))
    pick[s.votes != 0] = -1.0  # a uniform choice among the slots with nothing recorded
    has_free = (s.votes == 0).any(axis=0)
    frm = np.where(fresh & has_free, pick.argmax(axis=0), frm)
    m = np.zeros(g, dtype=pyoracle.STEP_MSG_DT)
    m["group"], m["type"], m["term"], m["from"] = np.arange(g), R.MsgVoteResp, 3, frm
    m["reject"] = rng.random(g) < 0.4
    return s, voters, m


def copy_state(s):
    c = pyoracle.NodeState(s.G, s.N, s.self_peer)
    for k, _ in s.FIELDS:
        getattr(c, k)[:] = getattr(s, k)
    c.match[:], c.votes[:] = s.match, s.votes
    return c


# floors of include-independent discrimination (the share of groups in which the masked statement and the same statement with
# every mask full end differently), asserted at G = 3,149: (input, N class) -> floor
FLOORS = {("commit", "n>=3"): 0.4, ("commit", "n=2"): 0.1, ("commit", "n=1"): 0.3, ("election", "n>=2"): 0.2, ("election", "n=1"): 0.2}


def floor_for(kind: str, n: int) -> float:
    if kind == "commit":
        return FLOORS[("commit", "n>=3" if n >= 3 else "n=%d" % n)]
    return FLOORS[("election", "n>=2" if n >= 2 else "n=1")]


def discrimination(kind: str, n: int, self_peer: int, g: int, seed: int) -> float:
    """share of the groups whose outcome (commit index after / role after) differs between the masks and full masks"""
    s, voters, m = (commit_input if kind == "commit" else election_input)(n, self_peer, g, seed)
    a, b = copy_state(s), copy_state(s)
    step_batch(a, voters, m)
    step_batch(b, full_masks(n, g), m)
    return float(((a.committed != b.committed) if kind == "commit" else (a.role != b.role)).mean())
