"""Reference for per-group voter sets (include/raftq.h "per-group voter sets"): the masked commit candidate and tally in
numpy, three ways that must agree (tests/test_voters_ref.py), and the state a run of voter deltas leaves.  voters[g] is a
16-bit mask, bit p = peer slot p votes in group g; n_g = popcount, q_g = n_g // 2 + 1.  An empty mask: candidate 0, pending.

Whole arrays in, whole arrays out: match / votes are [N, G] as the C-ABI's, voters / committed / first_idx are [G]."""
import numpy as np

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def popcount16(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.uint16).astype(np.uint32)
    return sum(((v >> p) & 1) for p in range(16)).astype(np.uint32)


def quorum(voters) -> np.ndarray:
    return popcount16(voters) // 2 + 1


def member_bits(voters, n_peers: int) -> np.ndarray:
    """-> bool [N, G]: slot p votes in group g"""
    v = np.asarray(voters, dtype=np.uint16).astype(np.uint32)
    return ((v[None, :] >> np.arange(n_peers, dtype=np.uint32)[:, None]) & 1).astype(bool)


def candidate_kernel_form(match, voters) -> np.ndarray:
    """The kernel's formulation: zero the non-voters, sort descending, take index q_g - 1."""
    match = np.asarray(match, dtype=np.uint64)
    n = match.shape[0]
    z = np.where(member_bits(voters, n), match, np.uint64(0))
    desc = np.sort(z, axis=0)[::-1]
    idx = (quorum(voters) - 1).astype(np.int64)
    return np.take_along_axis(desc, idx[None, :], axis=0)[0]


def candidate_counting_form(match, voters) -> np.ndarray:
    """The definition: the largest i such that at least q_g voters have match >= i (0 when no voter's value qualifies, as for
    an empty mask).  Such an i is 0 or one of the voters' values."""
    match = np.asarray(match, dtype=np.uint64)
    n = match.shape[0]
    bits = member_bits(voters, n)
    q = quorum(voters)
    best = np.zeros(match.shape[1], dtype=np.uint64)
    for c in range(n):  # candidate value: voter c's own match
        at_least = ((match >= match[c][None, :]) & bits).sum(axis=0)
        ok = bits[c] & (at_least >= q)
        best = np.where(ok & (match[c] > best), match[c], best)
    return best


def candidate_oracle_form(oracle, match, voters, count: bool = False) -> np.ndarray:
    """The existing oracle's per-group maybeCommit candidate (mci_sort, or mci_count) on the voters' gathered column."""
    match = np.asarray(match, dtype=np.uint64)
    bits = member_bits(voters, match.shape[0])
    f = oracle.mci_count if count else oracle.mci_sort
    out = np.zeros(match.shape[1], dtype=np.uint64)
    for g in range(match.shape[1]):
        col = match[bits[:, g], g]
        if col.size:
            out[g] = f(col)
    return out


def commit_advance(match, committed, voters, gated: bool = False, first_idx=None):
    """-> (committed' [G] u64, n_changed): raftLog.maybeCommit over the masked candidate; never decreases."""
    committed = np.asarray(committed, dtype=np.uint64)
    mci = candidate_kernel_form(match, voters)
    adv = mci > committed
    if gated:
        f = np.asarray(first_idx, dtype=np.uint64)
        adv &= (f != 0) & (mci >= f)
    out = np.where(adv, mci, committed)
    return out, int(adv.sum())


def vote_tally(votes, voters):
    """-> (outcome [G] u8, n_won, n_lost): granted / rejected counted over the voters only."""
    votes = np.asarray(votes, dtype=np.uint8)
    bits = member_bits(voters, votes.shape[0])
    q = quorum(voters)
    granted = ((votes == 1) & bits).sum(axis=0)
    rejected = ((votes == 2) & bits).sum(axis=0)
    won = granted >= q
    lost = ~won & (rejected >= q)
    out = np.where(won, 1, np.where(lost, 2, 0)).astype(np.uint8)
    return out, int(won.sum()), int(lost.sum())


def tally_oracle_form(oracle, votes, voters) -> np.ndarray:
    """The oracle's poll on the voters' column; an empty mask is pending by definition."""
    votes = np.asarray(votes, dtype=np.uint8)
    bits = member_bits(voters, votes.shape[0])
    out = np.zeros(votes.shape[1], dtype=np.uint8)
    for g in range(votes.shape[1]):
        col = votes[bits[:, g], g]
        if col.size:
            out[g] = oracle.poll(col)
    return out


def apply_voter_deltas(match, votes, voters, group, new_voters, reset):
    """-> (match', votes', voters') after one batch: the last record of a group wins (its mask AND its reset; the earlier
    records of that group do nothing)."""
    match, votes = np.array(match, dtype=np.uint64), np.array(votes, dtype=np.uint8)
    voters = np.array(voters, dtype=np.uint16)
    last = {}
    for i, g in enumerate(np.asarray(group, dtype=np.uint64).tolist()):
        last[g] = i
    for g, i in last.items():
        voters[g] = new_voters[i]
        for p in range(match.shape[0]):
            if (int(reset[i]) >> p) & 1:
                match[p, g] = 0
                votes[p, g] = 0
    return match, votes, voters


def sort_through_network(net, values):
    """values [N, K] through the comparator list `net` (descending compare-exchanges) -> sorted [N, K]"""
    v = [np.array(r, dtype=np.uint64) for r in values]
    for a, b in net:
        hi, lo = np.maximum(v[a], v[b]), np.minimum(v[a], v[b])
        v[a], v[b] = hi, lo
    return np.stack(v)
