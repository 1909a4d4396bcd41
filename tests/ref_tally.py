"""The tally mirror of the vote words, stated in numpy: one byte per group, granted | rejected << 4, the two counts
raft.poll takes over the group's N two-bit fields (01 granted, 10 rejected; 00 and 11 count as neither).  Build, the ingest
rule and the outcome from a byte, as raftq_kernels.hpp runs them (tally_build_kernel, vote_apply_kernel's add, poll_tally).
TEST INFRASTRUCTURE."""
import numpy as np

from tests import ref_numpy as R


def pack_words(votes):
    """the device's vote words of a [N][G] array of fields (values 0..3: 11 is carried as it is)"""
    votes = np.asarray(votes, dtype=np.uint32)
    w = np.zeros(votes.shape[1], np.uint32)
    for p in range(votes.shape[0]):
        w |= (votes[p] & 3) << (2 * p)
    return w


def fields(words, n):
    """[N][G] fields of the words"""
    words = np.asarray(words, dtype=np.uint32)
    return np.stack([(words >> (2 * p)) & 3 for p in range(n)]).astype(np.uint8)


def build(words, n):
    """tally[g] of every word: counted over the N fields"""
    f = fields(words, n)
    return ((f == 1).sum(axis=0) | ((f == 2).sum(axis=0) << 4)).astype(np.uint8)


def outcome_from_tally(byte, n):
    """poll's outcome from the byte alone: 1 won, 2 lost, 0 pending"""
    byte = np.asarray(byte, dtype=np.uint8)
    q = R.quorum(n)
    g, r = byte & 15, byte >> 4
    return np.where(g >= q, 1, np.where(r >= q, 2, 0)).astype(np.uint8)


def ingest(votes, tally, group, peer, vote):
    """One batch of vote records on fields [N][G] and bytes (G rounded up to a multiple of 4: the device's rows are padded),
    in place.  The first record of a (group, peer) in batch position holds the slot; it is applied if the field is unanswered
    (not 01 / 10), and then -- only then -- the byte gains one in the nibble of its answer, as a 32-bit add into the word of
    four bytes that holds it.  -> the number of adds"""
    assert tally.dtype == np.uint8 and tally.size % 4 == 0
    words = tally.view("<u4")
    seen, adds = set(), 0
    for g, p, v in zip(group, peer, vote):
        g, p, v = int(g), int(p), int(v)
        if (g, p) in seen:
            continue
        seen.add((g, p))
        if votes[p, g] in (1, 2):
            continue
        votes[p, g] = v
        words[g >> 2] = (int(words[g >> 2]) + ((1 if v == 1 else 16) << (8 * (g & 3)))) & 0xFFFFFFFF
        adds += 1
    return adds


def padded(tally):
    """the bytes with the device's padding (zeros) up to a multiple of 4"""
    return np.concatenate([tally, np.zeros(-tally.size % 4, np.uint8)])


# ---- the inputs of tests/test_tally_gpu.py (tests/test_tally_ref.py shows what they cover) ------------------------------------
G = 4099  # two full 2,048-group tiles and a ragged third


def gpu_state(n, seed):
    """synth's population with the first 3 * 4 groups' votes set by hand, so that whatever the draw every outcome is there:
    group 4k pending and one vote short of won, 4k + 1 one short of lost, 4k + 2 won, 4k + 3 lost (k = 0, 1, 2)"""
    from raftsql_amd import synth

    st = synth.make_groups(G, n, seed=seed, with_terms=True)
    q = R.quorum(n)
    for k in range(3):
        st.votes[:, 4 * k:4 * k + 4] = 0
        st.votes[:q - 1, 4 * k] = 1      # granted: q - 1 (pending; for n = 1 nothing)
        st.votes[:q - 1, 4 * k + 1] = 2  # rejected: q - 1
        st.votes[:q, 4 * k + 2] = 1      # won
        st.votes[:q, 4 * k + 3] = 2      # lost
    return st


def gpu_vote_batch(n, seed):
    """-> (group, peer, vote): a batch for a handle that holds gpu_state(n, ..).votes.  Random records all over (answered and unanswered
    slots alike), and by hand: the deciding vote of groups 0 and 1 sent THREE times (counted twice, group 0's byte would say
    q + 1 granted while its word says q -- and at n = 1..2 a pending group would read won), both answers for one slot of
    groups 4 and 5 (the first in batch position wins: group 4 gets the grant that decides it, group 5 a rejection in front of
    a grant), a record for an answered slot of group 2, and the last group of the ragged tile."""
    rng = np.random.default_rng(seed)
    q = R.quorum(n)
    m = 3000
    g = rng.integers(12, G, m).astype(np.uint64)
    p = rng.integers(0, n, m).astype(np.uint32)
    v = rng.integers(1, 3, m).astype(np.uint8)
    hand = [(0, q - 1, 1)] * 3 + [(1, q - 1, 2)] * 3 + [(4, q - 1, 1), (4, q - 1, 2), (5, q - 1, 2), (5, q - 1, 1), (2, 0, 2),
                                                          (G - 1, n - 1, 1), (G - 1, n - 1, 2)]
    where = rng.choice(m, len(hand), replace=False)  # spread through the batch, their own order kept
    for i, (hg, hp, hv) in zip(np.sort(where), hand):
        g[i], p[i], v[i] = hg, hp, hv
    return g, p, v
