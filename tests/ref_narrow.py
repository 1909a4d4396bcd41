"""The narrow mirror of the match rows, stated in numpy: one u64 anchor per group and one u32 offset per (row, group),
match[p][g] == anchor[g] + offset[p][g] while the mirror is valid.  Build, validity, the ingest rule and the commit
sweep over anchor and offsets, as raftq_kernels.hpp runs them (narrow_build_kernel, narrow_follow, the narrow body of
tile_finish).  TEST INFRASTRUCTURE."""
import numpy as np

from tests import ref_numpy as R

SPAN = 1 << 32  # offsets are 32 bits: a group whose values spread over SPAN or more has no mirror


class Mirror:
    def __init__(self, anchor, off, valid):
        self.anchor, self.off, self.valid = anchor, off, valid

    def rows(self):
        """the rows the mirror stands for (only meaningful while valid)"""
        return self.anchor[None, :] + self.off.astype(np.uint64)


def build(match) -> Mirror:
    """anchor = the group's smallest value; valid iff every group's largest is less than 2^32 above it"""
    match = np.asarray(match, dtype=np.uint64)
    anchor = match.min(axis=0)
    spread = match.max(axis=0) - anchor
    valid = bool((spread < np.uint64(SPAN)).all())
    off = (match - anchor[None, :]).astype(np.uint32)  # truncated where the group is too wide: nobody reads it then
    return Mirror(anchor, off, valid)


def ingest(match, mir: Mirror, group, peer, value):
    """One batch of acks (Progress.maybeUpdate: Match only rises), applied to the rows and followed by the mirror.
    A value below the anchor changes neither; one at or above anchor + 2^32 ends the mirror; every other one is the
    same maximum at 32 bits.  In place."""
    was_valid = mir.valid
    for g, p, v in zip(group, peer, value):
        g, p, v = int(g), int(p), int(v)
        if was_valid:
            base = int(mir.anchor[g])
            if v >= base + SPAN:
                mir.valid = False
            elif v >= base:
                mir.off[p, g] = max(int(mir.off[p, g]), v - base)
        match[p, g] = max(int(match[p, g]), v)
    return match, mir


def mci(mir: Mirror):
    """The q-th largest over the OFFSETS plus the anchor: the offsets of a group share its anchor, so their order and
    their ties are those of the values."""
    n = mir.off.shape[0]
    sel = np.sort(mir.off, axis=0)[n - R.quorum(n)]
    return mir.anchor + sel.astype(np.uint64)


def commit_advance(mir: Mirror, committed, gated=False, first_idx=None):
    m = mci(mir)
    committed = np.asarray(committed, dtype=np.uint64)
    adv = m > committed
    if gated:
        f = np.asarray(first_idx, dtype=np.uint64)
        adv &= (f != 0) & (m >= f)
    return np.where(adv, m, committed).astype(np.uint64), int(adv.sum())


def narrow_bytes(n):
    """match bytes a group costs each body of the sweep: (narrow, self-row skip, every row)"""
    return 8 + 4 * n, 8 * (n - 1), 8 * n


def body(n, self_max_valid, narrow_valid):
    """which body the sweep takes (tile_body): the one that moves the fewest bytes among those the words allow"""
    nb, sb, ab = narrow_bytes(n)
    best, cost = "all", ab
    if self_max_valid and n >= 2 and sb < cost:
        best, cost = "skip", sb
    if narrow_valid and n >= 3 and nb < cost:
        best, cost = "narrow", nb
    return best
