"""The narrowing rule of the decoder's packed output forms (include/raftq_wire.h, "A frame is NARROW when ..."), stated once more
in Python FROM THE HEADER TEXT -- not from raftsql_amd.wire.expand_packed, which it is used to check -- and the corpora the
packed tests (CPU: tests/test_decode_packed_abi.py, GPU: tests/test_decode_packed_gpu.py) share.  TEST INFRASTRUCTURE.

pack(records, to_slot, form, head_types) turns the 64-byte records of a plain decode (the oracle's, or a twin engine's) into
what the packed call has to deliver: the narrow array and wide[]."""
import functools

import numpy as np

from oracle import pywire as W
from tests import _wiregen

F_WIDE = 0x08
FORM_40, FORM_HEAD = 40, 8
MSG_APP_RESP = 4
RESPONSE_KINDS = (1 << 4) | (1 << 6) | (1 << 9)  # MsgAppResp, MsgVoteResp, MsgHeartbeatResp
# raftq_wire_head_t / raftq_wire_msg40_t, written out from the header
HEAD_DT = np.dtype([("group", "<u4"), ("from", "u1"), ("type", "u1"), ("reject", "u1"), ("flags", "u1")])
MSG40_DT = np.dtype([("group", "<u4"), ("from", "u1"), ("type", "u1"), ("reject", "u1"), ("flags", "u1"), ("term", "<u8"),
                     ("index", "<u8"), ("aux", "<u8"), ("commit", "<u8")])
NARROW_DT = {FORM_40: MSG40_DT, FORM_HEAD: HEAD_DT}


def is_narrow(r: np.ndarray, to_slot: int, form: int, head_types: int = 0) -> np.ndarray:
    """-> bool[n]: the frame is exactly expressible in the narrow record of `form`"""
    malformed = (r["flags"] & W.F_MALFORMED) != 0
    resp = r["type"] == MSG_APP_RESP
    not_carried = np.where(resp, r["log_term"], r["reject_hint"])
    ok = (r["group"] < (1 << 32)) & ((r["from"] <= 254) | (r["from"] == 0xFFFFFFFF)) & (r["to"] == to_slot) & (r["n_ents"] == 0) & (not_carried == 0)
    if form == FORM_HEAD:
        t = r["type"].astype(np.uint64)
        in_mask = (t < 32) & (((np.uint64(head_types) >> np.minimum(t, np.uint64(31))) & np.uint64(1)) != 0)
        ok = ok & in_mask & (r["reject"] == 0)
    return malformed | ok


def pack(r: np.ndarray, to_slot: int, form: int, head_types: int = 0):
    """-> (narrow[n], wide[n_wide]) as the header says the packed call delivers them"""
    narrow = is_narrow(r, to_slot, form, head_types)
    out = np.zeros(len(r), NARROW_DT[form])
    out["group"] = r["group"] & np.uint64(0xFFFFFFFF)  # "the full record's, truncated to their width"
    out["from"] = r["from"] & 0xFF  # (absent, 0xFFFFFFFF, is written as 0xFF)
    out["type"], out["reject"] = r["type"], r["reject"]
    out["flags"] = r["flags"] | np.where(narrow, 0, F_WIDE).astype(np.uint8)
    if form == FORM_40:
        out["term"], out["index"], out["commit"] = r["term"], r["index"], r["commit"]
        k = np.cumsum(~narrow) - 1  # wide[] is in ascending frame order
        out["aux"] = np.where(narrow, np.where(r["type"] == MSG_APP_RESP, r["reject_hint"], r["log_term"]), k.astype(np.uint64))
    return out, r[~narrow].copy()


def delivered(r: np.ndarray, to_slot: int, form: int, head_types: int = 0) -> np.ndarray:
    """the records an exact expansion has to give back: all of them in FORM_40; in FORM_HEAD a narrow frame's term, index,
    log_term, commit and reject_hint are the caller's declared loss (0)"""
    out = r.copy()
    if form == FORM_HEAD:
        narrow = is_narrow(r, to_slot, form, head_types)
        for f in ("term", "index", "log_term", "commit", "reject_hint"):
            out[f][narrow] = 0
    return out


# ---- corpora: -> (stream uint8[], frame_off uint64[n + 1]) -----------------------------------------------------------------
def _be(body: bytes) -> bytes:
    return len(body).to_bytes(8, "big") + body


def random_corpus(seed: int, n: int):
    """_wiregen.random_msgs: every varint length, any addressee, 64-bit groups -- almost only wide frames"""
    m, e, pool = _wiregen.random_msgs(np.random.default_rng(seed), n, ent_frac=0.3)
    return W.wire_encode(m, e, pool)


def noncanonical_corpus(seed: int, n: int = 300):
    rng = np.random.default_rng(seed)
    m, e, pool = _wiregen.random_msgs(rng, n, ent_frac=0.4)
    half = np.arange(n) % 2 == 0  # half of them shaped so that narrow frames occur among the odd encodings too
    m["to"] = np.where(half, 0, m["to"])
    m["group"] = np.where(half, m["group"] % np.uint64(1000), m["group"])
    m["log_term"] = np.where(half & (m["type"] == 4), 0, m["log_term"])
    m["reject_hint"] = np.where(half & (m["type"] != 4), 0, m["reject_hint"])
    bodies = [_wiregen.noncanonical_message(rng, m[i], e, pool) for i in range(n)]
    stream = np.frombuffer(b"".join(_be(b) for b in bodies), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(b) + 8 for b in bodies])]).astype(np.uint64)
    return stream, off


def malformed_corpus():
    """the hand cases of tests/test_wire_gpu.py::test_decode_malformed_frames, a good frame between any two"""
    good = _be(bytes.fromhex("0806100218012005"))
    cases = [
        (9).to_bytes(8, "big") + bytes.fromhex("0806100218012005"),  # length word disagrees
        _be(bytes.fromhex("080610021801208080")),  # truncated varint
        _be(bytes.fromhex("20" + "80" * 10 + "01")),  # 11-byte varint
        _be(bytes.fromhex("08033a0508001005")),  # entry length overruns
        _be(bytes.fromhex("2201aa")),  # wrong wire type on term
        _be(bytes.fromhex("0001")),  # tag 0
        _be(bytes.fromhex("6b")),  # group wire type
        _be(bytes.fromhex("3a021280")),  # bad entry inside
        _be(bytes.fromhex("4a021201")),  # bad snapshot inside
        b"\x00\x00\x00",  # shorter than a length word
        _be(bytes.fromhex("08" + "ff" * 9 + "01" + "20" + "ff" * 9 + "7f")),  # 10-byte varints: fine
        _be(bytes.fromhex("4a00")),  # empty snapshot, nothing else
        _be(bytes.fromhex("4a061204" "0a020801" "3a00" "3a021001")),  # snapshot with a conf_state member; two entries
    ]
    stream, off = good, [0, len(good)]
    for b in cases:
        stream += b + good
        off += [off[-1] + len(b), off[-1] + len(b) + len(good)]
    return np.frombuffer(stream, np.uint8), np.array(off, np.uint64)


MALFORMED_TO_SLOT = 1  # the good frame's `to` is raft ID 2


def fuzz_corpus(seed: int, n: int = 600):
    """valid frames with 1 byte in 40 overwritten (most length words repaired), then noise cut at random boundaries with
    valid length words, then boundaries that are themselves nonsense (decreasing, past the end)"""
    rng = np.random.default_rng(seed)
    m, e, pool = _wiregen.random_msgs(rng, n, ent_frac=0.5, max_payload=60)
    m["to"] = np.where(rng.random(n) < 0.6, 0, m["to"])
    s, off = W.wire_encode(m, e, pool)
    s = s.copy()
    pos = rng.integers(0, len(s), len(s) // 40)
    s[pos] = rng.integers(0, 256, len(pos), dtype=np.uint8)
    for i in rng.choice(n, n * 9 // 10, replace=False):
        a, b = int(off[i]), int(off[i + 1])
        s[a:a + 8] = np.frombuffer((b - a - 8).to_bytes(8, "big"), np.uint8)
    noise = rng.integers(0, 256, 6000, dtype=np.uint8)
    cuts = np.sort(rng.choice(np.arange(1, len(noise)), 200, replace=False))
    noff = np.concatenate([[0], cuts, [len(noise)]]).astype(np.uint64)
    for i in range(len(noff) - 1):
        a, b = int(noff[i]), int(noff[i + 1])
        if b - a >= 8:
            noise[a:a + 8] = np.frombuffer((b - a - 8).to_bytes(8, "big"), np.uint8)
    stream = np.concatenate([s, noise])
    total = len(stream)
    garbage = np.array([5, total + 100, total, 3, total - 1], np.uint64)
    return stream, np.concatenate([off, noff[1:] + np.uint64(len(s)), garbage])


def node_corpus(seed: int, n: int, to_slot: int = 0, n_peers: int = 3, n_groups: int = 64, app_frac: float = 0.15, wide_last: bool = True,
                reject_frac: float = 0.1):
    """what a node receives in a turn, all of it addressed to its own slot: acknowledgements (one in ten a rejection with its
    hint), heartbeats and their answers, votes and theirs, and app_frac MsgApp with 1-3 entries.  wide_last: the last frame
    is a MsgApp with entries (the one frame of an odd last tile is then wide: its place in wide[] comes from the look-back)"""
    rng = np.random.default_rng(seed)
    rest = 1.0 - app_frac
    t = rng.choice([3, 4, 9, 8, 6, 5], n, p=[app_frac, rest * 0.55, rest * 0.15, rest * 0.12, rest * 0.09, rest * 0.09])
    if wide_last and app_frac > 0:
        t[-1] = 3
    m = np.zeros(n, W.WIRE_MSG_DT)
    m["type"] = t
    m["group"] = rng.integers(0, n_groups, n)
    m["from"] = (to_slot + 1 + rng.integers(0, n_peers - 1, n)) % n_peers
    m["to"] = to_slot
    m["term"] = rng.integers(1, 9, n)
    m["index"] = rng.integers(0, 100000, n)
    m["commit"] = np.where(np.isin(t, [3, 8]), rng.integers(0, 100000, n), 0)
    m["log_term"] = np.where(np.isin(t, [3, 5]), rng.integers(1, 9, n), 0)
    rej = np.isin(t, [4, 6]) & (rng.random(n) < reject_frac)
    m["reject"] = rej
    m["reject_hint"] = np.where(rej & (t == 4), rng.integers(1, 100000, n), 0)
    k = np.where(t == 3, rng.integers(1, 4, n), 0)
    m["n_ents"] = k
    m["ent_first"] = np.where(k > 0, np.concatenate([[0], np.cumsum(k)[:-1]]), 0)
    ne = int(k.sum())
    e = np.zeros(ne, W.WIRE_ENT_DT)
    owner = np.repeat(np.arange(n), k)
    e["term"] = m["term"][owner]
    e["index"] = m["index"][owner] + 1 + (np.arange(ne) - m["ent_first"][owner])
    e["data_len"] = rng.integers(0, 48, ne)
    e["data_off"] = np.concatenate([[0], np.cumsum(e["data_len"])[:-1]]) if ne else 0
    pool = rng.integers(0, 256, int(e["data_len"].sum()) + 1, dtype=np.uint8)
    return W.wire_encode(m, e, pool)


@functools.lru_cache(maxsize=None)
def oracle_decode(kind: str, seed: int = 0, n: int = 0):
    """(stream, frame_off, records, entry headers, n_malformed) of a corpus, decoded ONCE by the oracle and shared (read-only)"""
    if kind == "node":
        s, off = node_corpus(seed, n)
    elif kind == "acks":  # the one-node leg's inbound traffic: nothing carries entries, nothing is rejected
        s, off = node_corpus(seed, n, app_frac=0.0, reject_frac=0.0)
    elif kind == "random":
        s, off = random_corpus(seed, n)
    elif kind == "noncanonical":
        s, off = noncanonical_corpus(seed)
    elif kind == "malformed":
        s, off = malformed_corpus()
    elif kind == "fuzz":
        s, off = fuzz_corpus(seed)
    else:
        raise KeyError(kind)
    s, off = np.ascontiguousarray(s), np.ascontiguousarray(off, np.uint64)
    m, e, bad = W.wire_decode(s, off)
    for a in (s, off, m, e):
        a.setflags(write=False)
    return s, off, m, e, bad
