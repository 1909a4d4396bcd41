"""Host-side mirror of the batched wire / WAL codecs (include/raftq_wire.h).

`WireEngine` is a NodeEngine that also marshals / unmarshals whole batches of
raftpb.Message stream frames (what the reference sends with
`rc.transport.Send(rd.Messages)`, raft.go:230) and walpb.Record WAL frames
(`rc.wal.Save`, raft.go:228; `w.ReadAll`, raft.go:124) on the GPU, and can feed
Step straight from received frames.  Records are numpy structured arrays
layout-identical to the C structs.  No CPU path: every codec call goes to the
library, which needs the handle's GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .engine import _ptr
from .step import NodeEngine

MSG_SNAP = 7
F_MALFORMED, F_SNAPSHOT, F_GROUP = 1, 2, 4
WAL_METADATA, WAL_ENTRY, WAL_STATE, WAL_CRC, WAL_SNAPSHOT = 1, 2, 3, 4, 5
WAL_F_MALFORMED, WAL_F_BADCRC, WAL_F_GROUP = 1, 2, 4

WIRE_MSG_DT = np.dtype([("group", "<u8"), ("term", "<u8"), ("log_term", "<u8"), ("index", "<u8"), ("commit", "<u8"),
                        ("reject_hint", "<u8"), ("from", "<u4"), ("type", "u1"), ("reject", "u1"), ("to", "u1"),
                        ("flags", "u1"), ("ent_first", "<u4"), ("n_ents", "<u4")])
WIRE_ENT_DT = np.dtype([("term", "<u8"), ("index", "<u8"), ("data_off", "<u8"), ("data_len", "<u4"), ("type", "<u4")])
PROP_DT = np.dtype([("group", "<u8"), ("ent_first", "<u4"), ("n_ents", "<u4")])  # == raftq_prop_t
PROP_ENT_DT = np.dtype([("data_off", "<u8"), ("data_len", "<u4"), ("type", "<u4")])  # == raftq_prop_ent_t
WAL_REC_DT = np.dtype([("group", "<u8"), ("term", "<u8"), ("index", "<u8"), ("data_off", "<u8"), ("data_len", "<u4"),
                       ("vote", "<u4"), ("crc", "<u4"), ("kind", "u1"), ("entry_type", "u1"), ("flags", "u1"),
                       ("_pad", "u1")])
assert WIRE_MSG_DT.itemsize == 64 and WIRE_ENT_DT.itemsize == 32 and WAL_REC_DT.itemsize == 48
# the decoder's narrow output forms (raftq_wire_decode_packed / raftq_step_frames_packed)
F_WIDE = 0x08  # narrow record only: the frame's full record is in wide[]
FORM_40, FORM_HEAD = 40, 8
WIRE_HEAD_DT = np.dtype([("group", "<u4"), ("from", "u1"), ("type", "u1"), ("reject", "u1"), ("flags", "u1")])  # == raftq_wire_head_t
WIRE_MSG40_DT = np.dtype(WIRE_HEAD_DT.descr + [("term", "<u8"), ("index", "<u8"), ("aux", "<u8"), ("commit", "<u8")])  # == raftq_wire_msg40_t
assert WIRE_MSG40_DT.itemsize == 40 and WIRE_HEAD_DT.itemsize == 8
_FORM_DT = {FORM_40: WIRE_MSG40_DT, FORM_HEAD: WIRE_HEAD_DT}
MSG_APP_RESP = 4
OUTF_ANSWERED = 0x10  # result flag of raftq_step_frames_respond: the messages the result calls for were built on the device
RESPOND_FRAME_MAX = 83  # bytes of the largest payload-free frame: cap >= n * (N - 1) * RESPOND_FRAME_MAX
PROP_APPENDED, PROP_FORWARDED, PROP_DROPPED = 0, 1, 2  # RAFTQ_PROP_*: propose_frames' outcome bytes under set_propose_forward
RESPOND_ENT_MAX = 40  # the most one entry adds to a frame beyond its payload: set_respond_props' bound (RAFTQ_RESPOND_ENT_MAX)
RESPOND_LEAD_FRAME_MAX = 109  # ... and of the largest frame with one empty entry: the bound once set_respond_lead is on


def _u8(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _p(a: np.ndarray):
    return _ptr(a) if a.size else None


def scan_frames(buf, big_endian: bool, cap: int | None = None):
    """The length-word walk (raftq_wire_scan_frames; host only) -> (off uint64[n+1], consumed)."""
    lib = _lib.load()
    b = _u8(buf)
    cap = len(b) // 8 + 1 if cap is None else int(cap)
    off = np.zeros(cap + 1, np.uint64)
    n, used = C.c_uint64(0), C.c_uint64(0)
    rc = lib.raftq_wire_scan_frames(_p(b), len(b), int(big_endian), _ptr(off), cap, C.byref(n), C.byref(used))
    if rc != 0:
        raise _lib.RaftqError(rc, (lib.raftq_last_error(None) or b"?").decode())
    return off[: n.value + 1].copy(), int(used.value)


def expand_packed(narrow: np.ndarray, wide: np.ndarray, to_slot: int, form: int) -> np.ndarray:
    """The 64-byte records raftq_wire_decode would have written, from the narrow array and wide[] (raftq_wire.h "Expansion is
    exact").  FORM_HEAD: a narrow frame's term / index / log_term / commit / reject_hint were not delivered and come out 0."""
    nar = np.asarray(narrow)
    assert nar.dtype == _FORM_DT[form] and np.asarray(wide).dtype == WIRE_MSG_DT
    out = np.zeros(len(nar), WIRE_MSG_DT)
    is_wide = (nar["flags"] & F_WIDE) != 0
    k = np.cumsum(is_wide) - 1  # wide[] is in frame order
    if form == FORM_40:
        assert np.array_equal(nar["aux"][is_wide], k[is_wide].astype(np.uint64)), "aux of a wide frame is its position in wide[]"
    assert int(is_wide.sum()) <= len(wide), "wide[] is shorter than the narrow array says"
    out[is_wide] = wide[k[is_wide]]
    plain = ~is_wide & ((nar["flags"] & F_MALFORMED) == 0)
    for f in ("group", "type", "reject"):
        out[f][plain] = nar[f][plain]
    out["from"][plain] = np.where(nar["from"][plain] == 0xFF, 0xFFFFFFFF, nar["from"][plain].astype(np.uint32))
    out["to"][plain] = to_slot
    if form == FORM_40:
        for f in ("term", "index", "commit"):
            out[f][plain] = nar[f][plain]
        resp = plain & (nar["type"] == MSG_APP_RESP)
        out["reject_hint"][resp] = nar["aux"][resp]
        out["log_term"][plain & ~resp] = nar["aux"][plain & ~resp]
    out["flags"][~is_wide] = nar["flags"][~is_wide]  # (a malformed frame: every other field 0)
    return out


class WireEngine(NodeEngine):
    """NodeEngine + the codecs of the byte formats either side of Step."""

    _respond_lead = False  # set_respond_lead's word, for respond_cap
    _respond_props = False  # set_respond_props', likewise
    _propose_forward = False  # set_propose_forward's: propose_frames then returns the outcomes too

    # -- raftpb.Message <-> rafthttp stream frames -----------------------------------------
    def wire_encode(self, msgs: np.ndarray, ents: np.ndarray | None = None, pool=b"", out: np.ndarray | None = None,
                    off: np.ndarray | None = None):
        """-> (stream uint8[], frame_off uint64[n+1]).  Without `out` two calls are made: the first learns
        the size.  With `out` (uint8, e.g. from engine.pinned_empty) one call writes into it."""
        m = np.ascontiguousarray(msgs, dtype=WIRE_MSG_DT)
        e = np.ascontiguousarray(ents if ents is not None else np.zeros(0, WIRE_ENT_DT), dtype=WIRE_ENT_DT)
        p = _u8(pool)
        if off is None:
            off = np.zeros(len(m) + 1, np.uint64)
        c = _lib.WireCounts()
        args = (self._h, _p(m), len(m), _p(e), len(e), _p(p), len(p))
        if out is not None:
            self._chk(self._lib.raftq_wire_encode(*args, _ptr(out), len(out), _ptr(off), C.byref(c)))
            return out[: int(c.bytes)], off
        rc = self._lib.raftq_wire_encode(*args, None, 0, _ptr(off), C.byref(c))
        if rc == 0:  # nothing to write
            return np.zeros(0, np.uint8), off
        if c.bytes == 0:
            self._chk(rc)
        out = np.zeros(int(c.bytes), np.uint8)
        self._chk(self._lib.raftq_wire_encode(*args, _ptr(out), len(out), _ptr(off), C.byref(c)))
        assert c.bytes == len(out)
        return out, off

    def wire_decode(self, stream, frame_off, want_ents: bool = True, msgs: np.ndarray | None = None,
                    ents: np.ndarray | None = None):
        """-> (msgs, ents, n_malformed).  `msgs` / `ents`: caller-provided result arrays (e.g. pinned)."""
        s = _u8(stream)
        off = np.ascontiguousarray(frame_off, np.uint64)
        n = len(off) - 1
        if msgs is None:
            msgs = np.zeros(n, WIRE_MSG_DT)
        c = _lib.WireCounts()
        if not want_ents:
            self._chk(self._lib.raftq_wire_decode(self._h, _p(s), len(s), _ptr(off), n, _p(msgs), None, 0, C.byref(c)))
            return msgs[:n], np.zeros(0, WIRE_ENT_DT), int(c.n_malformed)
        if ents is not None:
            self._chk(self._lib.raftq_wire_decode(self._h, _p(s), len(s), _ptr(off), n, _p(msgs), _ptr(ents), len(ents),
                                                  C.byref(c)))
            return msgs[:n], ents[: int(c.n_ents)], int(c.n_malformed)
        cap = max(n, 16)
        while True:
            ents = np.zeros(cap, WIRE_ENT_DT)
            rc = self._lib.raftq_wire_decode(self._h, _p(s), len(s), _ptr(off), n, _p(msgs), _ptr(ents), cap, C.byref(c))
            if rc != 0 and c.n_ents > cap:
                cap = int(c.n_ents)
                continue
            self._chk(rc)
            return msgs, ents[: int(c.n_ents)].copy(), int(c.n_malformed)

    def wire_decode_packed(self, stream: np.ndarray, frame_off: np.ndarray, form: int, to_slot: int, narrow: np.ndarray, wide: np.ndarray | None,
                           ents: np.ndarray | None = None, head_types: int = 0, check: bool = True):
        """raftq_wire_decode_packed: every array page-locked (engine.pinned_empty / pinned_copy); narrow: WIRE_MSG40_DT / WIRE_HEAD_DT
        [>= n]; wide: WIRE_MSG_DT [wide_cap] or None.  -> (narrow[:n], wide[:min(n_wide, cap)], ents, counts, n_wide, rc);
        check=False: a refusal is returned as rc instead of raised"""
        n = len(frame_off) - 1
        assert stream.dtype == np.uint8 and frame_off.dtype == np.uint64 and len(narrow) >= n
        assert form not in _FORM_DT or narrow.dtype == _FORM_DT[form]
        assert wide is None or wide.dtype == WIRE_MSG_DT
        c, nw = _lib.WireCounts(), C.c_uint64(0)
        cap = len(wide) if wide is not None else 0
        rc = self._lib.raftq_wire_decode_packed(self._h, stream.ctypes.data if len(stream) else None, len(stream), frame_off.ctypes.data, n, int(form),
                                                int(head_types), int(to_slot), narrow.ctypes.data, wide.ctypes.data if wide is not None else None, cap,
                                                ents.ctypes.data if ents is not None else None, len(ents) if ents is not None else 0, C.byref(c),
                                                C.byref(nw))
        if check:
            self._chk(rc)
        got_ents = ents[: min(int(c.n_ents), len(ents))] if ents is not None else np.zeros(0, WIRE_ENT_DT)
        got_wide = wide[: min(int(nw.value), cap)] if wide is not None else np.zeros(0, WIRE_MSG_DT)
        return narrow[:n], got_wide, got_ents, c, int(nw.value), rc

    # -- Step from the wire -------------------------------------------------------------------
    def step_submit_wire(self, stream, frame_off) -> None:
        s = _u8(stream)
        off = np.ascontiguousarray(frame_off, np.uint64)
        self._chk(self._lib.raftq_step_submit_wire(self._h, _p(s), len(s), _ptr(off), len(off) - 1))

    def step_frames(self, stream: np.ndarray, frame_off: np.ndarray, msgs: np.ndarray, ents: np.ndarray | None = None,
                    tail_appends: bool = True, copy: bool = True):
        """raftq_step_frames: decode + a node's checks + Step over every frame, one submission and one wait.  All arrays
        page-locked (engine.pinned_empty / pinned_copy).  -> (msgs[:n], ents[:min(n_ents, cap)], outs, counts); copy=False: outs
        is a view of the library's pinned result area, valid until the next Step call"""
        from .step import OUT_C_DT, OUT_DT

        n = len(frame_off) - 1
        assert stream.dtype == np.uint8 and frame_off.dtype == np.uint64 and msgs.dtype == WIRE_MSG_DT and len(msgs) >= n
        c = _lib.WireCounts()
        self._chk(self._lib.raftq_step_frames(self._h, stream.ctypes.data if len(stream) else None, len(stream), frame_off.ctypes.data, n,
                                              1 if tail_appends else 0, msgs.ctypes.data, ents.ctypes.data if ents is not None else None,
                                              len(ents) if ents is not None else 0, C.byref(c)))
        p, k = C.c_void_p(None), C.c_uint64(0)
        dt, fn = self._results_form()
        self._chk(fn(self._h, C.byref(p), C.byref(k)))
        outs = np.frombuffer((C.c_char * (k.value * dt.itemsize)).from_address(p.value), dtype=dt, count=k.value) if k.value else np.zeros(0, dt)
        if copy:
            outs = outs.copy()
        got_ents = ents[: min(int(c.n_ents), len(ents))] if ents is not None else np.zeros(0, WIRE_ENT_DT)
        return msgs[:n], got_ents, outs, c

    def step_frames_packed(self, stream: np.ndarray, frame_off: np.ndarray, form: int, narrow: np.ndarray, wide: np.ndarray | None,
                           ents: np.ndarray | None = None, head_types: int = 0, tail_appends: bool = True, copy: bool = True):
        """raftq_step_frames_packed: step_frames with narrow records (to_slot = the handle's own slot).
        -> (narrow[:n], wide[:min(n_wide, cap)], ents, outs, counts, n_wide)"""
        n = len(frame_off) - 1
        assert stream.dtype == np.uint8 and frame_off.dtype == np.uint64 and len(narrow) >= n
        assert form not in _FORM_DT or narrow.dtype == _FORM_DT[form]
        assert wide is None or wide.dtype == WIRE_MSG_DT
        c, nw = _lib.WireCounts(), C.c_uint64(0)
        cap = len(wide) if wide is not None else 0
        self._chk(self._lib.raftq_step_frames_packed(self._h, stream.ctypes.data if len(stream) else None, len(stream), frame_off.ctypes.data, n,
                                                     1 if tail_appends else 0, int(form), int(head_types), narrow.ctypes.data,
                                                     wide.ctypes.data if wide is not None else None, cap, ents.ctypes.data if ents is not None else None,
                                                     len(ents) if ents is not None else 0, C.byref(c), C.byref(nw)))
        p, k = C.c_void_p(None), C.c_uint64(0)
        dt, fn = self._results_form()
        self._chk(fn(self._h, C.byref(p), C.byref(k)))
        outs = np.frombuffer((C.c_char * (k.value * dt.itemsize)).from_address(p.value), dtype=dt, count=k.value) if k.value else np.zeros(0, dt)
        if copy:
            outs = outs.copy()
        got_ents = ents[: min(int(c.n_ents), len(ents))] if ents is not None else np.zeros(0, WIRE_ENT_DT)
        got_wide = wide[: min(int(nw.value), cap)] if wide is not None else np.zeros(0, WIRE_MSG_DT)
        return narrow[:n], got_wide, got_ents, outs, c, int(nw.value)

    def set_bcast_voters(self, on=True) -> None:
        """raftq_bcast_set_voters: with voter masks loaded step_frames_respond's commit broadcast and propose_frames' MsgApps go to
        each group's own members instead of the calls being refused (propose_frames: positional, a non-member's slot has zero length;
        a record whose append would move the commit index is refused); a property of the handle, independent of set_step_voters and
        set_tick_voters (no batch may be in flight)"""
        self._chk(self._lib.raftq_bcast_set_voters(self._h, int(on)))

    def set_respond_lead(self, on=True) -> None:
        """raftq_respond_set_lead: step_frames_respond answers RAFTQ_OUT_BECAME_LEADER too -- becomeLeader's broadcast, one MsgApp
        with the empty entry per peer, flagged answered; respond_cap then asks for the larger frames (no batch may be in flight)"""
        self._chk(self._lib.raftq_respond_set_lead(self._h, int(on)))
        self._respond_lead = int(on) == 1

    def set_respond_props(self, on=True) -> None:
        """raftq_respond_set_props: step_frames_respond answers a RAFTQ_OUT_PROPOSED of a group at the tail too -- the leader's
        MsgApps with the frame's entries, stamped and marshalled on the device, flagged answered; the call then needs ents and
        respond_cap(n, nbytes, ents_cap) bytes of out (no batch may be in flight; an effect only under set_step_props)"""
        self._chk(self._lib.raftq_respond_set_props(self._h, int(on)))
        self._respond_props = int(on) == 1

    def set_propose_forward(self, on=True) -> None:
        """raftq_propose_set_forward: propose_frames turns a record whose group this node follows into ONE MsgProp frame to the
        group's leader (in the run of the leader's slot; the other slots have zero length) and drops one whose group knows no
        leader, instead of refusing the call; it then returns one outcome byte per record too (no batch may be in flight)"""
        self._chk(self._lib.raftq_propose_set_forward(self._h, int(on)))
        self._propose_forward = int(on) == 1

    def propose_outcomes(self) -> np.ndarray:
        """raftq_propose_outcomes: PROP_* of every record of the last propose_frames call that succeeded under set_propose_forward
        (a copy; empty with the switch off or before any such call)"""
        p, k = C.c_void_p(None), C.c_uint64(0)
        self._chk(self._lib.raftq_propose_outcomes(self._h, C.byref(p), C.byref(k)))
        if k.value == 0:
            return np.zeros(0, np.uint8)
        return np.frombuffer((C.c_char * k.value).from_address(p.value), dtype=np.uint8, count=k.value).copy()

    def respond_cap(self, n: int, nbytes: int = 0, ents_cap: int = 0) -> int:
        """the `out` size raftq_step_frames_respond needs for n frames (the exact worst case; follows set_respond_lead) -- and, under
        set_respond_props, for a stream of nbytes bytes and an entry array of ents_cap headers"""
        frame_max = RESPOND_LEAD_FRAME_MAX if self._respond_lead else RESPOND_FRAME_MAX
        cap = int(n) * (self.n_peers - 1) * frame_max
        if self._respond_props:
            cap += (self.n_peers - 1) * (int(nbytes) + int(ents_cap) * RESPOND_ENT_MAX)
        return cap

    def step_frames_respond(self, stream: np.ndarray, frame_off: np.ndarray, msgs: np.ndarray, ents: np.ndarray | None, at_tail: np.ndarray | None,
                            out: np.ndarray, resp_off: np.ndarray | None, peer_off: np.ndarray, tail_appends: bool = True, copy: bool = True):
        """raftq_step_frames_respond: step_frames + the responses and commit broadcasts its results call for, built and marshalled on
        the device, one submission and one wait.  All arrays page-locked (engine.pinned_empty / pinned_copy); at_tail: uint64
        [ceil(G / 64)] or None; out: uint8 of at least respond_cap(n) bytes; resp_off: uint64 [n * (N - 1) + 1] or None; peer_off:
        uint64 [N + 1].  -> (msgs[:n], ents, outs, response bytes (a view of out), resp_off[:n_resp + 1] | None, peer_off, counts,
        resp_counts)"""
        n = len(frame_off) - 1
        assert stream.dtype == np.uint8 and frame_off.dtype == np.uint64 and msgs.dtype == WIRE_MSG_DT and len(msgs) >= n
        assert out.dtype == np.uint8 and peer_off.dtype == np.uint64 and len(peer_off) >= self.n_peers + 1
        assert resp_off is None or (resp_off.dtype == np.uint64 and len(resp_off) >= n * (self.n_peers - 1) + 1)
        assert at_tail is None or (at_tail.dtype == np.uint64 and len(at_tail) >= (self.n_groups + 63) // 64)
        c, rc_ = _lib.WireCounts(), _lib.WireCounts()
        self._chk(self._lib.raftq_step_frames_respond(
            self._h, stream.ctypes.data if len(stream) else None, len(stream), frame_off.ctypes.data, n, 1 if tail_appends else 0,
            msgs.ctypes.data, ents.ctypes.data if ents is not None else None, len(ents) if ents is not None else 0,
            at_tail.ctypes.data if at_tail is not None else None, out.ctypes.data, len(out),
            resp_off.ctypes.data if resp_off is not None else None, peer_off.ctypes.data, C.byref(c), C.byref(rc_)))
        p, k = C.c_void_p(None), C.c_uint64(0)
        dt, fn = self._results_form()
        self._chk(fn(self._h, C.byref(p), C.byref(k)))
        outs = np.frombuffer((C.c_char * (k.value * dt.itemsize)).from_address(p.value), dtype=dt, count=k.value) if k.value else np.zeros(0, dt)
        if copy:
            outs = outs.copy()
        got_ents = ents[: min(int(c.n_ents), len(ents))] if ents is not None else np.zeros(0, WIRE_ENT_DT)
        n_resp = int(rc_.n_msgs)
        return (msgs[:n], got_ents, outs, out[: int(rc_.bytes)], resp_off[: n_resp + 1] if resp_off is not None else None,
                peer_off[: self.n_peers + 1], c, rc_)

    def tick_frames(self, out: np.ndarray, frame_off: np.ndarray | None, peer_off: np.ndarray, beat_cap: int, hup_cap: int | None = None,
                    beat_bitmap: bool = False, cap: int | None = None):
        """raftq_tick_frames: the Tick, its lists (as tick_collect_lists) and the heartbeats of the first beat_cap MsgBeat groups built
        and marshalled on the device -- one submission, one wait.  out: uint8 of at least respond_cap(beat_cap) bytes (cap: what the
        call is told instead of len(out)); frame_off: uint64 [beat_cap * (N - 1) + 1] or None; peer_off: uint64 [N + 1]; all page-locked
        (engine.pinned_empty).  -> (heartbeat bytes (a view of out), frame_off[:n_frames + 1] | None, peer_off, counts, hups view u32,
        n_hup, beats view u32 | bitmap view u64, n_beat); the list views are the library's memory, valid until the next Tick call.
        With voter masks loaded and set_tick_voters on, the frames go to each group's members only: frame_off stays positional (one
        entry per slot, a non-member's slot has zero length) and counts.n_msgs is the number of frames that have bytes"""
        assert peer_off.dtype == np.uint64 and len(peer_off) >= self.n_peers + 1
        assert out is None or out.dtype == np.uint8
        assert frame_off is None or (frame_off.dtype == np.uint64 and len(frame_off) >= int(beat_cap) * (self.n_peers - 1) + 1)
        hc = self.n_groups if hup_cap is None else int(hup_cap)
        nh, nb, c = C.c_uint64(0), C.c_uint64(0), _lib.WireCounts()
        self._chk(self._lib.raftq_tick_frames(self._h, _lib.TICK_BEAT_BITMAP if beat_bitmap else 0, hc, int(beat_cap), C.byref(nh), C.byref(nb),
                                              out.ctypes.data if out is not None and len(out) else None,
                                              (len(out) if out is not None else 0) if cap is None else int(cap),
                                              frame_off.ctypes.data if frame_off is not None else None, peer_off.ctypes.data, C.byref(c)))
        ph, pb, pm = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None)
        lh, lb, lm = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.raftq_last_tick_lists(self._h, C.byref(ph), C.byref(lh), C.byref(pb), C.byref(lb), C.byref(pm), C.byref(lm)))

        def view(p, n, dt):
            if not n:
                return np.empty(0, dtype=dt)
            return np.frombuffer((C.c_char * (int(n) * np.dtype(dt).itemsize)).from_address(p.value), dtype=dt)

        hups = view(ph, lh.value, np.uint32)
        second = view(pm, lm.value, np.uint64) if beat_bitmap else view(pb, lb.value, np.uint32)
        n_frames = int(peer_off[self.n_peers])  # the slots: c.n_msgs of them have bytes (all, unless the round went to members only)
        return (out[: int(c.bytes)] if out is not None else np.zeros(0, np.uint8), frame_off[: n_frames + 1] if frame_off is not None else None,
                peer_off[: self.n_peers + 1], c, hups, int(nh.value), second, int(nb.value))

    def tick_elect_frames(self, camp: np.ndarray | None, out: np.ndarray, frame_off: np.ndarray | None, peer_off: np.ndarray, hup_cap: int,
                          beat_cap: int, beat_bitmap: bool = False, cap: int | None = None):
        """raftq_tick_elect_frames: tick_frames plus the election round -- Step(MsgHup) applied on the device to the first hup_cap
        MsgHup groups and their N - 1 MsgVotes marshalled behind the heartbeats; one submission, one wait.  camp: STEP_OUT_S_DT
        [hup_cap] (None only when hup_cap == 0); out: uint8 of at least respond_cap(beat_cap + hup_cap) bytes (cap: what the call is
        told instead of len(out)); frame_off: uint64 [(beat_cap + hup_cap) * (N - 1) + 1] or None; peer_off: uint64 [2 * (N + 1)];
        all page-locked (engine.pinned_empty).  -> (bytes (a view of out), frame_off[:n_frames + 1] | None, peer_off, counts,
        camp[:min(n_hup, hup_cap)], hups view u32, n_hup, beats view u32 | bitmap view u64, n_beat); the list views are the
        library's memory, valid until the next Tick call"""
        from .step import OUT_S_DT

        n_max = (int(beat_cap) + int(hup_cap)) * (self.n_peers - 1)
        assert peer_off.dtype == np.uint64 and len(peer_off) >= 2 * (self.n_peers + 1)
        assert out is None or out.dtype == np.uint8
        assert frame_off is None or (frame_off.dtype == np.uint64 and len(frame_off) >= n_max + 1)
        assert camp is None or (camp.dtype == OUT_S_DT and len(camp) >= int(hup_cap))
        nh, nb, c = C.c_uint64(0), C.c_uint64(0), _lib.WireCounts()
        self._chk(self._lib.raftq_tick_elect_frames(self._h, _lib.TICK_BEAT_BITMAP if beat_bitmap else 0, int(hup_cap), int(beat_cap), C.byref(nh),
                                                    C.byref(nb), camp.ctypes.data if camp is not None and len(camp) else None,
                                                    out.ctypes.data if out is not None and len(out) else None,
                                                    (len(out) if out is not None else 0) if cap is None else int(cap),
                                                    frame_off.ctypes.data if frame_off is not None else None, peer_off.ctypes.data, C.byref(c)))
        ph, pb, pm = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None)
        lh, lb, lm = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.raftq_last_tick_lists(self._h, C.byref(ph), C.byref(lh), C.byref(pb), C.byref(lb), C.byref(pm), C.byref(lm)))

        def view(p, n, dt):
            if not n:
                return np.empty(0, dtype=dt)
            return np.frombuffer((C.c_char * (int(n) * np.dtype(dt).itemsize)).from_address(p.value), dtype=dt)

        hups = view(ph, lh.value, np.uint32)
        second = view(pm, lm.value, np.uint64) if beat_bitmap else view(pb, lb.value, np.uint32)
        n_frames = int(peer_off[2 * self.n_peers + 1])  # the slots of both sections: c.n_msgs of them have bytes
        n_vb = min(int(nh.value), int(hup_cap))
        return (out[: int(c.bytes)] if out is not None else np.zeros(0, np.uint8), frame_off[: n_frames + 1] if frame_off is not None else None,
                peer_off[: 2 * (self.n_peers + 1)], c, camp[:n_vb] if camp is not None else np.zeros(0, OUT_S_DT), hups, int(nh.value), second,
                int(nb.value))

    def propose_frames(self, props: np.ndarray, prop_ents: np.ndarray, msgs: np.ndarray, ents: np.ndarray, pool: np.ndarray, out: np.ndarray,
                       off: np.ndarray | None = None, counts=None):
        """raftq_propose_frames: appendEntry + bcastAppend for props[] on the device, written into the encoder's input, and the
        marshal of msgs[] + those MsgApps -- one submission, one wait.  All arrays page-locked (engine.pinned_*).
        -> (stream view of out, frame_off | None, counts).  A call that raises has appended nothing; pass `counts` (a
        _lib.WireCounts) to learn counts.bytes, the size needed, when out was too small: retrying with an out of that size is safe.
        Under set_propose_forward -> (stream, frame_off | None, counts, outcomes): one PROP_* byte per record"""
        assert props.dtype == PROP_DT and prop_ents.dtype == PROP_ENT_DT and msgs.dtype == WIRE_MSG_DT and ents.dtype == WIRE_ENT_DT
        c = _lib.WireCounts() if counts is None else counts
        self._chk(self._lib.raftq_propose_frames(self._h, props.ctypes.data if len(props) else None, len(props),
                                                 prop_ents.ctypes.data if len(prop_ents) else None, len(prop_ents),
                                                 msgs.ctypes.data if len(msgs) else None, len(msgs), ents.ctypes.data if len(ents) else None, len(ents),
                                                 pool.ctypes.data if len(pool) else None, len(pool), out.ctypes.data, len(out),
                                                 off.ctypes.data if off is not None else None, C.byref(c)))
        if self._propose_forward:
            return out[: int(c.bytes)], off, c, self.propose_outcomes()
        return out[: int(c.bytes)], off, c

    def step_stage_wire(self, n_cap: int, nbytes_cap: int):
        """the arrays the next step_submit_wire_staged() takes (raftq_step_stage_wire) -> (frame_off uint64[n_cap + 1],
        stream uint8[nbytes_cap]); views of device memory behind a large BAR: write-only"""
        po, ps = C.c_void_p(None), C.c_void_p(None)
        self._chk(self._lib.raftq_step_stage_wire(self._h, int(n_cap), int(nbytes_cap), C.byref(po), C.byref(ps)))
        off = np.frombuffer((C.c_char * ((n_cap + 1) * 8)).from_address(po.value), dtype=np.uint64, count=n_cap + 1)
        stream = np.frombuffer((C.c_char * max(nbytes_cap, 1)).from_address(ps.value), dtype=np.uint8, count=nbytes_cap)
        return off, stream

    def step_submit_wire_staged(self, off: np.ndarray, stream: np.ndarray, n: int, nbytes: int) -> None:
        """submit the first n frames / nbytes bytes of step_stage_wire()'s arrays, in place"""
        self._chk(self._lib.raftq_step_submit_wire(self._h, stream.ctypes.data, int(nbytes), off.ctypes.data, int(n)))

    def step_wire_msgs(self) -> np.ndarray:
        p, k = C.c_void_p(None), C.c_uint64(0)
        self._chk(self._lib.raftq_step_wire_msgs(self._h, C.byref(p), C.byref(k)))
        if k.value == 0:
            return np.zeros(0, WIRE_MSG_DT)
        buf = (C.c_char * (k.value * 64)).from_address(p.value)
        return np.frombuffer(buf, dtype=WIRE_MSG_DT, count=k.value).copy()

    def step_wire_entries(self) -> np.ndarray:
        p, k = C.c_void_p(None), C.c_uint64(0)
        self._chk(self._lib.raftq_step_wire_entries(self._h, C.byref(p), C.byref(k)))
        if k.value == 0:
            return np.zeros(0, WIRE_ENT_DT)
        buf = (C.c_char * (k.value * 32)).from_address(p.value)
        return np.frombuffer(buf, dtype=WIRE_ENT_DT, count=k.value).copy()

    # -- walpb.Record <-> WAL frames ------------------------------------------------------------
    def wal_encode(self, recs: np.ndarray, pool=b"", prev_crc: int = 0, out: np.ndarray | None = None,
                   off: np.ndarray | None = None):
        """wal.Save for a batch -> (bytes uint8[], frame_off, last_crc); `out` as in wire_encode"""
        r = np.ascontiguousarray(recs, dtype=WAL_REC_DT)
        p = _u8(pool)
        if off is None:
            off = np.zeros(len(r) + 1, np.uint64)
        c = _lib.WalCounts()
        args = (self._h, _p(r), len(r), _p(p), len(p), int(prev_crc))
        if out is not None:
            self._chk(self._lib.raftq_wal_encode(*args, _ptr(out), len(out), _ptr(off), C.byref(c)))
            return out[: int(c.bytes)], off, int(c.last_crc)
        rc = self._lib.raftq_wal_encode(*args, None, 0, _ptr(off), C.byref(c))
        if rc == 0:
            return np.zeros(0, np.uint8), off, int(c.last_crc)
        if c.bytes == 0:
            self._chk(rc)
        out = np.zeros(int(c.bytes), np.uint8)
        self._chk(self._lib.raftq_wal_encode(*args, _ptr(out), len(out), _ptr(off), C.byref(c)))
        return out, off, int(c.last_crc)

    def wal_encode_begin(self, recs: np.ndarray, pool: np.ndarray, prev_crc: int, out: np.ndarray, off: np.ndarray | None = None) -> None:
        """raftq_wal_encode_begin: enqueue, do not wait; every array page-locked (engine.pinned_*) and kept alive until
        wal_encode_end()"""
        assert recs.dtype == WAL_REC_DT and pool.dtype == np.uint8 and out.dtype == np.uint8
        self._wal_begun = (recs, pool, out, off)
        self._chk(self._lib.raftq_wal_encode_begin(self._h, recs.ctypes.data, len(recs), pool.ctypes.data if len(pool) else None, len(pool),
                                                   int(prev_crc), out.ctypes.data, len(out), off.ctypes.data if off is not None else None))

    def wal_encode_end(self):
        """-> (bytes written, last_crc) of the encode wal_encode_begin() enqueued"""
        c = _lib.WalCounts()
        rc = self._lib.raftq_wal_encode_end(self._h, C.byref(c))
        self._wal_begun = None
        self._chk(rc)
        return int(c.bytes), int(c.last_crc)

    def wal_decode(self, data, frame_off, prev_crc: int = 0, recs: np.ndarray | None = None):
        """w.ReadAll for a batch -> (recs, n_valid, last_crc)"""
        b = _u8(data)
        off = np.ascontiguousarray(frame_off, np.uint64)
        n = len(off) - 1
        if recs is None:
            recs = np.zeros(n, WAL_REC_DT)
        c = _lib.WalCounts()
        self._chk(self._lib.raftq_wal_decode(self._h, _p(b), len(b), _ptr(off), n, int(prev_crc), _p(recs), C.byref(c)))
        return recs[:n], int(c.n_valid), int(c.last_crc)
