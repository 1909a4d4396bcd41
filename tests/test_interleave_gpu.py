"""GPU: every writer of a handle interleaved with Step on ONE WireEngine with the switches on (raftq_step_set_msg_flags,
raftq_step_set_props, raftq_respond_set_lead, raftq_respond_set_props, raftq_propose_set_forward; voter masks with their three
switches and raftq_set_check_quorum by case), against tests/ref_interleave.py, byte for byte.

A group's Step record holds copies of what the dense kernels own; the copies stay true only because every writer that is not Step
calls dense_changed() and Step stores back what it changed, the self-max word and the narrow word cleared with a match row.  Each
case runs its schedule -- about 35 moves, a Step batch (or a pipelined pair, one of them with a run longer than kMaxRun) behind
every move -- and holds, after EVERY move and after EVERY batch:
  the call's own outputs       result records, frame streams, offsets, peer offsets, lists, counts
  the whole handle             tests/_stepgen.assert_same_state, read_voters, read_tick's role and elapsed, read_activity
  two what-if sweeps           RAFTQ_SWEEP_COMMIT | VOTES | CHANGED | NO_ADOPT, plain and gated: whole arrays, the changed list, the
                               tally -- what finds a self-max or narrow word left standing over rows that moved
The cases with PreVote, leadership transfer, ReadIndex and the fused Tick calls on (ref_interleave.EXTENDED) also hold, after every
move and every batch, raftq_read_transfer and -- in the safe mode -- raftq_read_reads' seq, acked and confirmed; their moves add
raftq_load_transfer, raftq_load_reads, each switch turned off and on, a window without PreVote, raftq_tally_rebuild and every call the
switches close.  The tally word is held one-sidedly in every case: true right behind its build, unchanged across every move whose
contract keeps it, never asserted across a Step batch.
That the batches can tell each move from its absence is shown on the reference alone by tests/test_interleave_ref.py."""
import time

import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd._lib import CYCLE_SEGMENTED, RAFTQ_EINVAL, SWEEP_CHANGED, SWEEP_COMMIT, SWEEP_GATED, SWEEP_NO_ADOPT, SWEEP_VOTES
from tests import _refusals, _stepgen
from tests import ref_interleave as I

pytestmark = pytest.mark.gpu

ANSWERED = 0x10  # RAFTQ_OUTF_ANSWERED
# include/raftq.h, the tally mirror: Step and a voter delta that resets a slot end it until the next build.  Step is also what a
# device-built election round and raftq_step_frames_respond run; a clone has its source's word; raftq_tally_rebuild may set it.
TALLY_MAY_END = ("voter_deltas", "tick_elect", "respond", "clone", "tally_rebuild")
STATE_FIELDS = ("term", "vote", "lead", "last_index", "last_term", "first_idx", "role", "elapsed", "committed")


def _first(got, want):
    """the first group in which two [G] or [N, G] arrays differ, for a failure's text"""
    bad = np.asarray(got) != np.asarray(want)
    if bad.ndim == 2:
        bad = bad.any(axis=0)
    g = int(np.flatnonzero(bad)[0])
    return f"first at group {g}: got {np.asarray(got)[..., g]}, want {np.asarray(want)[..., g]}, {int(bad.sum())} groups differ"


def _engine(ref, loaded=True):
    """a WireEngine with the case's switches; loaded: with the reference's state (False: what a clone's destination starts with)"""
    from raftsql_amd.wire import WireEngine

    s = ref.s
    e = WireEngine(s.G, s.N, s.self_peer)  # (msg_flags: raftq_step_set_msg_flags)
    e.set_timers(I.ET, I.HB, I.SEED)
    if ref.ext:  # in front of the load: raftq_load_roles takes role 3 only under raftq_set_pre_vote
        e.set_check_quorum(True)
        e.set_pre_vote(ref.pv)
        e.set_lead_transfer(ref.lt)
        e.set_read_index(ref.ri)
        if ref.checks:
            e.set_tick_checks(s.G)
    if loaded:
        _stepgen.load_engine(e, s)
    if ref.cq:
        e.set_check_quorum(True)
        if loaded:
            e.load_activity(ref.active, ref.le)
            if ref.lt:
                e.load_transfer(ref.transferee)
            if ref.ri == I.SAFE:
                e.load_reads(ref.seq, ref.acked)
    e.set_step_props(True)
    e.set_respond_lead(True)
    e.set_respond_props(True)
    e.set_propose_forward(True)
    if loaded and ref.voters is not None:
        e.load_voters(ref.voters)
    if ref.voters is not None or ref.saved is not None:
        e.set_step_voters(True)
        e.set_tick_voters(True)
        e.set_bcast_voters(True)
    return e


def _held(e, ref, what):
    """the whole handle against the reference"""
    s = ref.s
    got = e.read_node()
    for k in STATE_FIELDS:
        assert np.array_equal(got[k], getattr(s, k)), f"{what}: {k}, {_first(got[k], getattr(s, k))}"
    for k, g, w in (("match", e.read_match(), s.match), ("votes", e.read_votes(), s.votes), ("voters", e.read_voters(), ref.masks)):
        assert np.array_equal(g, w), f"{what}: {k}, {_first(g, w)}"
    _stepgen.assert_same_state(e, s)
    _, el, role = e.read_tick()
    assert np.array_equal(role, s.role) and np.array_equal(el, s.elapsed), f"{what}: read_tick"
    if ref.cq:
        ac, le = e.read_activity()
        assert np.array_equal(ac, ref.active), f"{what}: active, {_first(ac, ref.active)}"
        assert np.array_equal(le, ref.le), f"{what}: lead_elapsed, {_first(le, ref.le)}"
    _held_more(e, ref, what)


def _held_more(e, ref, what):
    """what the three switches hold: the transferees, and in the safe mode the read records with confirmed() over the voters Step runs over"""
    if ref.lt:
        tr = e.read_transfer()
        assert np.array_equal(tr, ref.transferee), f"{what}: transferee, {_first(tr, ref.transferee)}"
    if ref.ri == I.SAFE:
        seq, acked, conf = e.read_reads()
        assert np.array_equal(seq, ref.seq), f"{what}: seq, {_first(seq, ref.seq)}"
        assert np.array_equal(acked, ref.acked), f"{what}: acked, {_first(acked, ref.acked)}"
        want = I.RI.confirmed_of(ref.extra, ref.voters, ref.s.N)
        assert np.array_equal(conf, want), f"{what}: confirmed, {_first(conf, want)}"


def _refused_with(f, word, what):
    from raftsql_amd._lib import RAFTQ_ESTATE
    from raftsql_amd.engine import RaftqError

    with pytest.raises(RaftqError) as ei:
        f()
    assert ei.value.code == RAFTQ_ESTATE and word in str(ei.value), f"{what}: expected RAFTQ_ESTATE naming '{word}', got {ei.value.code}: {ei.value}"


def _closed(e, mv, ref, what):
    """every call the case's switches close is refused with its word (the handle is then held unchanged by the caller's _held)"""
    from tests import test_tick_elect_gpu as TE
    from tests import test_tick_frames_gpu as TF

    a, s = mv.args, ref.s
    bf, be = TF.Bufs(e, s.G), TE.Bufs(e, s.G, s.G)
    frames = lambda: e.tick_frames(bf.out, bf.off[: bf.n_max + 1], bf.po, s.G, cap=bf.cap)  # noqa: E731
    elect = lambda: e.tick_elect_frames(be.camp[: s.G], be.out, be.off[: be.n_max + 1], be.po, s.G, s.G, cap=be.cap)  # noqa: E731

    def propose():
        room = (s.N - 1) * (len(a["pool"]) + 64 * len(a["pe"])) + 128 * len(a["props"]) * (s.N - 1) + 4096
        _refusals.ProposeArgs(a["props"], a["pe"], a["pool"], a["hm"], a["he"], s.N, room).whole(e)

    calls = {"tick_collect": e.tick_collect, "tick_collect_lists": e.tick_collect_lists, "tick_frames": frames, "tick_elect_frames": elect,
             "propose_frames": propose, "set_check_quorum(0)": lambda: e.set_check_quorum(False)}
    tick_before = e.read_tick()
    for name, word in a["calls"]:
        opened = name.endswith("+checks")
        if opened:  # raftq_tick_set_checks lets the call past CheckQuorum and PreVote: what is left is the safe mode's refusal
            e.set_tick_checks(s.G)
        try:
            _refused_with(calls[name.split("+")[0]], word, f"{what}: {name}")
        finally:
            if opened:
                e.set_tick_checks(0)
    for x, y in zip(tick_before, e.read_tick()):
        assert np.array_equal(x, y), f"{what}: a refused Tick call ticked"
    assert bf.canaries_ok() and (be.out == be.out[0]).all(), f"{what}: a refused call wrote"


def _what_if(e, ref, what):
    """the two sweeps that adopt nothing, then a tally alone: raftq_read_committed reads the live buffer again (behind a
    RAFTQ_SWEEP_NO_ADOPT sweep it reads the evaluated one until Step or a sweep moves the live state)"""
    w = I.what_if(ref)
    outcome, won, lost = w["outcome"]
    for gated in (False, True):
        c = e.sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED | SWEEP_NO_ADOPT | (SWEEP_GATED if gated else 0))
        new, n, at = w[gated]
        words = f"(narrow {e.narrow()}, self_max {e.self_max()})"
        got = e.read_committed()
        assert np.array_equal(got, new), f"{what}: what-if sweep gated={gated}, {_first(got, new)} {words}"
        got_o = e.read_outcome()
        assert np.array_equal(got_o, outcome), f"{what}: what-if tally gated={gated}, {_first(got_o, outcome)}"
        assert (c.n_changed, c.n_won, c.n_lost) == (n, won, lost), f"{what}: what-if counts gated={gated} {c} {words}"
        adv, total = e.collect_changed()
        assert total == len(at) and np.array_equal(adv["group"], at.astype(np.uint64)), f"{what}: what-if changed list gated={gated} {words}"
        assert np.array_equal(adv["old_commit"], ref.s.committed[at]) and np.array_equal(adv["new_commit"], new[at]), f"{what}: what-if changed list {words}"
    e.sweep(SWEEP_VOTES)
    assert np.array_equal(e.read_committed(), ref.s.committed), f"{what}: the live commit indices behind the what-if sweeps"


def _records(got, want, m, what):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        i = int(bad[0])
        assert False, f"{what}: {len(bad)} records differ, first at record {i}, group {int(m['group'][i])}: {m[i]} -> got {got[i]}, want {want[i]}"


def _tick_lists(e, mv, hups, nh, second, nb, what):
    w = mv.want
    assert (nh, nb) == (w["n_hup"], w["n_beat"]), f"{what}: tick counts {(nh, nb)}, want {(w['n_hup'], w['n_beat'])}"
    assert np.array_equal(hups, w["hups"]) and np.array_equal(second, w["beats"]), f"{what}: tick lists"
    assert np.array_equal(e.read_tick()[0], w["action"]), f"{what}: tick actions, {_first(e.read_tick()[0], w['action'])}"
    if "checks" in w:  # under raftq_tick_set_checks: the third list, left in place
        ids, n = e.last_tick_checks()
        assert n == len(w["checks"]) and np.array_equal(ids, w["checks"]), f"{what}: the list of failed checks, {n} of them, want {len(w['checks'])}"


def _frames(got_s, got_po, c, b, n_max, mv, what):
    w = mv.want
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (w["n_frames"], 0, 0, len(w["stream"])), f"{what}: frame counts"
    assert np.array_equal(got_po, w["peer_off"]), f"{what}: peer offsets {got_po}, want {w['peer_off']}"
    assert bytes(got_s) == bytes(w["stream"]), f"{what}: frame stream"
    assert np.array_equal(b.off[: n_max + 1], w["off"]), f"{what}: frame offsets"


def _apply(e, mv, ref, what):
    """the move's call on the handle, its own outputs held to the reference's -> the handle the run goes on with"""
    a, w, kind = mv.args, mv.want, mv.kind
    s = ref.s
    if kind == "deltas":
        e.apply_deltas(a["group"], a["peer"], a["match"])
    elif kind == "vote_deltas":
        e.apply_vote_deltas(a["group"], a["peer"], a["vote"])
    elif kind == "sweep":
        c = e.sweep(SWEEP_COMMIT | SWEEP_GATED | SWEEP_CHANGED)
        got = e.read_committed()
        assert np.array_equal(got, w["committed"]), f"{what}: {_first(got, w['committed'])}"
        adv, total = e.collect_changed()
        assert c.n_changed == w["n_changed"] == total, f"{what}: counts {c.n_changed} {total}, want {w['n_changed']}"
        assert all(np.array_equal(adv[k], w[k]) for k in ("group", "old_commit", "new_commit")), f"{what}: changed list"
    elif kind == "cycle":
        _, total, cnt = e.cycle_packed(SWEEP_COMMIT | SWEEP_GATED | SWEEP_VOTES | CYCLE_SEGMENTED, e.pack_deltas16(a["group"], a["peer"], a["match"]),
                                       e.pack_vote_deltas(a["vgroup"], a["vpeer"], a["vote"]), cap=s.G, inplace=True)
        adv = e.advance_list_from_segments()
        assert total == w["total"] and (cnt.n_changed, cnt.n_won, cnt.n_lost) == w["counts"], f"{what}: counts {total} {cnt}, want {w['total']} {w['counts']}"
        assert np.array_equal(adv["group"].astype(np.uint64), w["group"]), f"{what}: advance list"
        assert np.array_equal(adv["new_commit"], w["new_commit"]) and np.array_equal(adv["advanced_by"], w["advanced_by"]), f"{what}: advance list"
    elif kind == "roles":
        e.load_roles(a["role"], a["elapsed"])
    elif kind == "campaign":
        e.campaign(a["groups"], s.self_peer)
    elif kind == "term_deltas":
        e.apply_term_deltas(a["group"], a["cur_term"], a["first_idx"])
    elif kind == "log_deltas":
        got = e.apply_log_deltas(a["group"], a["last_index"], a["last_term"], a["commit_to"])
        assert np.array_equal(got, w["committed"]), f"{what}: commit indices returned, first at record {int(np.flatnonzero(got != w['committed'])[0])}"
    elif kind == "log_deltas_nowait":
        e.apply_log_deltas_nowait(a["group"], a["last_index"], a["last_term"], a["commit_to"])
    elif kind == "voter_deltas":
        e.apply_voter_deltas(e.pack_voter_deltas(a["group"], a["voters"], a["reset"]))
    elif kind == "unmask":
        e.load_voters(None)
    elif kind == "remask":
        e.load_voters(a["voters"])
    elif kind == "tick":
        assert e.tick() == (w["n_hup"], w["n_beat"]), f"{what}: tick counts"
        assert np.array_equal(e.read_tick()[0], w["action"]), f"{what}: tick actions, {_first(e.read_tick()[0], w['action'])}"
        for name, collect in (("hups", e.collect_hups), ("beats", e.collect_beats), ("checks", e.collect_checks)):
            ids, n = collect()
            assert n == len(w[name]) and np.array_equal(ids, w[name]), f"{what}: the list of {name}"
    elif kind == "tick_lists":
        _tick_lists(e, mv, *e.tick_collect_lists(), what)
    elif kind == "tick_frames":
        from tests import test_tick_frames_gpu as TF

        b = TF.Bufs(e, s.G)
        got_s, _, got_po, c, hups, nh, second, nb = e.tick_frames(b.out, b.off[: b.n_max + 1], b.po, s.G, cap=b.cap)
        _tick_lists(e, mv, hups, nh, second, nb, what)
        _frames(got_s, got_po, c, b, b.n_max, mv, what)
        assert b.canaries_ok(), f"{what}: canaries"
    elif kind == "tick_elect":
        from tests import test_tick_elect_gpu as TE

        b = TE.Bufs(e, s.G, s.G)
        got_s, _, got_po, c, camp, hups, nh, second, nb = e.tick_elect_frames(b.camp[: s.G], b.out, b.off[: b.n_max + 1], b.po, s.G, s.G, cap=b.cap)
        _tick_lists(e, mv, hups, nh, second, nb, what)
        _frames(got_s, got_po, c, b, b.n_max, mv, what)
        assert camp.tobytes() == w["camp"].tobytes(), f"{what}: campaign records"
        assert b.canaries_ok(s.N), f"{what}: canaries"
    elif kind == "propose":
        slots = len(a["hm"]) + len(a["props"]) * (s.N - 1)
        room = (s.N - 1) * (len(a["pool"]) + 64 * len(a["pe"])) + 128 * slots + 4096
        got = _refusals.ProposeArgs(a["props"], a["pe"], a["pool"], a["hm"], a["he"], s.N, room).whole(e)
        assert (got["n_msgs"], got["n_ents"], got["bytes"]) == (w["n_msgs"], w["n_ents"], w["bytes"]), f"{what}: counts {got['n_msgs'], got['n_ents'], got['bytes']}"
        assert bytes(got["stream"]) == bytes(w["stream"]), f"{what}: frame stream"
        assert np.array_equal(got["off"], w["off"]), f"{what}: frame offsets"
        out = e.propose_outcomes()
        assert np.array_equal(out, w["outcomes"]), f"{what}: outcomes, first at record {int(np.flatnonzero(out != w['outcomes'])[0])}"
    elif kind == "respond":
        from tests.test_respond_props_gpu import _call, _held_to

        e.campaign(a["campaign"], s.self_peer)
        n_e = len(W.wire_decode(a["stream"], a["off"])[1])
        got = _call(e, a["stream"], a["off"], n_e + 1, a["at_tail"])
        outs = got[2].copy()
        ans = (outs["flags"] & ANSWERED) != 0
        outs["flags"] &= np.uint8(~ANSWERED & 0xFF)
        _records(outs, w["outs"], w["rec"], f"{what}: result records")  # (names the group; _held_to then holds every output)
        bad = np.flatnonzero(ans != w["answered"])
        assert not len(bad), f"{what}: answered flags, first at record {int(bad[0])}, group {int(w['rec']['group'][bad[0]])}"
        _held_to(e, w, got, a["stream"], a["off"], what)
    elif kind == "clone":
        new = _engine(ref, loaded=False)
        new.clone_state_from(e)
        if ref.cq:
            ac, le = new.read_activity()
            assert np.array_equal(ac, ref.active) and np.array_equal(le, ref.le), f"{what}: the activity words the clone copied"
        _held_more(new, ref, f"{what}: what the clone copied")  # (the transferee travels with the word, the records with the handle)
        new.load_roles(s.role, s.elapsed)
        new.load_node(s.term, s.vote, s.lead, s.last_index, s.last_term)
        if ref.cq:
            new.load_activity(ref.active, ref.le)
        e.close()
        return new
    elif kind == "narrow_rebuild":
        e.narrow_rebuild()
    elif kind == "refused":
        from raftsql_amd.engine import RaftqError

        with pytest.raises(RaftqError) as ei:
            e.step_batch(np.array(a["bad"]))
        assert ei.value.code == RAFTQ_EINVAL, f"{what}: {ei.value}"
    elif kind == "activity":
        e.load_activity(a["active"], a["lead_elapsed"])
    elif kind == "cq_toggle":
        e.set_check_quorum(False)
        e.set_check_quorum(True)
    elif kind == "transfer":
        e.load_transfer(a["transferee"])
    elif kind == "reads":
        e.load_reads(a["seq"], a["acked"])
    elif kind == "lt_toggle":
        e.set_lead_transfer(False)
        e.set_lead_transfer(True)
    elif kind == "ri_toggle":
        e.set_read_index(a["other"])
        e.set_read_index(ref.ri)
    elif kind == "pv_off":
        e.set_pre_vote(False)
    elif kind == "pv_on":
        e.set_pre_vote(True)
    elif kind == "tally_rebuild":
        assert e.tally_rebuild() and e.tally(), f"{what}: the tally word right behind its build"
    elif kind == "closed":
        _closed(e, mv, ref, what)
    else:
        raise AssertionError(kind)
    return e


@pytest.mark.parametrize("case", list(I.CASES))
def test_every_writer_interleaved_with_step(oracle, gpu_engine_cls, monkeypatch, case):
    if I.CASES[case]["walk"] == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)
    sch = I.schedule(case)
    t0 = time.perf_counter()
    e = _engine(sch.start)
    try:
        _held(e, sch.start, f"{case}: the loaded state")
        for k, mv in enumerate(sch.moves):
            what = f"{case}, move {k} ({mv.kind})"
            tally = e.tally()
            e = _apply(e, mv, mv.after, what)
            if mv.kind not in TALLY_MAY_END:  # (never asserted across a Step batch: Step ends the mirror by contract)
                assert e.tally() == tally, f"{what}: the tally word was {tally} in front of the move and is {e.tally()} behind it"
            _held(e, mv.after, f"{what}: behind the move")
            _what_if(e, mv.after, f"{what}: behind the move")
            if len(mv.batches) == 1:
                got = [e.step_batch(np.array(mv.batches[0]))[0]]
            else:  # two submitted, then two collected
                for m in mv.batches:
                    e.step_submit(np.array(m))
                got = [e.step_collect()[0] for _ in mv.batches]
            for j, (g, w, m) in enumerate(zip(got, mv.wants, mv.batches)):
                _records(g, w, m, f"{what}: Step batch {j} of {len(mv.batches)} behind the move")
            _held(e, mv.after_step, f"{what}: behind the Step batch")
            _what_if(e, mv.after_step, f"{what}: behind the Step batch")
    finally:
        e.close()
    print(f"{case}: {len(sch.moves)} moves, reference {sch.ref_seconds:.2f} s, device side with its checks {time.perf_counter() - t0:.2f} s")
