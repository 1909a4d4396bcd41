"""CPU: the schedules of tests/ref_interleave.py discriminate -- what keeps tests/test_interleave_gpu.py honest.  A move that the batch
behind it cannot tell from its absence would let a walk that skipped the mirror refresh pass; so for EVERY state-changing move of
every schedule the batch behind it, stepped by the reference on the state as it stood BEFORE the move, must give other records in at
least one group the move changed.  The schedules with PreVote, leadership transfer and ReadIndex on are held to the same, to every
Step rule those switches enable (a batch somewhere changes when the rule is left out) and to the result kinds the switches add.
Nothing in here touches the device."""
import numpy as np
import pytest

from raftsql_amd import step as S
from tests import ref_interleave as I
from tests import ref_raft_py as R

SCHEDULES = sorted(set(c["schedule"] for c in I.CASES.values()))
EXTENDED = sorted(set(I.CASES[k]["schedule"] for k in I.EXTENDED))


def test_the_cases_are_the_issues():
    assert {k: (c["n"], c["me"], c["masks"], c["cq"], c["walk"]) for k, c in I.CASES.items() if k not in I.EXTENDED} == {
        "n3": (3, 1, False, False, "lists"), "n9": (9, 8, False, False, "lists"), "n5-masked": (5, 4, True, False, "lists"),
        "n3-cq": (3, 1, False, True, "lists"), "n5-masked-cq": (5, 4, True, True, "lists"), "n5-masked-cq-sort": (5, 4, True, True, "sort")}
    assert I.CASES["n5-masked-cq-sort"]["schedule"] == I.CASES["n5-masked-cq"]["schedule"], "the sorted walk runs the same schedule"
    assert I.G == 1027 and (I.ET, I.HB, I.SEED) == (10, 1, 0x5EED)
    assert I.schedule("n5-masked-cq-sort") is I.schedule("n5-masked-cq"), "built once"
    # the cases with PreVote, leadership transfer and ReadIndex: N, self, masks, PreVote, transfer, read mode, fused Ticks, walk
    assert {k: (c["n"], c["me"], c["masks"], c["pv"], c["lt"], c["ri"], c["checks"], c["walk"]) for k, c in I.CASES.items() if k in I.EXTENDED} == {
        "n3-all-safe": (3, 1, False, True, True, I.SAFE, False, "lists"), "n5-masked-all-safe": (5, 4, True, True, True, I.SAFE, False, "lists"),
        "n5-masked-all-safe-sort": (5, 4, True, True, True, I.SAFE, False, "sort"),
        "n9-lt-lease-checks": (9, 8, False, False, True, I.LEASE, True, "lists"), "n3-pv-lease-checks": (3, 1, False, True, False, I.LEASE, True, "lists")}
    assert all(I.CASES[k]["cq"] for k in I.EXTENDED), "every one of them runs under CheckQuorum"
    assert I.schedule("n5-masked-all-safe-sort") is I.schedule("n5-masked-all-safe"), "the same schedule object"
    assert (I.SAFE, I.LEASE) == (1, 2)
    for k in I.EXTENDED:
        c, kinds = I.CASES[k], I.kinds_of(k)
        assert "cq_toggle" not in kinds and ("propose" in kinds) == (not c["lt"]) and ("reads" in kinds) == (c["ri"] == I.SAFE)
        assert ("tick" in kinds) == (not c["checks"]) and all((t in kinds) == c["checks"] for t in ("tick_lists", "tick_frames", "tick_elect"))
        assert all(t in kinds for t in ("clone", "deltas", "vote_deltas", "sweep", "cycle", "campaign", "term_deltas", "log_deltas", "log_deltas_nowait",
                                        "narrow_rebuild", "refused", "roles", "activity", "ri_toggle", "tally_rebuild", "closed"))
        assert all((t in kinds) == c["lt"] for t in ("transfer", "lt_toggle")) and all((t in kinds) == c["pv"] for t in ("pv_off", "pv_on"))
        assert all((t in kinds) == c["masks"] for t in ("voter_deltas", "unmask", "remask"))


@pytest.mark.parametrize("case", SCHEDULES)
def test_every_kind_occurs_and_the_batches_have_their_shape(oracle, case):
    sch = I.schedule(case)
    got = I.counts(sch)
    for kind, k in I.kinds_of(case).items():
        assert got.get(kind, 0) >= k, (kind, got)
        assert k >= 2 or kind in I.ONCE + I.ELAPSED_ONLY, kind
    assert sum(got.get(k, 0) for k in I.TICKS) >= 2
    assert len(sch.moves) >= 30
    kinds = [mv.kind for mv in sch.moves]
    assert kinds != sorted(kinds) and len(set(zip(kinds, kinds[1:]))) > len(set(kinds)), "the order comes from the seed, not from a cycle"
    if I.CASES[case]["masks"]:
        at = kinds.index("unmask")
        assert kinds[at + 1] == "remask" and sch.moves[at].after.voters is None and sch.moves[at + 1].after.voters is not None
        assert not np.array_equal(sch.moves[at].before.masks, sch.moves[at].after.masks)
    if I.CASES[case].get("pv"):
        at = kinds.index("pv_off")
        off, on = sch.moves[at], sch.moves[at + 1]
        assert on.kind == "pv_on" and kinds.count("pv_off") == kinds.count("pv_on") == 1
        assert not off.after.pv and not off.after_step.pv and on.after.pv and all(mv.after.pv for mv in sch.moves if mv is not off)
        assert int((off.after.s.role == 3).sum()) >= 8, "the window has role-3 groups to take for followers"
        looked = (off.batches[0]["_pad"][:, 1] & (I.V.MSGF_SKIP | I.V.MSGF_HOLD)) == 0  # (a skipped record's type is garbage nobody reads)
        assert not np.isin(off.batches[0]["type"][looked], (S.MSG_PRE_VOTE, S.MSG_PRE_VOTE_RESP)).any()
    pairs = [mv for mv in sch.moves if len(mv.batches) == 2]
    assert len(pairs) >= 2
    for mv in pairs:  # a run longer than the list walk takes, in one of the two
        assert max(np.bincount(m["group"][m["group"] < I.G].astype(np.int64)).max() for m in mv.batches) >= I.K_RUN > 32
    for mv in sch.moves:
        assert all(len(m) <= 1024 and len(m) == len(w) for m, w in zip(mv.batches, mv.wants))
        listed = mv.changed[: I.MAX_CHANGED]
        assert np.isin(listed, mv.batches[0]["group"].astype(np.int64)).all(), (mv.kind, "a changed group without a record")
        assert not I.refuses(mv.batches[0], I.G, I.CASES[case]["n"]), "every input is in range"
        if mv.after.ext:
            assert not any(mv.after.unknown(m).any() for m in mv.batches), (mv.kind, "a kind the handle's switches do not know")


@pytest.mark.parametrize("case", SCHEDULES)
def test_every_state_changing_move_is_seen_by_the_batch_behind_it(oracle, case):
    """100 % of the moves that change state.  Exempt: the kinds that change nothing (clone, narrow_rebuild, the refused call; with the
    three switches also tally_rebuild, the closed calls and, in the lease mode, which holds no record, the switch to the other read
    mode and back) -- and a Tick that neither runs under CheckQuorum nor campaigns on the device: it moves `elapsed` alone, which Step
    without CheckQuorum neither reads nor reports, so no record CAN differ; for those it is asserted that elapsed is all that moved."""
    sch = I.schedule(case)
    seen = total = 0
    for k, mv in enumerate(sch.moves):
        if mv.kind in I.no_change(case):
            assert mv.before.same(mv.after), (k, mv.kind)
            continue
        assert not mv.before.same(mv.after), (k, mv.kind, "the move changed nothing")
        if mv.kind in I.ELAPSED_ONLY and not I.CASES[case]["cq"]:
            back = mv.after.copy()
            back.s.elapsed[:] = mv.before.s.elapsed
            assert back.same(mv.before), (k, mv.kind, "more than elapsed moved")
            continue
        total += 1
        differ = I.discriminates(mv)
        assert len(differ) >= 1 and np.isin(differ, mv.changed).all(), (case, k, mv.kind, "the batch behind the move does not read what it changed")
        seen += 1
    print(f"{case}: {seen} of {total} state-changing moves are told from their absence by the batch behind them")
    assert seen == total >= 20


@pytest.mark.parametrize("case", EXTENDED)
def test_no_move_under_the_three_switches_is_beyond_a_record(oracle, case):
    """the ELAPSED_ONLY exemption has no twin here: every Tick form runs under CheckQuorum, so a record reads what it moved (a lease
    that ended, a check that cleared the word), and every other kind either changes nothing by its contract or is told apart"""
    sch = I.schedule(case)
    exempt = [mv.kind for mv in sch.moves if mv.kind not in I.no_change(case) and not len(I.discriminates(mv))]
    assert exempt == []
    ticks = [mv for mv in sch.moves if mv.kind in I.TICKS]
    assert len(ticks) >= 3 and all(len(I.discriminates(mv)) >= 1 for mv in ticks)
    if I.CASES[case]["lt"]:
        assert sum(mv.want["aborted"] for mv in ticks) >= 1, "a Tick whose passed check aborts a transfer"


@pytest.mark.parametrize("case", SCHEDULES)
def test_the_batches_reach_every_result_kind(oracle, case):
    sch = I.schedule(case)
    c = I.CASES[case]
    types, flags, down_by_check = set(), 0, 0
    for mv in sch.moves:
        for m, w in zip(mv.batches, mv.wants):
            types |= set(int(t) for t in np.unique(w["type"]))
            flags |= int(np.bitwise_or.reduce(w["flags"]))
            down_by_check += int(((m["type"] == S.MSG_CHECK_QUORUM) & ((w["flags"] & R.FlagSteppedDown) != 0)).sum())
    assert set(range(S.OUT_VOTE_RESP, S.OUT_FORWARD + 1)) <= types, sorted(types)
    if c["cq"]:
        assert down_by_check >= 3, "RAFTQ_OUTF_STEPPED_DOWN by a check"
    else:
        assert down_by_check == 0
    if case in EXTENDED:  # what the switches add, wherever they allow it
        assert {S.OUT_READ_INDEX, S.OUT_READ_STATE} <= types and flags & S.OUTF_READ_READY, (sorted(types), hex(flags))
        assert (S.OUT_TRANSFER in types) == c["lt"] and bool(flags & S.OUTF_TIMEOUT_NOW) == c["lt"], (sorted(types), hex(flags))
        assert ({S.OUT_PRE_CAMPAIGN, S.OUT_PRE_VOTE_RESP, S.OUT_TERM_RESP} <= types) == c["pv"] and (S.OUT_PRE_CAMPAIGN in types) == c["pv"], sorted(types)


@pytest.mark.parametrize("case", EXTENDED)
def test_every_rule_of_the_three_switches_is_read_by_some_batch(oracle, case):
    """ref_read_index's, ref_lead_transfer's and ref_pre_vote's rules, each left out in turn while the schedule's batches are stepped
    again: a record or a word of state changes in at least one batch (python -m tests.interleave_digest --report counts them all)"""
    sch = I.schedule(case)
    rules = I.case_rules(case)
    c = I.CASES[case]
    assert len(rules) == (2 if c["ri"] == I.LEASE else 5) + (7 if c["lt"] else 0) + (5 if c["pv"] else 0)
    for which, rule in rules:
        assert I.batches_changed_without(sch, which, rule, stop_at=1) >= 1, (case, which, rule, "no batch of the schedule reads the rule")


@pytest.mark.parametrize("case", [k for k in EXTENDED if I.CASES[k]["pv"]])
def test_the_window_without_pre_vote_is_a_step_without_it(oracle, case):
    """inside pv_off the reference is ref_pre_vote's classes with all five rules left out.  On every group that is not in role 3
    that is, record for record and word for word, the classes that never had the arms"""
    from tests import ref_read_index as RI

    sch = I.schedule(case)
    mv = next(mv for mv in sch.moves if mv.kind == "pv_off")
    m = mv.batches[0]
    ref = mv.after.copy()
    keep = ((m["_pad"][:, 1] & I.V.MSGF_SKIP) != 0) | (m["group"] >= I.G) | (ref.s.role[np.minimum(m["group"], I.G - 1).astype(np.int64)] != 3)
    assert 0 < int((~keep).sum()) and int(keep.sum()) >= 300
    part = np.ascontiguousarray(m[keep])
    got = RI.step_batch(ref.s, ref.voters, ref.extra, part, mode=ref.ri, pre_vote=False, lead_transfer=ref.lt, election_tick=I.ET)
    assert got.tobytes() == np.ascontiguousarray(mv.wants[0][keep]).tobytes()
    if len(mv.batches) == 2:  # (a pipelined pair: after_step stands behind the second batch)
        return
    rest = np.setdiff1d(np.arange(I.G), m["group"][~keep].astype(np.int64))
    for k, _ in I.pyoracle.NodeState.FIELDS:
        assert np.array_equal(getattr(ref.s, k)[rest], getattr(mv.after_step.s, k)[rest]), k
    assert np.array_equal(ref.active[rest], mv.after_step.active[rest]) and np.array_equal(ref.transferee[rest], mv.after_step.transferee[rest])
    assert np.array_equal(ref.seq[rest], mv.after_step.seq[rest]) and np.array_equal(ref.acked[:, rest], mv.after_step.acked[:, rest])


@pytest.mark.parametrize("case", EXTENDED)
def test_the_new_moves_hold_what_the_issue_says(oracle, case):
    sch = I.schedule(case)
    c = I.CASES[case]
    standing = 0
    for mv in sch.moves:
        a, b = mv.before, mv.after
        if mv.kind == "activity":  # the transferees stand behind raftq_load_activity, some of them in groups whose word it rewrote
            assert np.array_equal(a.transferee, b.transferee)
            standing = max(standing, int((b.transferee[mv.changed] != 0).sum()))
        elif mv.kind == "lt_toggle":
            assert not b.transferee.any() and a.transferee.any() and np.array_equal(a.active, b.active) and np.array_equal(a.le, b.le)
        elif mv.kind == "ri_toggle":
            assert not b.seq.any() and not b.acked.any() and b.ri == a.ri and mv.args["other"] == (I.LEASE if a.ri == I.SAFE else I.SAFE)
            assert np.array_equal(a.transferee, b.transferee) and np.array_equal(a.active, b.active)
        elif mv.kind == "reads":
            assert (b.acked <= b.seq[None, :]).all() and len(mv.changed) >= 100
        elif mv.kind == "transfer":
            assert (b.transferee <= c["n"]).all() and len(mv.changed) >= 60
        elif mv.kind == "roles":
            new3 = (b.s.role == 3) & (a.s.role != 3)
            assert (b.s.lead[new3] == 0).all() and not (new3.any() and not c["pv"])
            kept = (a.s.role == 2) & ((a.transferee != 0) | (a.seq != 0))
            assert (b.s.role[kept] == 2).all(), "only a leader holds a transferee or a read record"
        elif mv.kind == "closed":
            words = [w for _, w in mv.args["calls"]]
            assert len(words) >= 1 and words[-1] == ("pre vote" if c["pv"] else "lead transfer")
            assert ("lead transfer" in words) == c["lt"] and ("read index" in words) == (c["ri"] == I.SAFE)
    assert standing >= 4 if c["lt"] else standing == 0
    roles3 = sum(int((mv.args["role"] == 3).sum()) for mv in sch.moves if mv.kind == "roles")
    assert (roles3 >= 4) if c["pv"] else roles3 == 0, "raftq_load_roles loads role 3 where PreVote is on"
    if c["n"] == 9 and c["lt"]:
        assert any((mv.after.transferee == 9).any() for mv in sch.moves), "a transferee of 9 in the four bits"


@pytest.mark.parametrize("case", SCHEDULES)
def test_the_refused_batch_moves_nothing_in_the_reference(oracle, case):
    sch = I.schedule(case)
    n = I.CASES[case]["n"]
    refused = [mv for mv in sch.moves if mv.kind == "refused"]
    assert len(refused) >= 2
    for mv in refused:
        bad, at = mv.args["bad"], mv.args["at"]
        assert int(bad["from"][at]) >= n and I.refuses(bad, I.G, n)
        good = bad.copy()
        good["from"][at] = 0
        assert not I.refuses(good, I.G, n), "one record is what is wrong with it"
        ref = mv.before.copy()
        with pytest.raises(ValueError):
            ref.step(bad)
        assert ref.same(mv.before) and ref.same(mv.after)
