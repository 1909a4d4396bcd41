"""CPU: the schedules of tests/ref_interleave.py discriminate -- what keeps tests/test_interleave_gpu.py honest.  A move that the batch
behind it cannot tell from its absence would let a walk that skipped the mirror refresh pass; so for EVERY state-changing move of
every schedule the batch behind it, stepped by the reference on the state as it stood BEFORE the move, must give other records in at
least one group the move changed.  Nothing in here touches the device."""
import numpy as np
import pytest

from raftsql_amd import step as S
from tests import ref_interleave as I
from tests import ref_raft_py as R

SCHEDULES = sorted(set(c["schedule"] for c in I.CASES.values()))


def test_the_cases_are_the_issues():
    assert {k: (c["n"], c["me"], c["masks"], c["cq"], c["walk"]) for k, c in I.CASES.items()} == {
        "n3": (3, 1, False, False, "lists"), "n9": (9, 8, False, False, "lists"), "n5-masked": (5, 4, True, False, "lists"),
        "n3-cq": (3, 1, False, True, "lists"), "n5-masked-cq": (5, 4, True, True, "lists"), "n5-masked-cq-sort": (5, 4, True, True, "sort")}
    assert I.CASES["n5-masked-cq-sort"]["schedule"] == I.CASES["n5-masked-cq"]["schedule"], "the sorted walk runs the same schedule"
    assert I.G == 1027 and (I.ET, I.HB, I.SEED) == (10, 1, 0x5EED)
    assert I.schedule("n5-masked-cq-sort") is I.schedule("n5-masked-cq"), "built once"


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
    pairs = [mv for mv in sch.moves if len(mv.batches) == 2]
    assert len(pairs) >= 2
    for mv in pairs:  # a run longer than the list walk takes, in one of the two
        assert max(np.bincount(m["group"][m["group"] < I.G].astype(np.int64)).max() for m in mv.batches) >= I.K_RUN > 32
    for mv in sch.moves:
        assert all(len(m) <= 1024 and len(m) == len(w) for m, w in zip(mv.batches, mv.wants))
        listed = mv.changed[: I.MAX_CHANGED]
        assert np.isin(listed, mv.batches[0]["group"].astype(np.int64)).all(), (mv.kind, "a changed group without a record")
        assert not I.refuses(mv.batches[0], I.G, I.CASES[case]["n"]), "every input is in range"


@pytest.mark.parametrize("case", SCHEDULES)
def test_every_state_changing_move_is_seen_by_the_batch_behind_it(oracle, case):
    """100 % of the moves that change state.  Exempt: the three kinds that change nothing (clone, narrow_rebuild, the refused call)
    -- and a Tick that neither runs under CheckQuorum nor campaigns on the device: it moves `elapsed` alone, which Step without
    CheckQuorum neither reads nor reports, so no record CAN differ; for those it is asserted that elapsed is all that moved."""
    sch = I.schedule(case)
    seen = total = 0
    for k, mv in enumerate(sch.moves):
        if mv.kind in I.NO_CHANGE:
            assert mv.before.same(mv.after), (k, mv.kind)
            continue
        assert not mv.before.same(mv.after), (k, mv.kind, "the move changed nothing")
        if mv.kind in I.ELAPSED_ONLY:
            assert not I.CASES[case]["cq"]
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


@pytest.mark.parametrize("case", SCHEDULES)
def test_the_batches_reach_every_result_kind(oracle, case):
    sch = I.schedule(case)
    types, down_by_check = set(), 0
    for mv in sch.moves:
        for m, w in zip(mv.batches, mv.wants):
            types |= set(int(t) for t in np.unique(w["type"]))
            down_by_check += int(((m["type"] == S.MSG_CHECK_QUORUM) & ((w["flags"] & R.FlagSteppedDown) != 0)).sum())
    assert set(range(S.OUT_VOTE_RESP, S.OUT_FORWARD + 1)) <= types, sorted(types)
    if I.CASES[case]["cq"]:
        assert down_by_check >= 3, "RAFTQ_OUTF_STEPPED_DOWN by a check"
    else:
        assert down_by_check == 0


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
