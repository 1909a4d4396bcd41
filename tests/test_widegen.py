"""CPU: the inputs of tests/test_step_wide_gpu.py can catch a narrow kernel.  Everything here runs on the oracle alone, with the
seeds the GPU tests use (tests/_widegen.step_run): the oracle's results cover every result type and flag in every band, the tails
straddle the boundary, a 32-bit reading of the same inputs changes what Step decides, the compares Step makes have operands on
both sides of 2^63 -- and the hand tables of tests/_stepgen.py, lifted to each band, hold the oracle to answers that do not come
from it."""
import numpy as np
import pytest

from tests import _stepgen
from tests import _widegen as WG
from tests import ref_step_voters as V

U = np.uint64
OUT_NAMES = {1: "VOTE_RESP", 2: "HEARTBEAT_RESP", 3: "CAMPAIGN", 4: "BECAME_LEADER", 5: "PROGRESS", 6: "BCAST_HEARTBEAT", 7: "APPEND",
             8: "APPENDED", 9: "DEFERRED"}
OUT_SKIPPED, OUT_HELD = 10, 11
FLAGS = {1: "HARDSTATE", 2: "COMMITTED", 4: "UPDATED", 8: "STEPPED_DOWN"}
FLOOR = 20


# ---- the generators themselves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_lift_keeps_zeros_and_invariants(oracle, band):
    rng = np.random.default_rng(1)
    s = _stepgen.random_state(rng, 3000, 5, 2)
    w = WG.lift(s, band, rng)
    for k in ("last_index", "last_term", "committed", "first_idx"):
        assert np.array_equal(getattr(w, k) == 0, getattr(s, k) == 0), k
    assert np.array_equal(w.match == 0, s.match == 0)
    for k in ("role", "elapsed", "vote", "lead"):
        assert np.array_equal(getattr(w, k), getattr(s, k)), k
    assert np.array_equal(w.votes, s.votes)
    live = s.last_index != 0
    lo, hi = (WG.TOP_LO, WG.TOP_HI - 1) if band == "top" else (WG.BANDS[band] - 6, WG.BANDS[band] + 6)
    assert int(w.last_index[live].min()) >= lo and int(w.last_index[live].max()) <= hi
    if band != "top":
        assert int(w.term.min()) == WG.BANDS[band] - 3 and int(w.term.max()) == WG.BANDS[band] + 3
        # the distances inside a group are the small state's
        assert np.array_equal((w.last_index - w.committed)[s.committed != 0], (s.last_index - s.committed)[s.committed != 0])
        led = (s.role == 2) & (s.match != 0).all(axis=0)
        assert led.any() and np.array_equal((w.last_index[None, :] - w.match)[:, led], (s.last_index[None, :] - s.match)[:, led])
    # a led group with a Match of 0 next to lifted ones: what no 32-bit mirror stands for
    assert (((w.match == 0).any(axis=0)) & ((w.match >= U(2**32)).any(axis=0))).sum() > 100


def test_saturating_arithmetic():
    rng = np.random.default_rng(2)
    v = np.array([0, 1, 2, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1], U)
    assert [int(x) for x in WG.sat_sub(v, 2)] == [0, 0, 0, 2**63 - 3, 2**63 - 2, 2**64 - 4, 2**64 - 3]
    assert [int(x) for x in WG.sat_add(v, 2)] == [2, 3, 4, 2**63 + 1, 2**63 + 2, 2**64 - 1, 2**64 - 1]
    for _ in range(50):
        a = WG.around(rng, v, -3, 4, len(v))
        d = a.astype(object) - v.astype(object)
        assert all(-3 <= int(x) <= 3 for x in d) and a.dtype == U
    with pytest.raises(AssertionError):
        WG.guard(np.array([WG.LIMIT], U))
    WG.guard(np.array([WG.LIMIT - 1], U))


@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_frames_and_proposals_stay_in_the_band(oracle, band):
    from oracle import pywire as W

    rng = np.random.default_rng(3)
    st = WG.lift(_stepgen.random_state(rng, 500, 3, 1), band, rng)
    s, off = WG.wide_node_frames(rng, 2000, st, 1)
    wm, we, _ = W.wire_decode(s, off)
    ok = (wm["flags"] & W.F_MALFORMED) == 0
    lo = (WG.TOP_LO if band == "top" else WG.BANDS[band]) - 16
    live = ok & (wm["group"] < 500) & (st.last_index[np.minimum(wm["group"], 499).astype(np.int64)] != 0)
    assert live.sum() > 1000 and int(wm["index"][live].min()) >= lo and int(wm["term"][live].min()) >= lo
    assert int(we["index"].max()) < WG.LIMIT
    d, props, pe, pool, hm, he = WG.wide_propose_setup(rng, band, 4096, 3, 0, 200, 50)
    assert int(props["n_ents"][0]) == WG.PROP_MAX_ENTS == int(props["n_ents"].max())
    g = props["group"].astype(np.int64)
    if band != "top":
        B = WG.BANDS[band]
        assert (d["last"] < U(B)).all() and (d["last"] >= U(B - 3)).all()
        cross = d["last"][g] + props["n_ents"].astype(U) >= U(B)  # the record's entries cross B inside one MsgApp
        assert cross[0] and cross.mean() > 0.5, cross.mean()
        assert (d["term"] < U(B)).any() and (d["term"] >= U(B)).any()
    assert (d["last_term"] <= d["term"]).all() and (d["committed"] <= d["last"]).all()


# ---- coverage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold_skip", [False, True], ids=["plain", "hold-skip"])
@pytest.mark.parametrize("N,me", WG.STEP_SHAPES)
@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_the_run_covers_every_result_and_straddles_the_boundary(oracle, band, N, me, hold_skip):
    """per band and shape, over the ten batches of test_step_wide (plain) and of the pipelined forms (hold-skip): at least 20 of
    every result type and of every RAFTQ_OUTF_* flag, HELD and SKIPPED where the run flags records; at the start at least 30 % of
    the tails below B and 30 % at or above it.  Measured: 44.6 % to 47.4 % of the tails start below B (6 of the 13 places)."""
    start, batches, _ = WG.step_run(band, N, me, hold_skip)
    outs = np.concatenate([want for _, want, _, _ in batches])
    types = np.bincount(outs["type"], minlength=12)
    for t, name in OUT_NAMES.items():
        assert types[t] >= FLOOR, (name, int(types[t]))
    if hold_skip:
        assert types[OUT_HELD] >= FLOOR and types[OUT_SKIPPED] >= FLOOR, types
    for bit, name in FLAGS.items():
        assert int(((outs["flags"] & bit) != 0).sum()) >= FLOOR, name
    assert max(np.unique(batches[2][0]["group"], return_counts=True)[1]) > 32  # the hot batches stall the list walk
    if band != "top":
        tails = start.last_index[start.last_index != 0]
        below = float(WG.below_boundary(band, tails).mean())
        print("%s N=%d: %.1f %% of the tails start below B" % (band, N, 100 * below))
        assert 0.30 <= below <= 0.70, below


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------
def _mod32(a):
    return a & U(0xFFFFFFFF)


@pytest.mark.parametrize("N,me", WG.STEP_SHAPES)
def test_a_32_bit_reading_of_the_b32_run_decides_differently(oracle, N, me):
    """the oracle over the same start state and batches with every 64-bit field reduced mod 2^32: at least 5 % of the records must
    differ in (type, reject, flags, role).  Measured with this generator: 27.9 % (N = 3), 25.0 % (N = 5), 26.2 % (N = 9) of 90,000
    records; the share grows with the run, as the 32-bit state drifts away from the wide one batch after batch."""
    start, batches, _ = WG.step_run("b32", N, me)
    s = V.copy_state(start)
    for k in ("term", "last_index", "last_term", "committed", "first_idx"):
        getattr(s, k)[:] = _mod32(getattr(s, k))
    s.match[:] = _mod32(s.match)
    differ = total = 0
    for m, want, _, _ in batches:
        m = m.copy()
        for k in ("term", "log_term", "index", "commit", "reject_hint"):
            m[k] = _mod32(m[k])
        got = s.step_batch(m)
        differ += int(np.any([got[k] != want[k] for k in ("type", "reject", "flags", "role")], axis=0).sum())
        total += len(m)
    print("b32 N=%d: a 32-bit reading differs in %.1f %% of %d records" % (N, 100 * differ / total, total))
    assert differ >= 0.05 * total, (differ, total)


@pytest.mark.parametrize("N,me", WG.STEP_SHAPES)
def test_the_b63_run_puts_compare_operands_on_both_sides_of_2_63(oracle, N, me):
    """no oracle mutation stands for a signed compare, so this counts from the inputs: the records for which a compare Step makes
    on that kind of message -- m.term : term, m.index : last_index, m.index : match[from], m.commit : committed, m.log_term :
    last_term, each against the group's state before the batch -- has its operands on opposite sides of 2^63.  At least 5 %.
    Measured: 22.4 % (N = 3), 24.0 % (N = 5), 25.0 % (N = 9) of 90,000 records; the share falls as the run goes on, since tails
    and terms only grow away from the boundary."""
    _, batches, _ = WG.step_run("b63", N, me)
    hit = total = 0
    for m, _, _, pre in batches:
        g, t = m["group"].astype(np.int64), m["type"]
        hi = lambda a: np.asarray(a) >= U(2**63)  # noqa: E731
        opp = lambda a, b: hi(a) != hi(b)  # noqa: E731
        remote = (t != 0) & (t != 1)
        c = remote & opp(m["term"], pre.term[g])
        c |= np.isin(t, [3, 5]) & opp(m["index"], pre.last_index[g])
        c |= (t == 4) & opp(m["index"], pre.match[m["from"].astype(np.int64), g])
        c |= np.isin(t, [3, 8]) & opp(m["commit"], pre.committed[g])
        c |= np.isin(t, [3, 5]) & opp(m["log_term"], pre.last_term[g])
        hit += int(c.sum())
        total += len(m)
    print("b63 N=%d: %.1f %% of %d records compare across 2^63" % (N, 100 * hit / total, total))
    assert hit >= 0.05 * total, (hit, total)


@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_the_oracle_is_the_python_restatement_in_every_band(oracle, band):
    """the reference of the GPU tests against a second one that cannot narrow: tests/ref_raft_py.py computes in Python integers.
    With every mask full, tests/ref_step_voters.step_batch over the first three batches of the run (the third a hot one) gives the
    C oracle's records byte for byte and its state word for word -- a 32-bit or signed temporary in the oracle's Step shows here"""
    N, me = 5, 4
    start, batches, _ = WG.step_run(band, N, me, True)
    s = V.copy_state(start)
    full = V.full_masks(N, s.G)
    for it in range(3):
        m, want, _, _ = batches[it]
        got = V.step_batch(s, full, m)
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))
        assert len(bad) == 0, (band, it, len(bad), m[bad[0]], got[bad[0]], want[bad[0]])
    after = batches[3][3]  # the oracle's state before the fourth batch
    for k, _ in s.FIELDS:
        assert np.array_equal(getattr(s, k), getattr(after, k)), k
    assert np.array_equal(s.match, after.match) and np.array_equal(s.votes, after.votes)


# ---- the hand tables, lifted: known answers that do not come from the oracle ---------------------------------------------------------
@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_tail_append_table_lifted(oracle, band):
    s, m, want = WG.lifted_tail_append_table(band)
    out = s.step_batch(m)
    _stepgen.check_tail_append_table(out, s, want)
    tb, ib = WG.table_bases(band)
    assert int(s.term[10]) == int(tb) + 6 and int(out["term"][10]) == int(tb) + 6  # the newer term was adopted
    assert int(s.term[0]) == int(tb) + 5 and int(out["type"][9]) == 0 and int(s.term[9]) == int(tb) + 5


@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_barrier_table_lifted(oracle, band):
    s, m, want, after = WG.lifted_barrier_table(band)
    out = s.step_batch(m)
    assert [int(t) for t in out["type"]] == want
    WG.check_state_after(s, after)
    tb, ib = WG.table_bases(band)
    assert int(out["index"][0]) == int(ib) + 11 and int(out["commit"][1]) == int(ib) + 11 and int(out["commit"][6]) == int(ib) + 9


def check_alias_table(out, s, want, after, match_row):
    assert [int(t) for t in out["type"]][:2] == want[:2]
    WG.check_state_after(s, after)
    assert [int(x) for x in s.match[:, 2]] == match_row


@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_alias_table(oracle, band):
    s, m, want, after, match_row = WG.alias_table(band)
    check_alias_table(s.step_batch(m), s, want, after, match_row)


@pytest.mark.parametrize("band", WG.BAND_NAMES)
def test_hold_skip_table_lifted(oracle, band):
    s, m, want, after = WG.lifted_hold_skip_table(band)
    out = s.step_batch(m)
    assert [int(t) for t in out["type"]] == want
    WG.check_state_after(s, after)
    tb, ib = WG.table_bases(band)
    assert int(out["commit"][0]) == int(ib) + 8 and int(out["commit"][5]) == int(ib) + 9
