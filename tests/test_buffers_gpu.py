"""GPU: every buffer a handle grows is regrown under traffic, call kind by call kind (raftsql_amd/csrc/raftq_buffers.hpp owns
them; tests/test_wire_gpu.py test_buffers_and_control_block_regrow_between_calls_of_different_kinds does this for the codecs).
One handle of 65,536 groups x 5 peers per test; for each call kind small, large, small, where small is 8-16 records and large
is the smallest batch past the first capacity the buffer behind that call gets -- asserted from the record sizes, not read off
the handle.  Every result is the oracle's, compared as the suites of the call kinds compare it."""
import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd._lib import SWEEP_COMMIT, SWEEP_VOTES
from tests import _stepgen
from tests.test_parity_gpu import _state
from tests.test_wire_gpu import _same, _step_traffic

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("stage_mode")]  # every test, both staging forms

G, N = 65536, 5
MiB = 1 << 20


def _turn(e, oracle, rng, ref, packed, n_groups, nd, nv, cap):
    """one batching turn of nd match + nv vote deltas, `n_groups` of the groups acked by a quorum; ref = [match, commit, votes]"""
    assert 3 * n_groups <= nd
    ref_match, ref_commit, ref_votes = ref
    quorum_g = np.repeat(rng.choice(G, n_groups, replace=False), 3)
    dg = np.concatenate([quorum_g, rng.integers(0, G, nd - len(quorum_g))]).astype(np.uint64)
    dp = np.concatenate([np.tile(np.arange(1, 4), n_groups), rng.integers(0, N, nd - len(quorum_g))]).astype(np.uint32)
    dm = (ref_commit[dg.astype(np.int64)] + np.uint64(10)).astype(np.uint64)
    dm[len(quorum_g):] += rng.integers(0, 3000, nd - len(quorum_g)).astype(np.uint64)
    vd = e.pack_vote_deltas(rng.integers(0, G, nv).astype(np.uint64), rng.integers(1, N, nv).astype(np.uint32), rng.integers(1, 3, nv).astype(np.uint8))
    flags = SWEEP_COMMIT | SWEEP_VOTES
    if packed:
        adv, total, cnt = e.cycle_packed(flags, e.pack_deltas16(dg, dp, dm), vd, cap=cap)
    else:
        adv, total, cnt = e.cycle(flags, e.pack_deltas(dg, dp, dm), vd, cap=cap)
    ref_match = oracle.apply_deltas(ref_match, dg, dp, dm)
    ref_votes = oracle.apply_vote_deltas(ref_votes, vd["group"].copy(), vd["peer"].copy(), vd["vote"].copy())
    new_commit, n_ch = oracle.commit_advance(ref_match, ref_commit)
    oc, w, l = oracle.vote_tally(ref_votes)
    idx = np.nonzero(new_commit != ref_commit)[0]
    assert total == n_ch == len(idx) >= n_groups and (cnt.n_changed, cnt.n_won, cnt.n_lost) == (n_ch, w, l)
    take = min(cap, n_ch)
    assert len(adv) == take and np.array_equal(adv["group"].astype(np.uint64), idx[:take].astype(np.uint64))
    assert np.array_equal(adv["new_commit"], new_commit[idx[:take]])
    old = adv["new_commit"] - adv["advanced_by"].astype(np.uint64) if packed else adv["old_commit"]
    assert np.array_equal(old, ref_commit[idx[:take]])
    assert np.array_equal(e.read_committed(), new_commit) and np.array_equal(e.read_outcome(), oc)
    assert np.array_equal(e.read_votes(), ref_votes) and np.array_equal(e.read_match(), ref_match)
    ref[:] = [ref_match, new_commit, ref_votes]
    return n_ch


@pytest.mark.parametrize("kind", ["cycle", "cycle_packed", "contiguous_list"])
def test_the_turns_buffers_regrow(gpu_engine_cls, oracle, kind):
    """raftq_cycle / raftq_cycle_packed: the ack buffer (first capacity 1 MiB) under 50,000 match + 50,000 vote deltas, which
    leaves it at 2 MiB; its device copy is sized from the ack buffer's capacity (first capacity 2 MiB), so a turn of 70,000 +
    70,000 follows, which takes both past 2 MiB.  The contiguous advance list (first capacity 4,096 entries) under a list
    longer than that after a shorter one."""
    rng = np.random.default_rng(1100 + len(kind))
    st = _state(G, N, 1100, adversarial=False)
    votes = np.zeros((N, G), dtype=np.uint8)
    votes[0] = 1
    packed = kind == "cycle_packed"
    settled, _ = oracle.commit_advance(st.match, st.committed)  # nothing is pending: a turn advances what its deltas advance
    with gpu_engine_cls(G, N) as e:
        e.load_match(st.match, settled)
        e.load_votes(votes)
        ref = [st.match.copy(), settled, votes.copy()]
        if kind == "contiguous_list":
            assert _turn(e, oracle, rng, ref, False, 4, 12, 8, cap=16) < 4096
            assert _turn(e, oracle, rng, ref, False, 5000, 15000, 8, cap=G) > 4096
            _turn(e, oracle, rng, ref, False, 4, 12, 8, cap=16)
            return
        rec = (e._DELTA16_DT if packed else e._DELTA_DT).itemsize
        assert rec == (16 if packed else 24) and 16 * (rec + e._VDELTA_DT.itemsize) < MiB < 50000 * (rec + e._VDELTA_DT.itemsize)
        _turn(e, oracle, rng, ref, packed, 4, 12, 16, cap=G)
        _turn(e, oracle, rng, ref, packed, 5000, 50000, 50000, cap=G)
        _turn(e, oracle, rng, ref, packed, 4, 12, 16, cap=G)
        assert 50000 * (rec + e._VDELTA_DT.itemsize) + 4096 <= 2 * MiB < 70000 * (rec + e._VDELTA_DT.itemsize)
        _turn(e, oracle, rng, ref, packed, 5000, 70000, 70000, cap=G)
        _turn(e, oracle, rng, ref, packed, 4, 12, 16, cap=G)


def test_the_tick_lists_regrow(gpu_engine_cls, oracle):
    """raftq_tick_collect_lists: the in-place lists (first capacity 64 KiB) under caps of 16, then of G, then of 16 again"""
    rng = np.random.default_rng(1200)
    role = (np.arange(G) % 3).astype(np.uint8)
    el = rng.integers(0, 21, G).astype(np.uint32)
    assert (16 + 16) * 4 + G // 8 + 512 < (1 << 16) < (G + G) * 4  # 4-byte ids, the bitmap's room behind them
    with gpu_engine_cls(G, N) as e:
        e.set_timers(10, 1, 0xBEEF)
        e.load_roles(role, el)
        ref_el = el.copy()
        for t, cap in enumerate((16, G, 16)):
            hups, nh, beats, nb = e.tick_collect_lists(cap, cap)
            ref_el, ref_act, rh, rb = oracle.tick(role, ref_el, 10, 1, 0xBEEF, t)
            want_h, want_b = np.nonzero(ref_act == 1)[0].astype(np.uint32), np.nonzero(ref_act == 2)[0].astype(np.uint32)
            assert (nh, nb) == (rh, rb) and rh > 16 and rb > 16 and hups.dtype == np.uint32
            assert len(hups) == min(cap, rh) and np.array_equal(hups, want_h[: len(hups)])
            assert len(beats) == min(cap, rb) and np.array_equal(beats, want_b[: len(beats)])
            act, got_el, _ = e.read_tick()
            assert np.array_equal(act, ref_act) and np.array_equal(got_el, ref_el)


def _tails(rng, s, g):
    li = s.last_index[g] + rng.integers(0, 3, len(g)).astype(np.uint64)
    lt = np.maximum(s.last_term[g], s.term[g] * (s.role[g] == 2))
    ct = np.where(s.role[g] == 2, 0, np.minimum(li, s.committed[g] + rng.integers(0, 3, len(g)).astype(np.uint64)))
    return g.astype(np.uint64), li, lt, ct


@pytest.mark.usefixtures("gpu_engine_cls", "oracle")  # a visible GPU, the oracle built
@pytest.mark.parametrize("nowait", [False, True], ids=["apply_log_deltas", "apply_log_deltas_nowait"])
def test_the_log_deltas_staging_regrows(nowait):
    """raftq_apply_log_deltas (the staging, first capacity 1 MiB) and _nowait (two areas taken in turn, 64 KiB): every group once"""
    from raftsql_amd.step import LOG_DELTA_DT, NodeEngine

    rng = np.random.default_rng(1300)
    s = _stepgen.random_state(rng, G, N, 1)
    assert 16 * LOG_DELTA_DT.itemsize < (1 << 16) and G * LOG_DELTA_DT.itemsize > MiB
    with NodeEngine(G, N, 1) as e:
        _stepgen.load_engine(e, s)
        # (the no-wait form takes its two areas in turn: both hold their first capacity before the large batch)
        for n in (12, 12, G, 12) if nowait else (12, G, 12):
            d = _tails(rng, s, rng.permutation(G)[:n])
            want = s.apply_log_deltas(*d)
            if nowait:
                e.apply_log_deltas_nowait(*d)
            else:
                assert np.array_equal(e.apply_log_deltas(*d), want)
            _stepgen.assert_same_state(e, s)


@pytest.mark.usefixtures("gpu_engine_cls", "oracle")  # a visible GPU, the oracle built
@pytest.mark.parametrize("kind", ["step_batch", "step_stage", "step_submit_wire"])
def test_the_step_slots_regrow(kind):
    """Step's slots (staging in, scratch, results out, the decoded records' copies: first capacities of 1 and 2 MiB) under 24,000
    messages -- from caller arrays, staged in place, as frames with entries.  Batches take the three slots in turn, so three small
    ones go before the large one and three behind it: one slot sees small, large, small, the other two stay at their first capacity."""
    from raftsql_amd import step as S
    from raftsql_amd.wire import WireEngine

    rng = np.random.default_rng(1400 + len(kind))
    s = _stepgen.random_state(rng, G, N, 0)
    big = 24000
    assert 16 * S.MSG_DT.itemsize < MiB < big * S.MSG_DT.itemsize and big * S.OUT_DT.itemsize > MiB
    with WireEngine(G, N, 0) as e:
        _stepgen.load_engine(e, s)
        for n in (12, 12, 12, big, 12, 12, 12):
            if kind == "step_submit_wire":
                m = _step_traffic(rng, n, G, N)
                app = np.nonzero(m["type"] == 3)[0]  # MsgApp frames carry entries; Step reads only the header
                m["n_ents"][app] = 2
                m["ent_first"][app] = np.arange(len(app)) * 2
                ents = np.zeros(2 * len(app), W.WIRE_ENT_DT)
                ents["term"], ents["index"], ents["data_len"] = 3, np.arange(len(ents)), 5
                ents["data_off"] = np.arange(len(ents)) * 5
                pool = rng.integers(0, 256, 5 * len(ents) + 1, dtype=np.uint8)
                stream, off = W.wire_encode(m, ents, pool)
                if n == big:
                    assert n * W.WIRE_MSG_DT.itemsize > MiB and len(ents) > 16  # the decoded records' copy alone
                rec = np.zeros(n, S.MSG_DT)
                for k in ("group", "term", "log_term", "index", "commit", "reject_hint", "from", "type", "reject"):
                    rec[k] = m[k]
                want = s.step_batch(rec)
                e.step_submit_wire(stream, off)
                got, touched = e.step_collect()
                wm, we, _ = W.wire_decode(stream, off)
                _same(e.step_wire_msgs(), wm, "decoded records of the batch")
                _same(e.step_wire_entries(), we, "decoded entries of the batch")
            else:
                rec = _stepgen.random_batch(rng, s, n)
                want = s.step_batch(rec)
                if kind == "step_stage":
                    staged = e.step_stage(n)
                    staged[:] = rec
                    got, touched = e.step_inplace(staged)
                else:
                    got, touched = e.step_batch(rec)
            assert touched == len(np.unique(rec["group"]))
            _same(got, want, "step results")
        _stepgen.assert_same_state(e, s)
