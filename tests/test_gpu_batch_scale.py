"""The replica batch beyond one workgroup's worth (csrc/kernels_batch.h, csrc/engine.hip batch_launch_sweep /
batch_reductions): the one-workgroup folds of k_finalize_batch and k_step_finalize_batch at 256, 257 and 513 records, the
partial layout rep * gridDim.x + blockIdx.x of k_psi_sum_batch with two chunks a replica, k_fold_batch at 64 / 65 / 128 / 129
rows and over the grids of the exact non-edge term and of the moments, and k_em_edges_batch at its cap of 1024 workgroups - on
the rings of tests/batch_scale_graph.py, against the oracle, the per-replica reductions and a single engine.
tests/test_batch_scale_cpu.py holds the CPU side: the sizes, the launch arithmetic, and that the oracle is finite, insensitive
to rounding and converges on every case run here.
Every case has three replicas with different seeds and different (cab, na) - identical replicas would hide an offset that
reads replica 0 - and first checks that the engine segments the graph as the model does. Tolerances are the project's: 1e-11
per sweep and between the engine's own reduction paths, 1e-9 against the oracle's reductions and on converged marginals, +- 2
sweeps for converge. Each case prints the largest differences it saw.
(sbmbp_batch_em_step takes no mask - only the learning loop passes one to the reductions -, so the masked reductions are
reached through learning(): two runs on the two-chunk ring in which replica 0, then replica 1, stops learning first.)"""
import numpy as np
import pytest

import batch_scale_graph as sc
import boundary_graph as bg
import coloured_model as cm
import coloured_step_graph as cg
from test_gpu_boundary import _Seen, _assert_plan

pytestmark = pytest.mark.gpu

SEEDS = list(bg.BATCH_SEEDS)


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _batch(S, g, t, params, seeds=SEEDS):
    b = S.ReplicaBatch(g, t["Q"], t["dc"], len(seeds))
    b.init_messages(0, None, t["tc"], list(seeds), conditional=True)
    for r, (cab, na) in enumerate(params):
        b.set_params(S.bp_blockmodel_state(cab, na), 1.0, r)
    return b


def _oracles(orc, t, params, seeds=SEEDS, msg_form=True):
    return [bg.oracle_of(orc, t, msg_form, seeds[r], cab, na)[1] for r, (cab, na) in enumerate(params)]


def _different(b, R):
    """the replicas are different runs"""
    psis = [b.get_state(r, msg=False)[0] for r in range(R)]
    assert all(np.abs(psis[x] - psis[y]).max() > 1e-3 for x in range(R) for y in range(x)), "replicas coincide"


# ---------------------------------------------------------------------------------------------------------------------
# (a) sweeps at 256, 257 and 513 records a replica: k_finalize_batch's fold beyond its first trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc,segs", sc.SWEEP)
def test_sweeps_beyond_one_trip_of_the_record_fold(S, orc, Q, dc, segs):
    t = sc.segments_instance(Q, dc, segs)
    seen = _Seen("batch scale sweeps cap %d Q %d dc %d, %d records" % (t["cap"], Q, dc, segs))
    g = S.Graph.from_edges(t["pairs"], t["N"])
    assert g.E2 == t["E2"]
    params = bg.three_params(t)
    oracles = _oracles(orc, t, params)
    b, b2 = _batch(S, g, t, params), _batch(S, g, t, params)
    _assert_plan(b.stats(), t)
    assert b.stats().n_blocks == segs and t["launch"]["finalize_trips"] == {256: 1, 257: 2, 513: 3}[segs]
    # four sweeps, one call each: state and reported maximum of every replica against its own oracle after every sweep
    ref = []
    for k, damp in enumerate(bg.BATCH_DAMPS):
        d = b.sweep(1, damp)
        row = []
        for r, ob in enumerate(oracles):
            do = ob.sweep_sync(damp)
            psi, msg = b.get_state(r)
            opsi, omsg = ob.get_state()
            seen.per_sweep(np.abs(psi - opsi).max(), "marginals after sweep %d, replica %d" % (k, r))
            seen.per_sweep(np.abs(msg - omsg).max(), "messages after sweep %d, replica %d" % (k, r))
            seen.per_sweep(abs(d[r] - do), "difference of sweep %d, replica %d" % (k, r))
            row.append((opsi, omsg, do))
        ref.append(row)
    assert min(x[2] for x in ref[-1]) > 1e-6  # still moving
    _different(b, sc.R)
    # the same sweeps as two calls of two: the second sweep of a call reads the field the fold of the first left behind
    done = 0
    for n, damp in sc.CALLS:
        d = b2.sweep(n, damp)
        done += n
        for r in range(sc.R):
            psi, msg = b2.get_state(r)
            opsi, omsg, do = ref[done - 1][r]
            seen.per_sweep(np.abs(psi - opsi).max(), "marginals after %d queued sweeps, replica %d" % (done, r))
            seen.per_sweep(np.abs(msg - omsg).max(), "messages after %d queued sweeps, replica %d" % (done, r))
            seen.per_sweep(abs(d[r] - do), "difference of queued sweep %d, replica %d" % (done - 1, r))
    st = b2.stats()
    assert st.sweeps == sc.R * len(bg.BATCH_DAMPS) and st.edge_msg_updates == st.sweeps * g.E2 and st.psi_form_sweeps == 0
    b2.close()
    # every replica stops on its own, within two sweeps of its oracle
    niter, last = b.converge(1e-10, sc.CONVERGE_SWEEPS, 1.0)
    counts = []
    for r, ob in enumerate(oracles):
        no, lo = ob.converge_sync(1e-10, sc.CONVERGE_SWEEPS, 1.0)
        counts.append("%d / %d" % (niter[r], no))
        assert niter[r] >= 0 and no >= 0 and last[r] < 1e-10 and abs(int(niter[r]) - no) <= 2, (r, niter[r], no, last[r], lo)
        seen.against_oracle(b.get_state(r, msg=False)[0], ob.get_state()[0], "converged marginals, replica %d" % r)
    b.close()
    seen.report(", converge engine / oracle %s" % ", ".join(counts))


def test_one_replica_of_a_257_record_batch_equals_a_single_engine(S):
    """as tests/test_gpu_batch.py test_batch_equals_three_single_engines: the middle replica against a single engine in the
    message-gather form from the same seed and parameters, 1e-12 per sweep, the field included - one call per sweep, and on a
    second pair as two calls of two (only the second sweep of a call reads the field the fold left)"""
    Q, dc, segs, r = sc.SINGLE_ENGINE
    t = sc.segments_instance(Q, dc, segs)
    g = S.Graph.from_edges(t["pairs"], t["N"])
    params = bg.three_params(t)
    worst = 0.0
    for calls in ([(1, damp) for damp in bg.BATCH_DAMPS], sc.CALLS):
        b = _batch(S, g, t, params)
        bp = S.bp_conditional()
        bp.init_messages(S.blockmodel_t(g, Q, dc), 0, None, t["tc"], SEEDS[r])
        bp.expand_bp_params(S.bp_blockmodel_state(*params[r]))
        bp.set_gather_mode(1)
        assert b.stats().n_blocks == bp.stats().n_blocks == segs
        assert all(np.array_equal(x, y) for x, y in zip(b.get_state(r), bp.get_state()))
        for k, (n, damp) in enumerate(calls):
            d, ds = b.sweep(n, damp), bp.sweep(n, damp)
            (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
            dh = np.abs(b.h(r) - bp.h()).max() / max(1.0, np.abs(bp.h()).max())
            worst = max(worst, np.abs(p1 - p2).max(), np.abs(m1 - m2).max(), abs(d[r] - ds), dh)
            assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12 and abs(d[r] - ds) < 1e-12 and dh <= 1e-12, (calls, k)
        b.close()
    print("batch scale: replica %d of the %d-record batch against a single engine, largest difference %.3g" % (r, segs, worst))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the coloured order: a step of 256 and of 257 records a replica (k_step_finalize_batch)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc,records", sc.COLOURED)
def test_a_coloured_step_of_256_and_of_257_records_a_replica(S, orc, Q, dc, records):
    t = cg.instance(Q, dc, "ring%d" % records)
    seen = _Seen("batch scale coloured ring of %d records, Q %d dc %d" % (records, Q, dc))
    tb = t["tables"]
    assert tb["seg0"][1] - tb["seg0"][0] == records == tb["max_rec"]
    g = S.Graph.from_edges(t["pairs"], t["N"])
    seeds = [t["seed"], t["seed"] + 1]
    params = [(t["cab"], t["na"]), (t["cab"] * 1.1, t["na"])]
    b = _batch(S, g, t, params, seeds)
    _assert_plan(b.stats(), t)
    b.set_sweep_order("coloured", t["colour"], t["fraction"])
    assert b.sweep_order == (1, t["n_colours"], t["n_steps"])
    d1 = b.sweep(4, 1.0)  # four sweeps in one call
    gi = t["deg"].astype(float) if dc else np.ones(t["N"])
    for r, ob in enumerate(_oracles(orc, t, params, seeds, msg_form=False)):
        for _ in range(4):
            d2 = cm.fast_sweep(ob, t["step"], 1.0)
        assert d2 > 1e-6  # still moving
        psi, msg = b.get_state(r)
        opsi, omsg = ob.get_state()
        seen.per_sweep(np.abs(psi - opsi).max(), "marginals after four sweeps, replica %d" % r)
        seen.per_sweep(np.abs(msg - omsg).max(), "messages after four sweeps, replica %d" % r)
        seen.per_sweep(abs(d1[r] - d2), "difference of the fourth sweep, replica %d" % r)
        h, href = b.h(r), b.get_params(r)[0].T @ (gi[:, None] * psi).sum(0)  # the field moved step by step
        dh = np.abs(h - href).max() / max(1.0, np.abs(href).max())
        seen.field = max(getattr(seen, "field", 0.0), dh)
        assert dh <= 1e-12, (r, h, href)
    _different(b, 2)
    b.close()
    seen.report(", field %.3g" % seen.field)


# ---------------------------------------------------------------------------------------------------------------------
# (c) one EM step after three sweeps with a relaxed field: the field refresh, the frame pass and every fold
# ---------------------------------------------------------------------------------------------------------------------
def _em_step_case(S, orc, t, mode, forced, label):
    """as tests/test_gpu_batch_learn.py test_em_step_equals_the_per_replica_reductions: em_step() of one batch against the
    per-replica reductions of a second batch in the same states (1e-11), a second call (the same bits) and the oracle on the
    downloaded states (1e-9; the series of the same order where the engine sums a series)"""
    seen = _Seen(label)
    Q, N, dc = t["Q"], t["N"], t["dc"]
    g = S.Graph.from_edges(t["pairs"], N)
    assert g.E2 == t["E2"]
    params = bg.three_params(t)

    def make():
        b = _batch(S, g, t, params)
        b.set_nonedge_mode(mode, forced)
        b.set_schedule(field_mix=0.5)  # a relaxed field is stale after the sweeps: the field refresh runs first
        assert (b.sweep(3, 1.0) > 1e-6).all()  # not converged
        return b

    b, b2 = make(), make()
    _assert_plan(b.stats(), t)
    assert all(np.array_equal(x, y) for r in range(sc.R) for x, y in zip(b.get_state(r), b2.get_state(r)))
    _different(b, sc.R)
    na_b, nna_b, cab_b, f_b, parts_b = b.em_step()
    f_r, parts_r = b2.compute_free_energy(parts=True)
    for r in range(sc.R):
        for a, y in zip((na_b[r], nna_b[r], cab_b[r]), b2.em_expectations(r)):
            seen.own_paths(a, y, "em_step / per-replica EM expectations, replica %d" % r)
        seen.own_paths(parts_b[r], parts_r[r], "em_step / per-replica free energy parts, replica %d" % r)
        seen.own_paths(f_b[r], f_r[r], "em_step / per-replica free energy, replica %d" % r)
    again = b.em_step()
    assert all(np.array_equal(u, v) for u, v in zip((na_b, nna_b, cab_b, f_b, parts_b), again))  # fixed summation order
    # no all-pairs term under degree correction; without it the exact sum (forced, or chosen up to 32 768 rows) or the series
    exact = dc != 0 or mode == 1 or (mode == 0 and t["launch"]["exact_auto"])
    for r, ob in enumerate(_oracles(orc, t, params)):
        ob.set_state(*b.get_state(r))
        ob.compute_h()
        for a, y in zip((na_b[r], nna_b[r], cab_b[r]), ob.em_expect()):
            seen.against_oracle(a, y, "EM expectations, replica %d" % r)
        K = 0 if exact else sc.series_order_model(Q, N, params[r][0], forced)
        assert exact or K > 0
        fo, oparts = ob.free_energy(K)
        seen.against_oracle(parts_b[r], oparts, "free energy parts, replica %d" % r)
        seen.against_oracle(f_b[r], fo, "free energy, replica %d" % r)
    b.close()
    b2.close()
    seen.report()


@pytest.mark.parametrize("Q,dc,rows", sc.EM_FOLD)
def test_em_step_with_64_65_128_and_129_rows_in_the_frame_fold(S, orc, Q, dc, rows):
    t, mode, forced = sc.em_instance("fold", Q, dc, rows)
    assert t["launch"]["rows"] == rows and t["launch"]["frame_fold_trips"] == (rows + 63) // 64
    _em_step_case(S, orc, t, mode, forced, "batch scale em_step, %d rows in the frame fold, Q %d dc %d" % (rows, Q, dc))


@pytest.mark.parametrize("Q,dc,N", sc.EM_FIELD)
def test_em_step_with_one_and_two_chunks_in_the_field_refresh(S, orc, Q, dc, N):
    t, mode, forced = sc.em_instance("field", Q, dc, N)
    assert t["launch"]["nbf"] == {4096: 1, 4100: 2}[N]
    _em_step_case(S, orc, t, mode, forced, "batch scale em_step, %d chunk(s) in the field refresh, Q %d dc %d" % (t["launch"]["nbf"], Q, dc))


@pytest.mark.parametrize("Q,dc,N", sc.EM_EXACT)
def test_em_step_with_64_and_81_rows_in_the_exact_nonedge_fold(S, orc, Q, dc, N):
    t, mode, forced = sc.em_instance("exact", Q, dc, N)
    assert t["launch"]["g"] ** 2 == {2048: 64, 2052: 81}[N] and mode == 1
    _em_step_case(S, orc, t, mode, forced, "batch scale em_step, exact non-edge grid of %d, Q %d" % (t["launch"]["g"] ** 2, Q))


@pytest.mark.parametrize("Q,dc,N", sc.EM_SERIES)
def test_em_step_with_65_rows_in_the_moment_fold(S, orc, Q, dc, N):
    t, mode, forced = sc.em_instance("series", Q, dc, N)
    assert t["launch"]["nbm"] == 65 and not t["launch"]["exact_auto"] and t["launch"]["nbf"] == 9
    _em_step_case(S, orc, t, mode, forced, "batch scale em_step, automatic series with %d rows in the moment fold, Q %d" % (t["launch"]["nbm"], Q))


@pytest.mark.parametrize("Q,dc", sc.EM_DENSE)
def test_em_step_past_the_cap_of_the_edge_grid(S, orc, Q, dc):
    t, mode, forced = sc.em_instance("dense", Q, dc, None)
    L = t["launch"]
    assert L["edge_capped"] and L["nbe"] == 1024 and L["edge_blocks_twice"] == 32 and L["em_edges"]
    _em_step_case(S, orc, t, mode, forced, "batch scale em_step, %d directed edges, Q %d dc %d" % (t["E2"], Q, dc))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the mask of the reductions, through the learning loop (sbmbp_batch_em_step itself takes none)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", sc.LEARN_FIRST_OUT)
def test_learning_with_one_replica_masked_out_of_the_two_chunk_reductions(S, first):
    """multi-start EM on the ring of two field chunks a replica: the replica started at the larger cab ends its learning first
    (tests/test_batch_scale_cpu.py), so the reductions of the later rounds run with replica 0, or replica 1, outside the
    mask. As tests/test_gpu_batch_learn.py test_an_early_finisher_stays_frozen: every replica ends as the single engine from
    the same start does - which knows no mask -, and the early finisher keeps the state of its last round"""
    t, _, _ = sc.em_instance("field", *sc.LEARN_CASE)
    Q, dc, N = t["Q"], t["dc"], t["N"]
    assert t["launch"]["nbf"] == 2
    g = S.Graph.from_edges(t["pairs"], N)
    bm = S.blockmodel_t(g, Q, dc)
    scales = [sc.LEARN_EARLY if r == first else s for r, s in enumerate(sc.LEARN_SCALES)]
    b = S.ReplicaBatch(g, Q, dc, sc.R)
    b.init_messages(0, None, t["tc"], SEEDS, conditional=False)
    for r, s in enumerate(scales):
        b.set_params(S.bp_blockmodel_state(t["cab"] * s, t["na"]), 1.0, r)
    res, eta, cab, best = b.learning(*sc.LEARN_ARGS)
    steps = [x.em_steps for x in res]
    print("batch scale learning, replica %d first: EM steps %s, status %s, sweeps %s" % (first, steps, [x.status for x in res], [x.total_sweeps for x in res]))
    assert all(x.status == 1 for x in res) and all(steps[first] < s for r, s in enumerate(steps) if r != first), steps
    for r, s in enumerate(scales):
        bp = S.bp_basic()
        bp.init_messages(bm, 0, None, t["tc"], SEEDS[r])
        bp.set_gather_mode(1)
        sres = bp.learning(bm, S.bp_blockmodel_state(t["cab"] * s, t["na"]), *sc.LEARN_ARGS)
        assert (sres.em_steps, sres.status, sres.total_sweeps) == (res[r].em_steps, res[r].status, res[r].total_sweeps), r
        scab, sna = bp.get_params()
        bcab, bna, _ = b.get_params(r)
        assert list(sna) == list(bna) and np.abs(scab - bcab).max() <= 1e-9 * np.abs(scab).max(), r
        assert abs(res[r].free_energy - sres.free_energy) <= 1e-9 and abs(res[r].overlap - sres.overlap) <= 1e-9, r
        if r == first:  # frozen while the others went on for rounds
            (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
            assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12, r
    assert b.stats().sweeps == sum(x.total_sweeps for x in res)
    b.close()
