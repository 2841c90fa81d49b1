"""Label counts above 16 where the suite did not reach (instances: tests/wide_cases.py, proved on the CPU by
tests/test_wide_cpu.py):

A. the convergence machine of k_wfinalize (kernels_wide.h) - the rules of finalize_update written out a second time over the
   parameter block - and the 2-step probe inside k_wsweep, on runs of the hub graph on which the adaptive relaxation acts:
   the engine must end on the oracle's levels, within two sweeps of it, on a fixed point of the plain update, and its
   reductions on that state (whose field is stale after a relaxed run: k_wfinalize mode 2) must be the oracle's.
B. the two-stage fold (engine.hip fold_stage) of the wide path's [n_blk][Q + 1] sweep records (sums and a sticky maximum) and
   of its [n_blk][WR_NP + 1] reduction records, on ring graphs of 1024, 1025 and 1027 segments.

Each case prints what it saw; the tolerances are those of test_gpu_wide.py, test_gpu_boundary.py and the fuzz."""
import numpy as np
import pytest

import boundary_graph as bg
import wide_cases as wc
from test_gpu_boundary import _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


# ---------------------------------------------------------------------------------------------------------------------
# A. relaxing runs on the hub graph
# ---------------------------------------------------------------------------------------------------------------------
def _engine(S, case):
    cab, na, tc = case.arrays()
    g = S.load_edge_list(wc.HUB_PATH, wc.HUB_N)
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, case.Q, 0), 0, None, tc, case.seed)
    bp.expand_bp_params(S.bp_blockmodel_state(cab, na))
    return g, bp


def _same_start(bp, ob):
    (psi, msg), (opsi, omsg) = bp.get_state(), ob.get_state()
    assert np.array_equal(psi, opsi) and np.array_equal(msg, omsg)


def _fresh_oracle_on(orc, case, bp):
    """a fresh oracle (no relaxation, no history) on the engine's state, its field computed from that state"""
    og, oc = case.oracle(orc)
    oc.set_auto_relax(True)
    oc.set_field_mix(1.0)
    oc.set_state(*bp.get_state())
    oc.compute_h()
    return oc


def _fixed_point(orc, case, bp):
    """max |m' - m| of one plain undamped sweep from the engine's state: the bound of test_gpu_wide.py"""
    oc = _fresh_oracle_on(orc, case, bp)
    d = oc.sweep_sync(1.0)
    assert d < 1e-8, d
    return d


def _reductions(orc, case, bp):
    """free energy, EM expectations and (Q = 17) entropy of the engine on the state it reached against the oracle's on that
    state. The engine's field is the relaxed one of the last sweep: it must refresh it first (launch_field mode 2)."""
    oc = _fresh_oracle_on(orc, case, bp)
    f, fp = bp.compute_free_energy(parts=True)
    fo, fop = oc.free_energy(0)
    d_f = _rel(fp, fop)
    assert d_f <= 1e-9, (fp, fop)
    assert abs(f - fo) <= 1e-9 * max(1.0, abs(fo)), (f, fo)
    na1, nna1, cab1 = bp.em_expectations()
    na2, nna2, cab2 = oc.em_expect()
    d_em = (np.abs(na1 - na2).max(), np.abs(nna1 - nna2).max(), _rel(cab1, cab2))
    assert d_em[0] < 1e-9 and d_em[1] < 1e-8 and d_em[2] <= 1e-9, d_em
    d_e = None
    if case.Q == 17:  # the oracle's exact entropy takes 13 s at Q = 33 and 50 s at Q = 64 on a graph of this size
        e, ep = bp.compute_entropy(parts=True)
        eo, eop = oc.entropy(0)
        assert np.isfinite(ep).all() and np.isfinite(eop).all()
        d_e = _rel(ep, eop)
        assert d_e <= 1e-8, (ep, eop)  # (test_gpu_wide.py's bound for the entropy parts)
    # the refreshed field itself: sums of N non-negative terms in two orders, N 2^-53 apart at the most on either side (the
    # bound tests/test_gpu_boundary.py gives the field of the coloured order)
    h, ho = bp.h(), oc.h()
    assert np.abs(h - ho).max() <= 1e-12 * max(1.0, np.abs(ho).max()), (h, ho)
    return d_f, d_em, d_e


@pytest.mark.parametrize("case", wc.FIELD + wc.DAMPED + wc.PROBE, ids=lambda c: c.id)
def test_wide_relaxed_run_follows_the_oracle(S, orc, case):
    g, bp = _engine(S, case)
    og, ob = case.oracle(orc)
    _same_start(bp, ob)
    n1, l1 = bp.converge(wc.CRIT, case.tmax, 1.0)
    n2, l2 = ob.converge_sync(wc.CRIT, case.tmax, 1.0)
    fl, gl, mix, damp = bp.relaxation()
    print("wide relax %s: engine %d sweeps, levels (%d, %d), mix %g, damping %g, last %.3g; oracle %d sweeps, levels %s, last %.3g"
          % (case.id, n1, fl, gl, mix, damp, l1, n2, ob.ar_levels(), l2))
    assert ob.ar_levels() == case.levels and n2 == case.niter  # (tests/test_wide_cpu.py)
    assert (fl, gl) == ob.ar_levels(), (fl, gl, ob.ar_levels())
    assert (mix, damp) == wc.mix_damp(fl, gl), (mix, damp)
    assert n1 >= 0 and n2 >= 0 and abs(n1 - n2) <= 2, (n1, n2)
    assert l1 < wc.CRIT
    assert bp.stats().psi_form_sweeps == 0
    d_fix = _fixed_point(orc, case, bp)
    d_psi = np.abs(bp.get_state()[0] - ob.get_state()[0]).max()
    assert d_psi < 1e-7, d_psi
    d_f, d_em, d_e = _reductions(orc, case, bp)
    print("wide relax %s: plain sweep from the engine's state moves %.3g, marginals %.3g from the oracle's, free energy parts %.3g, "
          "EM (na, nna, cab) %.3g %.3g %.3g, entropy parts %s" % (case.id, d_fix, d_psi, d_f, d_em[0], d_em[1], d_em[2], "%.3g" % d_e if d_e is not None else "-"))


@pytest.mark.parametrize("case", wc.EXHAUSTED, ids=lambda c: c.id)
def test_wide_exhausted_ladder(S, orc, case):
    """every level of the generic ladder is used up and the run goes on as it is (hold = 1 << 30) to the sweep limit"""
    g, bp = _engine(S, case)
    og, ob = case.oracle(orc)
    _same_start(bp, ob)
    n1, l1 = bp.converge(wc.CRIT, case.tmax, 1.0)
    n2, l2 = ob.converge_sync(wc.CRIT, case.tmax, 1.0)
    fl, gl, mix, damp = bp.relaxation()
    print("wide relax %s: engine %d, levels (%d, %d), last %.3g; oracle %d, levels %s, last %.3g" % (case.id, n1, fl, gl, l1, n2, ob.ar_levels(), l2))
    assert n1 == -1 and n2 == -1
    assert (fl, gl) == ob.ar_levels() == case.levels
    assert (mix, damp) == wc.mix_damp(fl, gl)
    assert np.isfinite(l1)  # (a chaotic trajectory: the last differences need not agree)
    assert bp.stats().psi_form_sweeps == 0
    # here the run stops far from a fixed point with a field mixed at 0.1: the field the last sweep left is nowhere near the one
    # of the marginals, so the reductions are right only behind the exact refresh (k_wfinalize mode 2)
    d_f, d_em, _ = _reductions(orc, case, bp)
    print("wide relax %s: on the engine's unconverged state free energy parts %.3g, EM %.3g %.3g %.3g" % ((case.id, d_f) + d_em))


@pytest.mark.parametrize("case", wc.NO_AUTO, ids=lambda c: c.id)
def test_wide_plain_jacobi_when_the_machine_is_off(S, orc, case):
    g, bp = _engine(S, case)
    bp.set_auto_relax(False)
    og, ob = case.oracle(orc)
    _same_start(bp, ob)
    n1, l1 = bp.converge(wc.CRIT, case.tmax, 1.0)
    n2, l2 = ob.converge_sync(wc.CRIT, case.tmax, 1.0)
    print("wide relax %s: engine %d last %.3g; oracle %d last %.3g" % (case.id, n1, l1, n2, l2))
    assert n1 == -1 and n2 == -1 and np.isfinite(l1)
    assert bp.relaxation() == (0, -1, 1.0, 1.0) and ob.ar_levels() == (0, -1)
    assert bp.stats().psi_form_sweeps == 0


@pytest.mark.parametrize("case", wc.FIXED_MIX, ids=lambda c: c.id)
def test_wide_fixed_field_mix_and_the_field_gate(S, orc, case):
    """set_schedule(field_mix=0.25) with the machine off: S <- 0.75 S_prev + 0.25 sum_i psi_i on both sides, and convergence
    only once the lagging field would move by less than the criterion as well (rf in k_wfinalize)"""
    g, bp = _engine(S, case)
    bp.set_auto_relax(False)
    bp.set_schedule(field_mix=case.fixed_mix, check_every=1)
    og, ob = case.oracle(orc)
    _same_start(bp, ob)
    n1, l1 = bp.converge(wc.CRIT, case.tmax, 1.0)
    n2, l2 = ob.converge_sync(wc.CRIT, case.tmax, 1.0)
    fl, gl, mix, damp = bp.relaxation()
    print("wide relax %s: engine %d sweeps last %.3g; oracle %d sweeps last %.3g" % (case.id, n1, l1, n2, l2))
    assert n2 == case.niter and (fl, gl) == ob.ar_levels() == (0, -1) and (mix, damp) == (case.fixed_mix, 1.0)
    assert n1 >= 0 and abs(n1 - n2) <= 2 and l1 < wc.CRIT, (n1, n2, l1)
    d_fix = _fixed_point(orc, case, bp)
    d_psi = np.abs(bp.get_state()[0] - ob.get_state()[0]).max()
    assert d_psi < 1e-7, d_psi
    d_f, d_em, d_e = _reductions(orc, case, bp)
    print("wide relax %s: plain sweep moves %.3g, marginals %.3g, free energy parts %.3g, EM %.3g %.3g %.3g" % ((case.id, d_fix, d_psi, d_f) + d_em))
    assert bp.stats().psi_form_sweeps == 0


# ---------------------------------------------------------------------------------------------------------------------
# B. more than 1024 segments: the two-stage fold of the sweep and reduction records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc,N", wc.RING)
def test_wide_two_stage_fold_on_the_ring(S, orc, Q, dc, N):
    t = wc.ring_instance(Q, dc, N)
    segs, chunk, nb, last_rows = wc.RING_SIZES[N]
    bounds, hubs = bg.segment_model(t["deg"], wc.WCAP, wc.WRCAP)
    assert len(bounds) - 1 == segs and not hubs and wc.fold_model(segs) == (chunk, nb, last_rows)
    g = S.Graph.from_edges(t["pairs"], N)
    og, ob = wc.ring_oracle(orc, t)
    assert g.E2 == og.E2 == 2 * len(t["pairs"])
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, Q, dc), t["flag"], t["conf"], t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    assert bp.stats().n_blocks == segs, (bp.stats().n_blocks, segs)  # WCAP / WRCAP as modelled: the case is on its edge
    _same_start(bp, ob)
    psi0 = bp.get_state()[0]
    clamped = t["conf"] != -1
    d_sweep = 0.0
    for k, damp in enumerate(wc.RING_DAMPS):
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        (psi, msg), (opsi, omsg) = bp.get_state(), ob.get_state()
        seen = max(abs(d1 - d2), np.abs(psi - opsi).max(), np.abs(msg - omsg).max())
        d_sweep = max(d_sweep, seen)
        assert abs(d1 - d2) < 1e-11, (k, d1, d2)  # the sticky maximum through both stages
        assert np.abs(psi - opsi).max() < 1e-11 and np.abs(msg - omsg).max() < 1e-11, k  # the field sums through both stages
    assert np.array_equal(bp.get_state()[0][clamped], psi0[clamped])
    d_ov = abs(bp.compute_overlap() - ob.overlap())
    assert d_ov < 1e-11
    # the reductions (k_wreduce records, stride WR_NP + 1, through fold_to_host): site and edge parts, and the whole free energy
    # with the moment series on both sides (the exact non-edge loop is O(N^2 Q^2): out of reach for the oracle at this N)
    ob.compute_h()
    bp.set_nonedge_mode(2, 2)
    f, fp = bp.compute_free_energy(parts=True)
    fo, fop = ob.free_energy(2)
    d_f = _rel(fp, fop)
    assert _rel(fp[:2], fop[:2]) <= 1e-9, (fp, fop)
    assert d_f <= 1e-9 and abs(f - fo) <= 1e-9 * max(1.0, abs(fo)), (f, fo, fp, fop)
    bp.set_nonedge_mode(0, 0)
    na1, nna1, cab1 = bp.em_expectations()
    na2, nna2, cab2 = ob.em_expect()
    d_em = (np.abs(na1 - na2).max(), np.abs(nna1 - nna2).max(), _rel(cab1, cab2))
    assert d_em[0] < 1e-9 and d_em[1] < 1e-8 and d_em[2] <= 1e-9, d_em
    note = ""
    if Q < 64:  # (the oracle costs 0.3 s per sweep at Q = 64)
        n1, l1 = bp.converge(wc.CRIT, 600, 1.0)
        n2, l2 = ob.converge_sync(wc.CRIT, 600, 1.0)
        assert n1 == n2, (n1, n2, l1, l2)  # the same sweep
        assert n1 >= 0 and l1 < wc.CRIT
        d_psi = np.abs(bp.get_state()[0] - ob.get_state()[0]).max()
        assert d_psi < 1e-9
        assert bp.relaxation()[:2] == ob.ar_levels() == (0, -1)
        note = ", converged at sweep %d, marginals %.3g" % (n1, d_psi)
    assert bp.stats().psi_form_sweeps == 0
    print("wide ring Q %d dc %d N %d (%d segments, fold %s): per sweep %.3g, overlap %.3g, free energy parts %.3g, EM %.3g %.3g %.3g%s"
          % (Q, dc, N, segs, "%d x %d + %d" % (nb - 1, chunk, last_rows) if chunk else "single stage", d_sweep, d_ov, d_f, d_em[0], d_em[1], d_em[2], note))
