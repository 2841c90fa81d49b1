"""The per-vertex prior (include/sbmbp.h sbmbp_set_vertex_prior) on the GPU: k_sweep_prior, the hub
cavity kernel and the message-form reductions under a prior, against tests/prior_model.py (oracle calls stitched per prior
class), the oracle with other group sizes, the clamped engine and numpy. Tolerances are the project's: 1e-11 per sweep against
the oracle (tests/test_gpu_boundary.py), 1e-9 on free-energy parts and EM expectations, 1e-8 on entropy parts, 1e-13 / 1e-12
between two runs of the engine's own kernels. Each case prints the largest differences it saw."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import boundary_graph as bg
import prior_model as pm
from conftest import ROOT, args_of, best_perm_diff, golden, gpath
from test_gpu_parity import engine_from

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _rel(a, b):
    """max |a - b| / max(1, max |b|) over the entries where b is finite; a must be finite there (tests/test_gpu_boundary.py)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    assert np.isfinite(a[fin]).all(), (a, b)
    return float(np.abs(a[fin] - b[fin]).max() / max(1.0, np.abs(b[fin]).max())) if fin.any() else 0.0


_CASES = {}


def case(Q, dc):
    """the boundary graph of this Q's (CAP, RCAP) - a segment exactly at CAP edges and one the next row would overflow, rows of
    BIG_ROW and BIG_ROW + 1 edges, hub rows of CAP + 1 edges, isolated vertices - plus one more last row: a hub of 2 * 256 + 1
    edges (three fragments, the last holding one edge)"""
    t = bg.instance(Q, dc)
    key = (t["cap"], t["rcap"])
    if key not in _CASES:
        N, ns = t["N"], t["ns"]
        extra = np.stack([np.full(2 * bg.FRAG + 1, N, dtype=np.uint32), (ns + np.arange(2 * bg.FRAG + 1)).astype(np.uint32)], 1)
        pairs = np.concatenate([t["pairs"], extra])
        deg = bg.degrees(pairs, N + 1)
        hubs = bg.segment_model(deg, t["cap"], t["rcap"])[1]
        assert deg[N] == 2 * bg.FRAG + 1 and N in hubs and 0 in hubs and deg[0] == t["cap"] + 1
        assert {t["cap"], 32, 33, 0} <= set(int(d) for d in deg[:ns]) and (deg[N - 4:N - 1] == 0).all()
        _CASES[key] = dict(pairs=pairs, N=N + 1, deg=deg, hubs=hubs, isolated=N - 4)
    c = _CASES[key]
    cab, na, tc = bg.params(Q, c["N"], dc, c["pairs"])
    return dict(t, **c, cab=cab, na=na, tc=tc)


def three_classes(t, Q):
    """(weights[3][Q] of small positive integers, class of every row): the hub of CAP + 1 edges, the hub of 2 * 256 + 1 edges
    and an isolated vertex in three different classes, the other rows round-robin"""
    rng = np.random.default_rng(900 + Q)
    weights = rng.integers(1, 5, size=(3, Q)).astype(np.int64)
    weights[np.arange(3), np.arange(3) % Q] += 2  # no class is a constant line
    cls = np.arange(t["N"]) % 3
    cls[0], cls[t["N"] - 1], cls[t["isolated"]] = 0, 1, 2
    return weights, cls


def engine(S, t, g=None, kind="conditional"):
    g = g or S.Graph.from_edges(t["pairs"], t["N"])
    bp = S.bp_conditional() if kind == "conditional" else S.bp_basic()
    bp.init_messages(S.blockmodel_t(g, t["Q"], t["dc"]), 0, None, t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    return g, bp


def oracle(orc, t, na=None):
    og = orc.Graph.from_edges(t["pairs"], t["N"])
    ob = orc.OracleBP(og, t["Q"], t["dc"])
    ob.init_messages(0, None, t["tc"], orc.Rng(t["seed"]))
    ob.set_params(t["cab"], t["na"] if na is None else na, 1.0)
    return og, ob


# ---------------------------------------------------------------------------------------------------------------------
# 1. every instantiation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(Q, dc) for Q in range(2, 17) for dc in (0, 1)] + [(Q, 2) for Q in (2, 8, 16)])
def test_every_instantiation_against_the_model(S, orc, Q, dc):
    t = case(Q, dc)
    weights, cls = three_classes(t, Q)
    g, bp = engine(S, t)
    og, ob = oracle(orc, t)
    assert bp.stats().n_hub_rows == len(t["hubs"]) and len(t["hubs"]) >= 6
    bp.set_vertex_prior(pm.classes_of(weights, cls))
    bp.reset_stats()
    worst = 0.0
    for k, damp in enumerate((0.7, 1.0, 1.0)):
        d1, d2 = bp.sweep(1, damp), pm.sweep(ob, t["cab"], t["na"], weights, cls, damp)
        (psi, msg), (opsi, omsg) = bp.get_state(), ob.get_state()
        seen = max(np.abs(psi - opsi).max(), np.abs(msg - omsg).max(), abs(d1 - d2))
        worst = max(worst, seen)
        assert seen <= 1e-11, ("sweep %d" % k, np.abs(psi - opsi).max(), np.abs(msg - omsg).max(), d1, d2)
    st = bp.stats()
    assert st.psi_form_sweeps == 0 and st.sweeps == 3
    print("prior Q %d dc %d cap %d: per sweep %.3g" % (Q, dc, t["cap"], worst))


# ---------------------------------------------------------------------------------------------------------------------
# 2. a uniform prior is no prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(3, 0), (5, 1)])
@pytest.mark.parametrize("table", ["ones", "row_constants"])
def test_uniform_prior_is_no_prior(S, Q, dc, table):
    t = case(Q, dc)
    g, plain = engine(S, t)
    plain.set_gather_mode(1)
    _, bp = engine(S, t, g)
    c = np.ones(t["N"]) if table == "ones" else np.random.default_rng(3).uniform(0.25, 4.0, size=t["N"])
    bp.set_vertex_prior(np.repeat(c[:, None], Q, 1))
    b0 = plain.stats().bytes_per_sweep
    assert bp.stats().bytes_per_sweep == b0 + 8.0 * Q * t["N"]
    for damp in (0.7, 1.0, 1.0):
        d1, d2 = bp.sweep(1, damp), plain.sweep(1, damp)
        assert abs(d1 - d2) <= 1e-13
    seen = max(np.abs(x - y).max() for x, y in zip(bp.get_state(), plain.get_state()))
    assert seen <= 1e-13, seen
    n1, n2 = bp.converge(1e-10, 600, 1.0)[0], plain.converge(1e-10, 600, 1.0)[0]
    assert n1 == n2 and n1 >= 0
    plain.set_state(*bp.get_state())  # the reductions on ONE state
    (f1, p1), (f2, p2) = bp.compute_free_energy(parts=True), plain.compute_free_energy(parts=True)
    shift = float(np.log(c).sum()) / t["N"]  # scaling row i by c_i: log Z_i grows by log c_i
    assert abs((p1[0] - p2[0]) - shift) <= 1e-12 and np.abs(p1[1:] - p2[1:]).max() <= 1e-12, (p1, p2, shift)
    assert abs((f1 - f2) + shift) <= 1e-12  # the free energy takes f_site with a minus sign
    if dc == 0:
        (e1, q1), (e2, q2) = bp.compute_entropy(parts=True), plain.compute_entropy(parts=True)
        assert np.abs(q1 - q2).max() <= 1e-12 and abs(e1 - e2) <= 1e-12, (q1, q2)  # a constant cancels in e_site's ratio
    assert bp.stats().psi_form_sweeps == 0
    print("uniform prior (%s) Q %d dc %d: state %.3g, niter %d, f_site shift %.3g" % (table, Q, dc, seen, n1, shift))


# ---------------------------------------------------------------------------------------------------------------------
# 3. a one-hot prior is a clamp
# ---------------------------------------------------------------------------------------------------------------------
def test_one_hot_prior_is_a_clamp(S):
    gd = golden("c1_planted_i1_seed0")
    a, r = args_of(gd), gd["result"]
    assert a["init_flag"] == 1
    _, _, clamped, _ = engine_from(S, a)             # bp_conditional: the planted rows are clamped
    _, _, bp, _ = engine_from(S, a, learn=True)      # bp_basic: every row is updated
    planted = np.flatnonzero(a["beliefs"] != -1)
    prior = np.ones((a["N"], a["Q"]))
    prior[planted] = 0.0
    prior[planted, a["beliefs"][planted]] = 1.0
    bp.set_vertex_prior(prior)
    assert all(np.array_equal(x, y) for x, y in zip(bp.get_state(), clamped.get_state()))
    seen = 0.0
    for _ in range(3):
        d1, d2 = bp.sweep(1, 1.0), clamped.sweep(1, 1.0)
        seen = max([seen, abs(d1 - d2)] + [np.abs(x - y).max() for x, y in zip(bp.get_state(), clamped.get_state())])
        assert seen <= 1e-13, seen
    niter, last = bp.converge(1e-13, 5000, 1.0)
    assert niter >= 0 and last < 1e-13
    psi = bp.real_psi()
    d, _ = best_perm_diff(psi, np.array(r["psi"]).reshape(psi.shape))
    assert d < 1e-9  # tests/test_gpu_parity.py test_converged_fixed_point_equals_reference_golden
    assert bp.stats().psi_form_sweeps == 0 and len(planted) > 0
    print("one-hot prior against the clamp: 3 sweeps %.3g, fixed point against the golden %.3g" % (seen, d))


# ---------------------------------------------------------------------------------------------------------------------
# 4. one prior line on every row is other group sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(3, 0), (3, 1), (16, 0), (16, 1)])
def test_row_constant_prior_is_other_group_sizes(S, orc, Q, dc):
    t = case(Q, dc)
    w = 1 + (np.arange(Q) * 2) % 5
    g, bp = engine(S, t)
    bp.set_vertex_prior(np.repeat(w[None, :].astype(float), t["N"], 0))
    og, ob = oracle(orc, t, na=t["na"] * w)
    sw = 0.0
    for damp in (0.7, 1.0, 1.0):
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        sw = max([sw, abs(d1 - d2)] + [np.abs(x - y).max() for x, y in zip(bp.get_state(), ob.get_state())])
        assert sw <= 1e-11, sw
    f, fp = bp.compute_free_energy(parts=True)
    em = bp.em_expectations()
    ob.set_state(*bp.get_state())
    ob.compute_h()
    dfe = _rel(fp, ob.free_energy(0)[1])
    assert dfe <= 1e-9, (fp, ob.free_energy(0)[1])
    dent = 0.0
    if dc == 0:
        e, ep = bp.compute_entropy(parts=True)
        eop = ob.entropy(0)[1]  # (the reference's site entropy is NaN once a hub row underflows: the finite parts are compared)
        assert np.isfinite(eop[1:]).all() and np.isfinite(ep).all()
        dent = _rel(ep, eop)
        assert dent <= 1e-8, (ep, eop)
    dem = max(_rel(x, y) for x, y in zip(em, ob.em_expect()))
    assert dem <= 1e-9
    print("row-constant prior Q %d dc %d: per sweep %.3g, free-energy parts %.3g, entropy parts %.3g, EM %.3g" % (Q, dc, sw, dfe, dent, dem))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the site term under a row-varying prior, against a sum formed here
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [4, 9])
def test_site_term_with_a_row_varying_prior(S, Q):
    t = case(Q, 0)
    g, bp = engine(S, t)
    prior = np.random.default_rng(11).uniform(0.1, 3.0, size=(t["N"], Q))
    prior[::7, 1] = 0.0  # some forbidden labels
    bp.set_vertex_prior(prior)
    bp.sweep(2, 1.0)
    f, parts = bp.compute_free_energy(parts=True)
    psi, msg = bp.get_state()
    rp, nbr, rev = g.csr()
    rp = rp.astype(np.int64)
    src = np.repeat(np.arange(t["N"]), np.diff(rp))
    h = bp.h()
    eta = t["na"].astype(float) / t["N"]
    with np.errstate(divide="ignore"):
        la = np.log(prior) + np.log(eta)[None, :] - h[None, :] / t["N"]
        np.add.at(la, src, np.log(msg[rev.astype(np.int64)] @ t["cab"]))
    m = la.max(1)
    f_site = float((m + np.log(np.exp(la - m[:, None]).sum(1))).sum()) / t["N"]
    assert abs(parts[0] - f_site) <= 1e-9 * max(1.0, abs(f_site)), (parts[0], f_site)
    _, plain = engine(S, t, g)
    plain.set_gather_mode(1)
    plain.set_state(psi, msg)
    _, pp = plain.compute_free_energy(parts=True)
    assert np.abs(parts[1:] - pp[1:]).max() <= 1e-12 and abs(parts[0] - pp[0]) > 1e-3, (parts, pp)
    print("site term Q %d: %.3g against the numpy sum; edge / non-edge parts against the plain engine %.3g"
          % (Q, abs(parts[0] - f_site), np.abs(parts[1:] - pp[1:]).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 6. zero components
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(3, 0), (8, 1), (16, 0)])
def test_zero_components_forbid_a_label(S, Q, dc):
    t = case(Q, dc)
    g, bp = engine(S, t)
    rp, nbr, rev = g.csr()
    rp = rp.astype(np.int64)
    rows = bg.named_rows(t["cap"], t["rcap"])
    zero_rows = sorted(set([rows["d32"], rows["d33"], rows["cap_row"], rows["ones_first"], rows["zero_first"], 0, t["N"] - 1]
                           + list(range(t["ns"], t["N"], 5))))
    assert {32, 33, t["cap"], 1, 0, t["cap"] + 1, 2 * bg.FRAG + 1} <= set(int(t["deg"][i]) for i in zero_rows)  # short, wave-product, hub
    prior = np.random.default_rng(17).uniform(0.5, 2.0, size=(t["N"], Q))
    zl = np.array(zero_rows) % Q
    prior[zero_rows, zl] = 0.0
    assert ((prior[zero_rows] > 0).sum(1) >= 2).all()  # not one-hot
    tiny = prior.copy()
    tiny[zero_rows, zl] = 1e-300
    bp.set_vertex_prior(prior)
    edge_zero = np.zeros((g.E2, Q), dtype=bool)
    for i, q in zip(zero_rows, zl):
        edge_zero[rp[i]:rp[i + 1], q] = True
    worst = 0.0
    for k in range(2):
        psi0, msg0 = bp.get_state()
        bp.sweep(1, 1.0)
        psi, msg = bp.get_state()
        assert np.isfinite(psi).all() and np.isfinite(msg).all()
        assert (psi[zero_rows, zl] == 0.0).all() and (msg[edge_zero] == 0.0).all()
        mpsi, mmsg, _ = pm.numpy_sweep(rp, nbr, rev, psi0, msg0, t["cab"], t["na"], tiny, dc, 1.0)
        keep_p = np.ones_like(psi, dtype=bool)
        keep_p[zero_rows, zl] = False
        worst = max(worst, np.abs(psi - mpsi)[keep_p].max(), np.abs(msg - mmsg)[~edge_zero].max())
        assert worst <= 1e-11, (k, worst)
        assert mpsi[zero_rows, zl].max() < 1e-250  # (what the model makes of 1e-300)
    print("zero components Q %d dc %d: other entries against the model at 1e-300: %.3g" % (Q, dc, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 7. life cycle and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle(S):
    t = case(4, 0)
    g, bp = engine(S, t)
    assert bp.vertex_prior() is None
    prior = np.random.default_rng(5).uniform(0.5, 2.0, size=(t["N"], 4))
    bp.set_vertex_prior(prior)
    assert np.array_equal(bp.vertex_prior(), prior)
    bp.sweep(2, 1.0)
    with_prior = bp.get_state()
    # the same engine: new initial state, new parameters, a declared state - the prior stays
    bp.reinit_messages_device(t["tc"], 3)
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"] * 1.1, t["na"]))
    bp.set_state(*bp.get_state())
    assert np.array_equal(bp.vertex_prior(), prior)
    # a new engine over the same model (init_messages allocates one): the prior goes with it
    bp.init_messages(S.blockmodel_t(g, 4, 0), 0, None, t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    assert np.array_equal(bp.vertex_prior(), prior)
    bp.sweep(2, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(bp.get_state(), with_prior)) and bp.stats().psi_form_sweeps == 0
    # replaced by the next call, removed by None: the no-prior trajectory, bit for bit, marginal-gather sweeps included
    bp.set_vertex_prior(prior * 2.0)
    assert np.array_equal(bp.vertex_prior(), prior * 2.0)
    bp.init_messages(S.blockmodel_t(g, 4, 0), 0, None, t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    bp.set_vertex_prior(None)
    assert bp.vertex_prior() is None
    _, plain = engine(S, t, g)
    for b in (bp, plain):
        b.reset_stats()
        b.sweep(3, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(bp.get_state(), plain.get_state()))
    assert bp.stats().psi_form_sweeps == plain.stats().psi_form_sweeps == 2
    assert bp.stats().bytes_per_sweep == plain.stats().bytes_per_sweep
    assert bp.compute_free_energy() == plain.compute_free_energy()
    # argument errors: reported before anything changes, the first offending vertex named
    for bad, what in ((-1.0, "negative"), (np.nan, "NaN"), (np.inf, "Inf")):
        p = prior.copy()
        p[17, 2] = bad
        p[40, 0] = bad
        with pytest.raises(S.SbmbpError) as ei:
            bp.set_vertex_prior(p)
        assert ei.value.code == -1 and "vertex 17" in str(ei.value) and what in str(ei.value)
    p = prior.copy()
    p[23] = 0.0
    with pytest.raises(S.SbmbpError) as ei:
        bp.set_vertex_prior(p)
    assert ei.value.code == -1 and "vertex 23" in str(ei.value)
    assert bp.vertex_prior() is None


def test_refusals(S):
    lib = S.load_library()
    rng = np.random.default_rng(0)
    N = 200
    g = S.Graph.from_edges(rng.integers(0, N, size=(600, 2)).astype(np.uint32), N)
    # Q = 20: the matrix-core kernels take no prior
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, 20, 0), 0, None, rng.integers(0, 20, size=N).astype(np.uint32), 0)
    bp.expand_bp_params(S.bp_param_from_epsilon_c(S.blockmodel_t(g, 20, 0), 0.1, 3.0))
    with pytest.raises(S.SbmbpError) as ei:
        bp.set_vertex_prior(np.ones((N, 20)))
    assert ei.value.code == -6 and "Q = 16" in str(ei.value) and bp.vertex_prior() is None
    assert np.isfinite(bp.sweep(1, 1.0))
    # the coloured order, both ways round
    bm = S.blockmodel_t(g, 4, 0)
    tc = rng.integers(0, 4, size=N).astype(np.uint32)
    bp = S.bp_conditional()
    bp.init_messages(bm, 0, None, tc, 0)
    bp.expand_bp_params(S.bp_param_from_epsilon_c(bm, 0.1, 3.0))
    bp.set_sweep_order("coloured")
    with pytest.raises(S.SbmbpError) as ei:
        bp.set_vertex_prior(np.ones((N, 4)))
    assert ei.value.code == -6 and "coloured" in str(ei.value) and bp.vertex_prior() is None
    assert np.isfinite(bp.sweep(1, 1.0)) and bp.sweep_order()[0] == 1
    bp.set_sweep_order("jacobi")
    bp.set_vertex_prior(np.full((N, 4), 2.0))
    with pytest.raises(S.SbmbpError) as ei:
        bp.set_sweep_order("coloured")
    assert ei.value.code == -6 and "prior" in str(ei.value) and bp.sweep_order()[0] == 0
    assert np.isfinite(bp.sweep(1, 1.0)) and bp.vertex_prior() is not None
    # a shard engine of the step interface (one shard owning every row)
    import torch
    from sbm_bp_amd.capi import ShardDesc, c_dp, c_u32p, c_u64p
    rp, nbr, _ = g.csr()
    psi0, psi1 = (torch.zeros(N * 4, dtype=torch.float64, device="cuda") for _ in range(2))
    red = torch.zeros(8192, dtype=torch.float64, device="cuda")
    desc = ShardDesc(n_global=N, n_own=N, n_halo=0, row0=0, n_edges=g.E2, edge0=0, row_ptr=rp.ctypes.data_as(c_u64p),
                     nbr_local=nbr.ctypes.data_as(c_u32p), psi_buf0=psi0.data_ptr(), psi_buf1=psi1.data_ptr(), red_buf=red.data_ptr(),
                     n_chunks=0, chunk_row=None, rev_local=None, n_halo_msgs=0, table_deg=None)
    h = C.c_void_p()
    assert lib.sbmbp_shard_create(C.byref(h), C.byref(desc), 4, 0, 0) == 0, lib.sbmbp_last_error()
    ones = np.ones((N, 4))
    present = C.c_int(7)
    assert lib.sbmbp_set_vertex_prior(h, ones.ctypes.data_as(c_dp)) == -6 and b"shard" in lib.sbmbp_last_error()
    assert lib.sbmbp_get_vertex_prior(h, None, C.byref(present)) == 0 and present.value == 0
    assert lib.sbmbp_set_vertex_prior(h, None) == 0
    lib.sbmbp_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 8. learning and the command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(3, 0), (4, 1)])
def test_learning_first_em_step_follows_the_oracle(S, orc, Q, dc):
    """the prior is held fixed and the reference's update rules run unchanged: with one prior line w on every row the first EM
    step is the oracle's with group sizes na * w (after it the two differ by construction: the oracle re-learns na * w)"""
    t = case(Q, dc)
    w = 1 + np.arange(Q) % 3
    g, bp = engine(S, t, kind="basic")
    bp.set_vertex_prior(np.repeat(w[None, :].astype(float), t["N"], 0))
    og, ob = oracle(orc, t, na=t["na"] * w)
    ob.set_msg_form(True)  # under a prior the engine gathers messages: every sweep reports the 1-step difference
    # what the first EM step sees: the BP run from the initial state, then the expectations and the free energy
    n1, n2 = bp.converge(1e-6, 40, 1.0)[0], ob.converge_sync(1e-6, 40, 1.0)[0]
    assert n1 == n2
    dem = max(_rel(x, y) for x, y in zip(bp.em_expectations(), ob.em_expect()))
    assert dem <= 1e-9
    # and sbmbp_learning itself, one EM step from the same start
    _, bp = engine(S, t, kind="basic")
    bp.set_vertex_prior(np.repeat(w[None, :].astype(float), t["N"], 0))
    _, ob = oracle(orc, t, na=t["na"] * w)
    res = bp.learning(None, S.bp_blockmodel_state(t["cab"], t["na"]), 1e-6, 1, 0.2, 1.0)
    steps, f = ob.learning(1e-6, 1, 0.2, 1.0, None, sync=True, series_K=0)
    assert res.em_steps == steps == 1 and abs(res.free_energy - f) <= 1e-9 * max(1.0, abs(f)), (res.free_energy, f)
    assert np.array_equal(bp.vertex_prior(), np.repeat(w[None, :].astype(float), t["N"], 0))
    print("learning under a prior Q %d dc %d: EM expectations %.3g, f %.3g" % (Q, dc, dem, abs(res.free_energy - f)))


def test_cli_prior_path(S, tmp_path):
    ds = gpath("c1_dataset.edgelist")
    rows = {3: (4, 1), 10: (1, 3), 57: (0, 1), 200: (2.5, 1), 499: (1, 1), 500: (1, 6), 731: (1, 0), 800: (0.25, 1), 901: (1, 2), 999: (3, 1)}
    p = tmp_path / "prior.txt"
    p.write_text("".join("%d %r %r\n" % (v, a, b) for v, (a, b) in sorted(rows.items(), reverse=True)))
    mj = tmp_path / "metrics.json"
    run = subprocess.run([os.path.join(ROOT, "bin", "bp"), "-l", ds, "-n", "500", "500", "--epsilon_c", "0.1", "3", "-m", "infer", "-d", "0",
                          "-t", "500", "--prior_path", str(p), "--metrics_json", str(mj)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    g = S.load_edge_list(ds, 1000)
    bm = S.blockmodel_t(g, 2, 0)
    bp = S.bp_conditional()
    bp.init_messages(bm, 0, None, np.repeat([0, 1], 500), 0)
    bp.set_schedule(1.0, 8)
    prior = S.load_priors(str(p), 1000, 2)
    assert (prior != 1.0).any(1).sum() == 9 and list(prior[3]) == [4, 1]
    bp.set_vertex_prior(prior)
    res = bp.inference(bm, S.bp_param_from_epsilon_c(bm, 0.1, 3.0), 5e-6, 500, 1.0)
    assert run.stdout == S.format_infer_line(res), (run.stdout, S.format_infer_line(res))
    m = json.load(open(mj))
    assert m["prior_rows"] == 10 and m["marginal_gather_sweeps"] == 0
    plain = subprocess.run([os.path.join(ROOT, "bin", "bp"), "-l", ds, "-n", "500", "500", "--epsilon_c", "0.1", "3", "-m", "infer", "-d", "0",
                            "-t", "500", "--metrics_json", str(mj)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and plain.stdout != run.stdout and "prior_rows" not in json.load(open(mj))
