"""Every label count the engine compiles a kernel instance for (DISPATCH_Q: Q = 2 .. 16; the instances differ in frame_cfg,
psi_waves, the index bits and the load form for odd Q) against the oracle's synchronous twin, the way tests/test_gpu_fuzz.py
compares a random instance: per sweep, to convergence, then the reductions. Each instance has isolated vertices, a long row
(~300 edges) and a hub row above every segment capacity (1100 edges); beta = 0.8 on odd Q, deg_corr_flag 1 on every third
Q; and a second run with 10 % of the rows clamped (-i 1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _instance(Q, clamp):
    from sbm_bp_amd import synth
    N = 3000
    rng = np.random.default_rng(6000 + Q)
    pairs, cin, cout = synth.planted_partition(N, Q, 10.0, 0.04, 60 + Q)
    pairs = pairs[(pairs[:, 0] < N - 6) & (pairs[:, 1] < N - 6)]  # the last six vertices stay isolated
    long_row = np.stack([np.full(300, 11), rng.choice(np.arange(20, N - 6), 300, replace=False)], 1)
    hub_row = np.stack([np.full(1100, 17), rng.choice(np.arange(20, N - 6), 1100, replace=False)], 1)
    pairs = np.concatenate([pairs, long_row, hub_row]).astype(np.uint32)
    dc = 1 if Q % 3 == 0 else 0
    cab = synth.cab_matrix(Q, cin, cout) * rng.uniform(0.8, 1.2, size=(Q, Q))
    cab = (cab + cab.T) / 2
    if dc:  # degree-corrected weights are d_i d_l cab: cab of order 1 / (mean degree)^2 (as tests/test_gpu_fuzz.py)
        cab = cab / (2.0 * len(pairs) / N) ** 2
    tc = synth.true_conf(N, Q)
    na = np.array(synth.group_sizes(N, Q), dtype=np.uint32)
    beta = 0.8 if (Q % 2 == 1 and dc == 0) else 1.0
    conf = None
    if clamp:
        conf = np.where(rng.random(N) < 0.1, tc.astype(np.int32), -1).astype(np.int32)
        conf[11] = int(tc[11])  # the long row is clamped too
    return dict(N=N, Q=Q, dc=dc, pairs=pairs, cab=cab, na=na, tc=tc, beta=beta, flag=int(clamp), conf=conf, seed=Q)


def _close(a, b, rel):
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("Q", list(range(2, 17)))
def test_label_count_against_the_oracle(S, orc, Q, clamp):
    t = _instance(Q, clamp)
    N, dc = t["N"], t["dc"]
    g = S.Graph.from_edges(t["pairs"], N)
    og = orc.Graph.from_edges(t["pairs"], N)
    assert g.E2 == og.E2 and g.max_degree >= 1100 and (og.deg[-6:] == 0).all()
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, Q, dc), t["flag"], t["conf"], t["tc"], t["seed"])
    bp.set_beta(t["beta"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    ob = orc.OracleBP(og, Q, dc)
    ob.init_messages(t["flag"], t["conf"], t["tc"], orc.Rng(t["seed"]))
    ob.set_params(t["cab"], t["na"], t["beta"])
    psi0 = bp.get_state()[0]
    bp.reset_stats()
    for k in range(5):
        damp = 0.7 if k < 2 else 1.0  # two damped sweeps (message-gather form), then undamped ones
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        psi, msg = bp.get_state()
        opsi, omsg = ob.get_state()
        assert np.abs(psi - opsi).max() < 1e-11 and np.abs(msg - omsg).max() < 1e-11, "sweep %d" % k
        assert abs(d1 - d2) < 1e-11, (k, d1, d2)
    # the undamped sweeps run in the marginal-gather form, all but the first: a damped sweep leaves marginals that are not
    # those of the message pair, so the next sweep forms them explicitly (engine.hip run_sweeps, first_explicit)
    assert bp.stats().psi_form_sweeps == 2
    if clamp:
        assert np.array_equal(bp.get_state()[0][t["conf"] != -1], psi0[t["conf"] != -1])
    n1, l1 = bp.converge(1e-10, 600, 1.0)
    n2, l2 = ob.converge_sync(1e-10, 600, 1.0)
    assert n1 == n2, (n1, n2, l1, l2)  # the same sweep - or both at the limit
    if n1 >= 0:
        assert l1 < 1e-10
        assert np.abs(bp.get_state()[0] - ob.get_state()[0]).max() < 1e-9
    # the reductions on the state reached: the fused pass (marginals consistent with the messages) ...
    f, fp = bp.compute_free_energy(parts=True)
    e, ep = bp.compute_entropy(parts=True)
    em = bp.em_expectations()
    # ... against the separate kernels (message-gather mode: no fused pass) ...
    bp.set_gather_mode(1)
    f_s, fp_s = bp.compute_free_energy(parts=True)
    e_s, ep_s = bp.compute_entropy(parts=True)
    em_s = bp.em_expectations()
    bp.set_gather_mode(0)
    assert _close(fp, fp_s, 1e-11), (fp, fp_s)
    for a, b in zip(em, em_s):
        assert _close(a, b, 1e-11)
    if dc:
        assert np.isnan(e) and np.isnan(e_s)
    else:
        assert _close(ep, ep_s, 1e-11), (ep, ep_s)
    # ... and against the oracle's exact terms on the engine's state (N < 32 768: the exact non-edge loop)
    psi, msg = bp.get_state()
    ob.set_state(psi, msg)
    ob.compute_h()
    fo, fop = ob.free_energy(0)
    assert _close(fp, fop, 1e-9), (fp, fop)
    eo, eop = ob.entropy(0)
    if dc:
        assert np.isnan(eo)
    else:
        # the reference's site entropy multiplies a row's factors directly (bp.cpp:506-560) and gives NaN once a row of a
        # few hundred edges underflows (the hub row here); the engine stays finite. The finite parts must agree.
        fin = np.isfinite(eop)
        assert fin[1:].all() and np.isfinite(ep).all()
        assert _close(np.asarray(ep)[fin], eop[fin], 1e-9), (ep, eop)
    for a, b in zip(em, ob.em_expect()):
        assert _close(a, b, 1e-9), (a, b)
