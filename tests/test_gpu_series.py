"""The engine's moment series of the non-edge terms (engine.hip nonedge_terms, k_moments, contract, the adjacent
pairs of k_nonedge_adj / k_fe_psi / k_wreduce, and the sharded copy) - the path every free energy and entropy above
N = 32 768 takes. Three references:
* the oracle's series of the same order (checked itself against a numpy restatement in tests/test_oracle_series.py),
  at every order 1 .. Kmax(Q) and in every regime of Kmax;
* a restatement of the engine's automatic choice of the order and of the exact/series switch;
* the exact tiled kernels (mode 1) at N ~ 4e4, through the truncation remainder of tests/series_model.py."""
import numpy as np
import pytest

import series_model as sm

pytestmark = pytest.mark.gpu

# 78 full 512-row blocks of k_moments and a partial one of 101 rows (above Q = 16 the LDS stages hold fewer rows than a block)
N_BIG = 40_000 + 37
HUB = 1500  # one row above the frame segment (512 edges, 1024 at Q = 2; 64 on the wide path): a hub row


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _pairs(N, Q, seed, c=10.0, hub=HUB):
    from sbm_bp_amd import synth
    pairs, cin, cout = synth.planted_partition(N, Q, c, 0.1, seed)
    if hub:
        rng = np.random.default_rng(seed)
        nb = rng.choice(np.arange(6, N), hub, replace=False)
        pairs = np.concatenate([pairs, np.stack([np.full(hub, 5), nb], 1).astype(np.uint32)])
    return pairs, synth.cab_matrix(Q, cin, cout), np.array(synth.group_sizes(N, Q), dtype=np.uint32), synth.true_conf(N, Q)


def _setup(S, orc, N, Q, beta, seed, c=10.0, hub=HUB):
    pairs, cab, na, tc = _pairs(N, Q, seed, c, hub)
    g = S.Graph.from_edges(pairs, N)
    og = orc.Graph.from_edges(pairs, N)
    rp, nbr, _ = g.csr()
    assert (rp == og.row_ptr).all() and (nbr == og.nbr).all()
    if hub:
        assert g.max_degree >= HUB
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, Q, 0), 0, None, tc, seed)
    bp.set_beta(beta)
    bp.expand_bp_params(S.bp_blockmodel_state(cab, na))
    ob = orc.OracleBP(og, Q, 0)
    ob.init_messages(0, None, tc, orc.Rng(seed))
    ob.set_params(cab, na, beta)
    return g, og, bp, ob, cab, na, tc


def _state(bp, ob, kind, N, Q, seed):
    """'sweeps': three undamped sweeps from the seeded state (marginals consistent with the messages: the fused reduction
    pass); 'random': marginals set with set_state (Dirichlet rows, some near one-hot, some with exact zeros)"""
    if kind == "sweeps":
        for _ in range(3):
            bp.sweep(1, 1.0)
        psi, msg = bp.get_state()
    else:
        msg = bp.get_state(psi=False)[1]
        psi = sm.random_marginals(N, Q, seed)
        bp.set_state(psi, msg)
    ob.set_state(psi, msg)
    return psi


def _parts(bp, mode, order):
    """part 2 (non-edge) of the free energy and of the entropy. compute_free_energy first: above Q = 16 the fused pass
    (k_wreduce) produces the adjacent pairs the series needs (engine.hip nonedge_terms)"""
    bp.set_nonedge_mode(mode, order)
    f = bp.compute_free_energy(parts=True)[1][2]
    e = bp.compute_entropy(parts=True)[1][2]
    return f, e


def _rel(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize("kind", ["sweeps", "random"])
@pytest.mark.parametrize("Q,beta", [(2, 1.0), (3, 0.8), (4, 1.0), (5, 1.0), (8, 1.0), (9, 0.8), (12, 1.0), (16, 1.0),
                                    (17, 1.0), (32, 0.8), (33, 1.0), (64, 1.0)])
def test_series_every_order_against_the_oracle(S, orc, Q, beta, kind):
    """every order 1 .. Kmax(Q) (4 up to Q = 8, 3 for 9 .. 16, 2 above; the largest moment tensors k_moments takes are
    4680 entries at Q = 8, 4368 at Q = 16, 4160 at Q = 64) against the oracle's series of the same order on the same state;
    then the automatic mode against the order the engine's rule must pick"""
    N = N_BIG
    g, og, bp, ob, cab, na, tc = _setup(S, orc, N, Q, beta, seed=Q)
    _state(bp, ob, kind, N, Q, seed=100 + Q)
    Kmax = sm.max_series_order(Q)
    assert Kmax == (4 if Q <= 8 else 3 if Q <= 16 else 2)
    got = {}
    for K in range(1, Kmax + 1):
        f, e = got[K] = _parts(bp, 2, K)
        fo, eo = ob.nonedge(K)
        assert _rel(f, fo, 1e-11), (K, f, fo)
        assert _rel(e, eo, 1e-11), (K, e, eo)
    # orders above the cap are the cap (sbmbp_set_nonedge_mode takes up to 4)
    if Kmax < 4:
        assert _parts(bp, 2, 4) == got[Kmax]
    # the automatic mode above N = 32 768: the series of the order the rule picks (here always the cap)
    Ke = sm.choose_series_order(N, Q, cab, beta)
    assert Ke == Kmax
    f0, e0 = _parts(bp, 0, 0)
    assert _rel(f0, got[Ke][0], 1e-15) and _rel(e0, got[Ke][1], 1e-15), (f0, e0, got[Ke])
    bp.set_nonedge_mode(0, 0)


def test_automatic_order_below_the_cap(S):
    """N = 1e6, Q = 2, c = 3 (BASELINE C2): the rule's 1e-12 target is met at order 3, one below the cap"""
    from sbm_bp_amd import synth
    N, Q = 1_000_000, 2
    pairs, cin, cout = synth.planted_partition(N, Q, 3.0, 0.1, 1)
    cab = synth.cab_matrix(Q, cin, cout)
    g = S.Graph.from_edges(pairs, N)
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, Q, 0), 0, None, synth.true_conf(N, Q), 1)
    bp.expand_bp_params(S.bp_blockmodel_state(cab, np.array(synth.group_sizes(N, Q), dtype=np.uint32)))
    bp.sweep(2, 1.0)
    Ke = sm.choose_series_order(N, Q, cab, 1.0)
    assert Ke == 3 < sm.max_series_order(Q)
    f3, e3 = _parts(bp, 2, 3)
    f0, e0 = _parts(bp, 0, 0)
    assert _rel(f0, f3, 1e-15) and _rel(e0, e3, 1e-15), (f0, f3, e0, e3)


@pytest.mark.parametrize("Q", [4, 20])
def test_exact_series_switch_at_32768(S, orc, Q):
    """mode 0 is the exact loop up to N = 32 768 and the series from 32 769 on"""
    for N in (32_768, 32_769):
        g, og, bp, ob, cab, na, tc = _setup(S, orc, N, Q, 1.0, seed=7 + Q, hub=0)
        for _ in range(2):
            bp.sweep(1, 1.0)
        f0, e0 = _parts(bp, 0, 0)
        f1, e1 = _parts(bp, 1, 0)
        Ke = sm.choose_series_order(N, Q, cab, 1.0)
        f2, e2 = _parts(bp, 2, Ke)
        if N == 32_768:
            assert _rel(f0, f1, 1e-15) and _rel(e0, e1, 1e-15), (f0, f1, e0, e1)
        else:
            assert _rel(f0, f2, 1e-15) and _rel(e0, e2, 1e-15), (f0, f2, e0, e2)
        if Q == 20:  # order 2 leaves ~1e-7 here: the two modes are told apart
            assert abs(f2 - f1) > 1e-9
        bp.set_nonedge_mode(0, 0)


@pytest.mark.parametrize("Q", [4, 12, 32, 64])
def test_series_truncation_against_the_exact_tiled_kernels(S, orc, Q):
    """the automatic series against the exact tiled kernels (k_nonedge_exact / k_wnonedge_exact, mode 1) at N ~ 4e4.
    Every omitted term of f is positive (w >= 0), so with T the first omitted term and x = max y over all pairs:
    T <= f_series - f_exact <= T / (1 - x). The entropy remainder is an identity. T, x and the entropy remainder come from
    the engine's own marginals, pairwise on the host (tests/series_model.py)."""
    N = N_BIG
    g, og, bp, ob, cab, na, tc = _setup(S, orc, N, Q, 1.0, seed=50 + Q)
    psi = _state(bp, ob, "sweeps", N, Q, 0)
    f1, e1 = _parts(bp, 1, 0)
    fs, es = _parts(bp, 0, 0)
    Ke = sm.choose_series_order(N, Q, cab, 1.0)
    rp, nbr, _ = g.csr()
    m = sm.pair_terms(psi, cab, 1.0, rp, nbr, [Ke], exact=(Q == 4), series=False)
    T, x, erem = m["T"][Ke], m["x"], m["e_rem"][Ke]
    d = 1e-12 * max(1.0, abs(fs))
    # at Q = 4 (order 4) T is ~1e-13, below the round-off allowance d: there only the upper side says anything
    assert T - d <= fs - f1 <= T / (1.0 - x) + d, (fs - f1, T, T / (1.0 - x))
    assert abs((e1 - es) - erem) <= 1e-12 * max(1.0, abs(es)), (e1 - es, erem)
    print("truncation Q=%d K=%d N=%d: f_series - f_exact = %.3g (T = %.3g), e_exact - e_series = %.3g" % (Q, Ke, N, fs - f1, T, e1 - es))
    if Q == 4:  # the exact tiled kernel at a size it was never compared at: sum log(psi_i^T P psi_l) minus the adjacent pairs
        assert _rel(f1, m["f_exact"], 1e-12) and _rel(e1, m["e_exact"], 1e-12), (f1, m["f_exact"], e1, m["e_exact"])
    bp.set_nonedge_mode(0, 0)


@pytest.mark.parametrize("Q", [6, 12])
def test_sharded_series_equals_single_engine_and_oracle(S, orc, Q):
    """sbmbp_shard_nonedge_partial / _finish over 3 ranks at N = 4e4: order 4 (Q = 6) and 3 (Q = 12)"""
    from sbm_bp_amd.distributed import LocalShards
    N = 40_000
    g, og, bp, ob, cab, na, tc = _setup(S, orc, N, Q, 1.0, seed=300 + Q)
    sb = LocalShards(g, Q, 0, 3)
    try:
        sb.init_messages(0, None, tc, 300 + Q, True)
        sb.expand_bp_params(cab, na, 1.0)
        for _ in range(3):
            bp.sweep(1, 1.0)
            sb.sweep(1, 1.0)
        f1, fp1 = bp.compute_free_energy(parts=True)
        e1, ep1 = bp.compute_entropy(parts=True)
        fk, fpk = sb.compute_free_energy(parts=True)
        ek, epk = sb.compute_entropy(parts=True)
    finally:
        sb.close()
    assert _rel(fk, f1, 1e-12) and _rel(ek, e1, 1e-12), (fk, f1, ek, e1)
    for a, b in zip(list(fpk) + list(epk), list(fp1) + list(ep1)):
        assert _rel(a, b, 1e-12), (fpk, fp1, epk, ep1)
    Ke = sm.choose_series_order(N, Q, cab, 1.0)
    assert Ke == (4 if Q == 6 else 3)
    psi, msg = bp.get_state()
    ob.set_state(psi, msg)
    fo, eo = ob.nonedge(Ke)
    assert _rel(fpk[2], fo, 1e-11) and _rel(epk[2], eo, 1e-11), (fpk[2], fo, epk[2], eo)
