"""The oracle's moment series of the non-edge terms (bp_oracle.cpp f_nonedge_series / e_nonedge_series)
against a direct numpy restatement, at every order 1 .. Kmax(Q). The compiled reference has no series, so no golden pins
it; these checks make the oracle's series the reference the GPU tier (tests/test_gpu_series.py) compares the engine with.

Three checks per order K:
* same formula: oracle part 2 = the numpy series of order K (pairwise over all ordered pairs, minus the CSR-adjacent pairs);
* free-energy remainder: every omitted term y^k / k is positive for w >= 0, so with T the first omitted term summed over all
  pairs and x = max y,  T <= f_series(K) - f_exact <= T / (1 - x);
* entropy remainder, an identity: e_exact - e_series(K) = sum u yc^K / (1 - yc) / 2N."""
import numpy as np
import pytest

import series_model as sm


def _instance(orc, N, Q, beta, seed, extra=False, sweeps=3):
    from sbm_bp_amd import synth
    pairs, cin, cout = synth.planted_partition(N, Q, 10.0, 0.1, seed)
    if extra:  # a self-loop (one CSR entry) and five isolated vertices
        pairs = pairs[(pairs[:, 0] < N - 5) & (pairs[:, 1] < N - 5)]
        pairs = np.concatenate([pairs, np.array([[7, 7]], dtype=np.uint32)])
    tc = synth.true_conf(N, Q)
    cab = synth.cab_matrix(Q, cin, cout)
    na = np.array(synth.group_sizes(N, Q), dtype=np.uint32)
    og = orc.Graph.from_edges(pairs, N)
    ob = orc.OracleBP(og, Q, 0)
    ob.init_messages(0, None, tc, orc.Rng(seed))
    ob.set_params(cab, na, beta)
    for _ in range(sweeps):  # an unconverged state
        ob.sweep_sync(1.0)
    return og, ob, cab


def _check_orders(og, ob, cab, beta, exact_from_oracle):
    Q = ob.Q
    Kmax = sm.max_series_order(Q)
    psi = ob.get_state()[0]
    m = sm.pair_terms(psi, cab, beta, og.row_ptr, og.nbr, range(1, Kmax + 1))
    f_ex, e_ex = m["f_exact"], m["e_exact"]
    if exact_from_oracle:  # the numpy exact terms are the oracle's O(N^2 Q^2) loop (the one the goldens pin)
        fo0 = ob.free_energy(0)[1][2]
        eo0 = ob.entropy(0)[1][2]
        assert abs(f_ex - fo0) <= 1e-12 * max(1.0, abs(fo0)), (f_ex, fo0)
        assert abs(e_ex - eo0) <= 1e-12 * max(1.0, abs(eo0)), (e_ex, eo0)
    assert 0.0 < m["x"] < 0.5
    for K in range(1, Kmax + 1):
        fK = ob.free_energy(K)[1][2]
        eK = ob.entropy(K)[1][2]
        assert ob.nonedge(K) == (fK, eK)  # the entry point the GPU tier uses at N = 4e4
        # same formula
        assert abs(fK - m["f_series"][K]) <= 1e-12 * max(1.0, abs(fK)), (K, fK, m["f_series"][K])
        assert abs(eK - m["e_series"][K]) <= 1e-12 * max(1.0, abs(eK)), (K, eK, m["e_series"][K])
        # free-energy remainder, both sides
        d = 1e-12 * max(1.0, abs(fK))
        T, x = m["T"][K], m["x"]
        assert T - d <= fK - f_ex <= T / (1.0 - x) + d, (K, fK - f_ex, T, T / (1.0 - x))
        # entropy remainder: an identity
        assert abs((e_ex - eK) - m["e_rem"][K]) <= 1e-12 * max(1.0, abs(eK)), (K, e_ex - eK, m["e_rem"][K])


@pytest.mark.parametrize("beta", [1.0, 0.7])
@pytest.mark.parametrize("Q", [2, 3, 5, 8, 9, 16, 17, 33, 64])
def test_oracle_series_every_order(orc, Q, beta):
    N = 1500 if Q <= 16 else 1200
    og, ob, cab = _instance(orc, N, Q, beta, seed=Q + int(10 * beta))
    _check_orders(og, ob, cab, beta, exact_from_oracle=Q <= 9)


def test_oracle_series_self_loop_and_isolated_vertices(orc):
    og, ob, cab = _instance(orc, 1000, 4, 1.0, seed=11, extra=True)
    deg = og.deg
    assert (deg[-5:] == 0).all() and 7 in og.nbr[og.row_ptr[7]:og.row_ptr[8]]
    _check_orders(og, ob, cab, 1.0, exact_from_oracle=True)


def test_series_order_rule_restatement():
    # the caps, and the boundaries of the moment-tensor sizes (Q + .. + Q^K entries) the engine's k_moments takes
    assert [sm.max_series_order(q) for q in (2, 8, 9, 16, 17, 64)] == [4, 4, 3, 3, 2, 2]
    assert 8 + 8 ** 2 + 8 ** 3 + 8 ** 4 == 4680 and 16 + 16 ** 2 + 16 ** 3 == 4368 and 64 + 64 ** 2 == 4160
    # the one case where the rule picks less than the cap: N = 1e6, Q = 2, c = 3
    from sbm_bp_amd import synth
    cin, cout = synth.cin_cout(2, 3.0, 0.1)
    assert sm.choose_series_order(1_000_000, 2, synth.cab_matrix(2, cin, cout), 1.0) == 3
