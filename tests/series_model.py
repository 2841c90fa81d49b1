"""Restatement of the non-edge terms (bp.cpp:675-741) in float64 on the host (numpy, torch CPU threads),
pairwise over all ordered (i, l) in row chunks with a BLAS product per chunk, minus the CSR-adjacent pairs. The reference for
tests/test_oracle_series.py (the oracle's moment series) and tests/test_gpu_series.py (the engine's series and its exact tiled kernels).

With y_il = psi_i^T w psi_l / N (w = N (1 - (1 - cab/N)^beta)), yc_il = psi_i^T cab psi_l / N and
u_il = psi_i^T (cab log cab) psi_l / N:

  f_nonedge series(K) = [ -sum_all sum_{k=1..K} y^k / k  -  sum_adj log1p(-y) ] / 2N
  e_nonedge series(K) = [  sum_all sum_{k=0..K-1} u yc^k  -  sum_adj u / (1 - yc) ] / 2N
  f_nonedge exact     = [  sum_nonadj log(psi_i^T P psi_l) ] / 2N,  P = (1 - cab/N)^beta
  e_nonedge exact     = [  sum_nonadj u / (psi_i^T (1 - cab/N) psi_l), where both are non-zero ] / 2N
"""
import math

import numpy as np

# the engine's moment tensors (k_moments): Q + Q^2 + ... + Q^K entries, at most 20 per thread of 256 = 5120, order <= 4
MOMENT_ENTRIES = 5120


def max_series_order(Q):
    """restatement of host_reduce.h max_series_order: 4 up to Q = 8, 3 for Q = 9 .. 16, 2 for Q = 17 .. 64"""
    K, T, sz = 0, 0, 1
    while K < 4:
        sz *= Q
        if T + sz > MOMENT_ENTRIES:
            break
        T += sz
        K += 1
    return K


def series_bound(N, wmax, K):
    """a-priori truncation bound of order K: N (wmax/N)^(K+1) / (2(K+1))"""
    return N * (wmax / N) ** (K + 1) / (2.0 * (K + 1))


def choose_series_order(N, Q, cab, beta):
    """restatement of host_reduce.h series_order for the automatic mode: the smallest K whose bound is below 1e-12,
    else (silently) the cap of the label count. wmax = max over entries of max(w, cab)."""
    Kmax = max_series_order(Q)
    w = nonedge_mats(N, cab, beta)[0]
    wmax = float(max(w.max(), np.asarray(cab).max()))
    for K in range(1, Kmax + 1):
        if series_bound(N, wmax, K) < 1e-12:
            return K
    return Kmax


def nonedge_mats(N, cab, beta):
    cab = np.asarray(cab, dtype=np.float64)
    P = (1.0 - cab / N) ** beta
    w = N * (1.0 - P)
    v = cab * np.log(cab)
    return w, P, v


def _adjacent(psi, row_ptr, nbr):
    src = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr.astype(np.int64)))
    return src, nbr.astype(np.int64)


def pair_terms(psi, cab, beta, row_ptr, nbr, Ks, exact=True, series=True, chunk=1024):
    """the sums of the module docstring, all divided by 2N. Returns a dict:
    f_series[K], e_series[K]          the series of order K, K in Ks (series=True)
    T[K]                              sum_all y^(K+1) / ((K+1) 2N): the leading omitted term of f
    e_rem[K]                          sum_all u yc^K / (1 - yc) / 2N: e_exact - e_series(K), an identity
    x                                 max y over all pairs
    f_exact, e_exact                  (exact=True)
    The pair matrices are symmetric (cab is): each block of rows is taken against the columns from its own first row on, the
    blocks right of the diagonal block twice. Element-wise work runs on torch's CPU threads (float64)."""
    import torch
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    N, Q = psi.shape
    cab = np.asarray(cab, dtype=np.float64)
    assert np.array_equal(cab, cab.T)
    w, P, v = nonedge_mats(N, cab, beta)
    D = 1.0 - cab / N
    Ks = sorted(set(int(k) for k in Ks))
    Kmax = max(Ks) if Ks else 0
    acc = {}

    def add(key, blk_sum):
        acc.setdefault(key, []).append(blk_sum)

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tpsi = t(psi)
    tw, tcab, tv, tP, tD = (t(m) for m in (w, cab, v, P, D))
    x = 0.0
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        p = tpsi[r0:r1]
        cols = tpsi[r0:].T
        wt = torch.ones(N - r0, dtype=torch.float64)
        wt[r1 - r0:] = 2.0  # (i, l) and (l, i)

        def S(m, key):
            add(key, float((m.sum(0) * wt).sum()))

        y = (p @ tw) @ cols / N
        yc = (p @ tcab) @ cols / N
        u = (p @ tv) @ cols / N
        x = max(x, float(y.max()))
        fs = torch.zeros_like(y) if series else None
        es = torch.zeros_like(y) if series else None
        yk = torch.ones_like(y)   # y^k after step k
        yck = torch.ones_like(y)  # yc^(k-1) before the update of step k
        for k in range(1, Kmax + 2):
            if series and k <= Kmax:  # e term k-1: u yc^(k-1)
                es += u * yck
            yk *= y
            if series and k <= Kmax:
                fs += yk / k
            if k - 1 in Ks:  # T(K) = y^(K+1) / (K+1), K = k-1
                S(yk, ("T", k - 1))
            if series and k in Ks:
                S(fs, ("f", k))
                S(es, ("e", k))
            yck *= yc
            if k in Ks:  # yc^K
                S(u * yck / (1.0 - yc), ("r", k))
        if exact:
            S(torch.log((p @ tP) @ cols), "fx")
            den = (p @ tD) @ cols
            ok = (u * den) != 0
            S(torch.where(ok, u / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den)), "ex")
        del y, yc, u, fs, es, yk, yck
    # the adjacent pairs, one per CSR entry
    src, dst = _adjacent(psi, row_ptr, nbr)
    ya = np.einsum("ea,ab,eb->e", psi[src], w, psi[dst]) / N
    yca = np.einsum("ea,ab,eb->e", psi[src], cab, psi[dst]) / N
    ua = np.einsum("ea,ab,eb->e", psi[src], v, psi[dst]) / N
    adj_f = math.fsum(np.log1p(-ya))
    adj_e = math.fsum(ua / (1.0 - yca))
    two_n = 2.0 * N
    tot = lambda key: math.fsum(acc[key])
    out = dict(x=x, f_series={}, e_series={}, T={}, e_rem={})
    for K in Ks:
        if series:
            out["f_series"][K] = (-tot(("f", K)) - adj_f) / two_n
            out["e_series"][K] = (tot(("e", K)) - adj_e) / two_n
        out["T"][K] = tot(("T", K)) / (K + 1) / two_n
        out["e_rem"][K] = tot(("r", K)) / two_n
    if exact:
        za = np.einsum("ea,ab,eb->e", psi[src], P, psi[dst])
        dena = np.einsum("ea,ab,eb->e", psi[src], D, psi[dst])
        oka = (ua * dena) != 0
        out["f_exact"] = (tot("fx") - math.fsum(np.log(za))) / two_n
        out["e_exact"] = (tot("ex") - math.fsum(np.where(oka, ua / np.where(oka, dena, 1.0), 0.0))) / two_n
    return out


def random_marginals(N, Q, seed):
    """Dirichlet rows; every 7th row near one-hot, every 11th with exact zeros in half its columns"""
    rng = np.random.default_rng(seed)
    psi = rng.dirichlet(np.full(Q, 0.7), size=N)
    near = np.arange(0, N, 7)
    hot = rng.integers(0, Q, len(near))
    psi[near] = 1e-6 * rng.random((len(near), Q))
    psi[near, hot] = 1.0
    zr = np.arange(3, N, 11)
    mask = rng.random((len(zr), Q)) < 0.5
    mask[np.arange(len(zr)), rng.integers(0, Q, len(zr))] = False  # at least one column stays
    psi[zr] = np.where(mask, 0.0, psi[zr])
    return psi / psi.sum(1, keepdims=True)
