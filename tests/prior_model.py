"""TEST INFRASTRUCTURE - one synchronous sweep under a per-vertex prior (include/sbmbp.h sbmbp_set_vertex_prior, DESIGN.md
section 2), restated for the tests. Never imported by the product.

sweep(): assembled from oracle calls only, no arithmetic of its own. Rows are grouped into K classes that share a prior
line of small positive INTEGER weights w_c. For every class the oracle is put on the common start state (set_state; its
sweep rebuilds the field from it), given set_params(cab, na * w_c, beta) - its eta is then exactly eta * w_c, and eta
enters nothing but the row update - and makes one sweep_sync(damp); the class's rows (marginals and out-messages) are
taken from that run and stitched. The reported difference is the maximum over the rows taken.

numpy_sweep(): the same sweep written out in numpy in the log domain (deg_corr_flag 0 and 1), for prior lines the integer
route cannot express (weights like 1e-300). tests/test_prior_cpu.py pins both to the oracle's sweep_sync at weight 1."""
import numpy as np


def classes_of(weights, cls):
    """the dense (N, Q) prior table of class lines weights[K][Q] and the class cls[N] of every row"""
    return np.asarray(weights, dtype=np.float64)[np.asarray(cls, dtype=np.int64)]


def sweep(ob, cab, na, weights, cls, damp=1.0, beta=1.0):
    """one sweep of the oracle `ob` (state set) under the prior classes_of(weights, cls), in place; returns the maximum
    undamped 1-step message difference over the rows taken. Leaves ob with the parameters (cab, na)."""
    weights = np.asarray(weights)
    assert np.issubdtype(weights.dtype, np.integer) and (weights > 0).all()
    cls = np.asarray(cls, dtype=np.int64)
    rp = ob.g.row_ptr.astype(np.int64)
    edge_cls = np.repeat(cls, np.diff(rp))
    psi0, msg0 = ob.get_state()
    psi1, msg1 = psi0.copy(), msg0.copy()
    md = 0.0
    for c in range(len(weights)):
        ob.set_state(psi0, msg0)
        ob.set_field_mix(1.0)  # no sums of an earlier sweep
        ob.set_params(cab, (np.asarray(na, dtype=np.int64) * weights[c].astype(np.int64)).astype(np.uint32), beta)
        ob.sweep_sync(damp)
        p, m = ob.get_state()
        rows, edges = cls == c, edge_cls == c
        psi1[rows] = p[rows]
        msg1[edges] = m[edges]
        if edges.any():
            md = max(md, float(np.abs(m[edges] - msg0[edges]).max()) / damp)  # a damped message moves by damp * (new - old)
    ob.set_params(cab, na, beta)
    ob.set_state(psi1, msg1)
    return md


def numpy_sweep(row_ptr, nbr, rev, psi, msg, cab, na, prior, dc=0, damp=1.0, beta=1.0, clamped=None):
    """(psi', msg', max undamped 1-step difference) of one synchronous sweep from (psi, msg): deg_corr_flag 0 / 1, every
    row product in the log domain (a zero factor is log 0 = -inf and comes back as an exact 0)"""
    assert dc in (0, 1)
    rp = np.asarray(row_ptr, dtype=np.int64)
    N, Q = psi.shape
    deg = np.diff(rp)
    src = np.repeat(np.arange(N), deg)
    g = deg.astype(np.float64) if dc else np.ones(N)
    h = (g[:, None] * psi).sum(0) @ cab  # h[q1] = sum_q2 cab[q2][q1] S[q2]
    W = cab ** beta if dc == 0 else cab
    b = msg[np.asarray(rev, dtype=np.int64)] @ W  # b_e[q] = sum_t W[t][q] m_in[t]
    with np.errstate(divide="ignore"):
        lb = np.log(b)
        lprior = np.log(np.asarray(prior, dtype=np.float64))
    eta = np.asarray(na, dtype=np.float64) / N
    field = (deg[:, None] * h[None, :] if dc else beta * np.broadcast_to(h, (N, Q))) / N
    lA = lprior + np.log(eta)[None, :] - field
    np.add.at(lA, src, lb)
    new_psi = np.exp(lA - lA.max(1, keepdims=True))
    new_psi /= new_psi.sum(1, keepdims=True)
    lc = lA[src] - lb
    cav = np.exp(lc - lc.max(1, keepdims=True))
    cav /= cav.sum(1, keepdims=True)
    md = float(np.abs(cav - msg).max(initial=0.0))
    new_msg = damp * cav + (1.0 - damp) * msg
    if clamped is not None:
        keep = np.asarray(clamped, dtype=bool)
        new_psi[keep] = psi[keep]
        new_msg[keep[src]] = msg[keep[src]]
    return new_psi, new_msg, md
