"""CPU tier of the coloured sweep order (include/sbmbp.h sbmbp_set_sweep_order): the host-side plan
of the library against its Python restatement, and the test-side model of a coloured sweep (tests/coloured_model.py,
assembled from oracle calls) tied to the reference's own schedule and to the reference's fixed points. No GPU."""
import numpy as np
import pytest

import coloured_model as cm
from conftest import args_of, best_perm_diff, golden, gpath


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def _multigraph(seed):
    """self-loops, duplicate and reversed pairs, isolated vertices, a long row"""
    rng = np.random.default_rng(400 + seed)
    N = int(rng.choice([1, 2, 9, 60, 333]))
    m = int(N * rng.choice([0.4, 2.0, 6.0]))
    pairs = rng.integers(0, max(1, N - N // 5), size=(m, 2))  # the last fifth of the vertices stays isolated
    if m > 4:
        pairs[: m // 8] = pairs[m // 8: 2 * (m // 8)][: m // 8][:, ::-1]
        pairs[-1] = [pairs[-1, 0], pairs[-1, 0]]
    if N >= 60:
        pairs = np.concatenate([pairs, np.stack([np.zeros(N // 2, dtype=np.int64), np.arange(1, N // 2 + 1)], 1)])
    return N, pairs.astype(np.uint32).reshape(-1, 2)


def _graphs(S):
    yield "c1_dataset", S.load_edge_list(gpath("c1_dataset.edgelist"), 1000)
    yield "hub_n600", S.load_edge_list(gpath("hub_n600.edgelist"), 600)
    yield "q4_n400", S.load_edge_list(gpath("q4_n400.edgelist"), 400)
    for seed in range(12):
        N, pairs = _multigraph(seed)
        yield "random%d" % seed, S.Graph.from_edges(pairs, N)


@pytest.mark.parametrize("step_fraction", [0, 0.125, 0.3, 1, 1e-9])
def test_plan_equals_the_python_restatement(S, step_fraction):
    for name, g in _graphs(S):
        rp, nbr, _ = g.csr()
        nc, ns, col, st = S.coloured_plan(g, None, step_fraction)
        mc, ms, mcol, mst = cm.plan(rp, nbr, None, step_fraction)
        assert (nc, ns) == (mc, ms), name
        assert (col == mcol).all() and (st == mst).all(), name
        assert cm.is_proper(rp, nbr, col.astype(np.int64)), name
        B = max(1, int(np.ceil((step_fraction or 0.125) * g.N)))
        assert np.bincount(st, minlength=ns).max(initial=0) <= B, name           # steps respect B ...
        assert (np.bincount(st, minlength=ns) > 0).all(), name                  # ... none is empty ...
        assert all(len(set(col[st == s])) == 1 for s in range(ns)), name        # ... and none mixes classes
        order = np.lexsort((np.arange(g.N), st))
        assert (np.diff(col[order]) >= 0).all(), name                           # classes in colour order
        if step_fraction == 1:
            assert ns == nc and (st == col).all(), name                         # one step per class
        if step_fraction == 1e-9:
            assert ns == g.N and sorted(st) == list(range(g.N)), name           # one vertex per step


def test_a_callers_colouring_is_validated(S):
    g = S.load_edge_list(gpath("q4_n400.edgelist"), 400)
    rp, nbr, _ = g.csr()
    _, _, col, _ = S.coloured_plan(g)
    mine = (col.astype(np.int64) * 3 + 1) % 397  # another proper colouring (an injective relabelling), with empty classes
    nc, ns, col2, st2 = S.coloured_plan(g, mine, 0.05)
    mc, ms, mcol, mst = cm.plan(rp, nbr, mine, 0.05)
    assert (nc, ns) == (mc, ms) and (col2 == mine).all() and (st2 == mst).all()
    i = int(np.flatnonzero(np.diff(rp.astype(np.int64)) > 0)[0])
    l = int(next(x for x in nbr[int(rp[i]):int(rp[i + 1])] if x != i))
    bad = col.copy()
    bad[i] = bad[l]
    with pytest.raises(S.SbmbpError) as ei:
        S.coloured_plan(g, bad)
    assert ei.value.code == -1 and "improper" in str(ei.value)
    with pytest.raises(S.SbmbpError) as ei:
        S.coloured_plan(g, np.full(400, 400))  # values must be below N
    assert ei.value.code == -1
    with pytest.raises(S.SbmbpError) as ei:
        S.coloured_plan(g, None, -0.5)
    assert ei.value.code == -1
    # a self-loop does not make a colouring improper
    g = S.Graph.from_edges([[0, 0], [0, 1], [1, 2]], 3)
    assert S.coloured_plan(g, [0, 1, 0], 1)[:2] == (2, 2)


def _oracle(orc, a):
    g = orc.Graph.from_edgelist(a["path"], a["N"])
    bp = orc.OracleBP(g, a["Q"], a["dc"])
    bp.init_messages(a["init_flag"], a.get("beliefs"), a["true_conf"], orc.Rng(a["seed"]))
    if "eps" in a:
        cab, na = orc.param_from_epsilon_c(a["N"], a["Q"], a["eps"], a["c"])
    else:
        cab, na = orc.param_from_direct(a["N"], a["Q"], a["pa"], a["cab_upper"])
    bp.set_params(cab, na, a["beta"])
    return g, bp


@pytest.mark.parametrize("name", ["q4_tight_seed0", "c1_dc1_tight_seed0"])
def test_one_vertex_per_step_is_the_sequential_schedule(orc, name):
    """with one vertex per step the model is node_update one vertex at a time in the order of the plan: the reference's
    schedule (bp.cpp:394-401, 1088-1095) with a fixed order, where node_update keeps the field current by itself"""
    a = args_of(golden(name))
    g, m = _oracle(orc, a)
    _, s = _oracle(orc, a)
    _, ns, _, step = cm.plan(g.row_ptr, g.nbr, None, 1e-9)
    assert ns == g.N
    order = np.argsort(step)
    s.init_h()
    for _ in range(3):
        d1, d2 = cm.sweep(m, step), cm.sequential_sweep(s, order)
        assert abs(d1 - d2) < 1e-12
    (p1, m1), (p2, m2) = m.get_state(), s.get_state()
    assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12


def test_model_converges_on_the_hub_graph_without_any_relaxation(orc):
    """plain Jacobi never converges on this instance (test_gpu_parity); the coloured order with the field refreshed every
    1/8 of the vertices does, on one of the three fixed points the reference reaches from its seeds"""
    gs = [golden("hub_dc0_tight_seed%d" % d) for d in (0, 1, 23)]
    a = args_of(gs[0])
    g, ob = _oracle(orc, a)
    _, _, _, step = cm.plan(g.row_ptr, g.nbr)
    niter, last = cm.converge(ob, step, a["crit"], a["tmax"])
    assert 0 <= niter < 400 and last < a["crit"], (niter, last)
    psi = ob.get_state()[0]
    f, _ = ob.free_energy(0)
    hit = [gd for gd in gs if abs(f - gd["result"]["f"]) <= 1e-9 * abs(gd["result"]["f"])]
    assert hit, f
    assert best_perm_diff(psi, np.array(hit[0]["result"]["psi"]).reshape(psi.shape))[0] < 1e-8
