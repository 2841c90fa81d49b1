"""Per-vertex priors of replica batches (include/sbmbp.h sbmbp_batch_set_vertex_prior; csrc/kernels_batch.h
k_sweep_batch_prior / k_em_frame_batch_prior, the hub kernels on a replica's table) on the GPU. The yardstick throughout is the
single engine under set_vertex_prior, which tests/test_gpu_prior.py pins to the oracle model at 1e-11 at every Q: a replica
that reads a table goes through the single engine's states with that table bit for bit, a replica without one (while another
holds one) through those of a single engine with a table of ones. Reductions: the 1e-11 of tests/test_gpu_batch_learn.py;
uniform tables: the 1e-13 / 1e-12 of test_uniform_prior_is_no_prior; learning: the bounds of
test_every_replica_learns_as_a_single_engine_does. Every case prints the largest differences it saw before it asserts."""
import ctypes as C

import numpy as np
import pytest

import boundary_graph as bg
import prior_model as pm
from conftest import args_of, golden, gpath

pytestmark = pytest.mark.gpu

DAMPS = (0.7, 1.0, 1.0)


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


_CASES = {}


def case(Q, dc):
    """tests/test_gpu_prior.py::case: the boundary graph of this Q's (CAP, RCAP) plus one more last row, a hub of 2 * 256 + 1
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
    """tests/test_gpu_prior.py::three_classes: the hub of CAP + 1 edges, the hub of 2 * 256 + 1 edges and an isolated vertex in
    three different classes, the other rows round-robin"""
    rng = np.random.default_rng(900 + Q)
    weights = rng.integers(1, 5, size=(3, Q)).astype(np.int64)
    weights[np.arange(3), np.arange(3) % Q] += 2
    cls = np.arange(t["N"]) % 3
    cls[0], cls[t["N"] - 1], cls[t["isolated"]] = 0, 1, 2
    return weights, cls


def tables(t, Q):
    """[shared, own, ones]: the three_classes table; a table of other weights with a zero entry on one ordinary row and on one
    hub row; what a replica without a table reads"""
    weights, cls = three_classes(t, Q)
    shared = pm.classes_of(weights, cls)
    other = np.random.default_rng(1700 + Q).integers(1, 7, size=(3, Q)).astype(np.float64)
    own = pm.classes_of(other, (cls + 1) % 3).copy()
    hubs = set(int(h) for h in t["hubs"])
    ordinary = next(i for i in range(1, t["N"]) if i not in hubs and 3 <= t["deg"][i] <= 30)
    own[ordinary, 0] = 0.0
    own[t["N"] - 1, 1] = 0.0  # the hub of three fragments
    assert (own.max(1) > 0).all()
    return [shared, own, np.ones_like(shared)], ordinary


def single(S, t, g, table, seed=None):
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, t["Q"], t["dc"]), 0, None, t["tc"], t["seed"] if seed is None else seed)
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    if table is not None:
        bp.set_vertex_prior(table)
    return bp


def mixed_batch(S, t, g, tabs):
    """R = 3 from ONE seed: replica 0 shared, replica 1 own, replica 2 none"""
    b = S.ReplicaBatch(g, t["Q"], t["dc"], 3)
    b.init_messages(0, None, t["tc"], [t["seed"]] * 3)
    b.set_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    b.set_vertex_prior(tabs[0])
    b.set_vertex_prior(tabs[1], 1)
    b.set_vertex_prior(None, 2)
    assert [b.vertex_prior(r)[0] for r in range(3)] == [1, 2, 0]
    return b


def swept(S, Q, dc, check=False):
    """the mixed batch and its three single engines after the three sweeps; check: bit equality after every sweep"""
    t = case(Q, dc)
    g = S.Graph.from_edges(t["pairs"], t["N"])
    tabs, ordinary = tables(t, Q)
    b = mixed_batch(S, t, g, tabs)
    singles = [single(S, t, g, tab) for tab in tabs]
    assert b.stats().n_hub_rows == len(t["hubs"]) and len(t["hubs"]) >= 6
    for r, bp in enumerate(singles):
        assert all(np.array_equal(x, y) for x, y in zip(b.get_state(r), bp.get_state()))
    worst = 0.0
    for k, damp in enumerate(DAMPS):
        d = b.sweep(1, damp)
        for r, bp in enumerate(singles):
            ds = bp.sweep(1, damp)
            if not check:
                continue
            (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
            assert np.isfinite(p1).all() and np.isfinite(m1).all()
            seen = max(np.abs(p1 - p2).max(), np.abs(m1 - m2).max(), abs(d[r] - ds))
            worst = max(worst, seen)
            print("batch prior Q %d dc %d sweep %d replica %d: max difference %.3g" % (Q, dc, k, r, seen))
            assert np.array_equal(p1, p2) and np.array_equal(m1, m2) and d[r] == ds, (k, r, seen)
    return t, g, tabs, ordinary, b, singles, worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. every instantiation, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(Q, dc) for Q in range(2, 17) for dc in (0, 1)] + [(Q, 2) for Q in (2, 8, 16)])
def test_every_instantiation_equals_three_single_engines(S, Q, dc):
    t, g, tabs, ordinary, b, singles, worst = swept(S, Q, dc, check=True)
    psi, msg = b.get_state(1)
    rp = g.csr()[0].astype(np.int64)
    # a zero forbids the label exactly: in the marginal and in every message the row sends
    assert (psi[ordinary, 0] == 0.0) and (msg[rp[ordinary]:rp[ordinary + 1], 0] == 0.0).all()
    assert (psi[t["N"] - 1, 1] == 0.0) and (msg[rp[t["N"] - 1]:rp[t["N"]], 1] == 0.0).all()
    st = b.stats()
    assert st.psi_form_sweeps == 0 and st.sweeps == 9
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. replicas stop on their own under a prior
# ---------------------------------------------------------------------------------------------------------------------
def c1_instance(S):
    N, Q = 1000, 2
    tc = np.repeat(np.arange(Q, dtype=np.uint32), N // Q)
    g = S.load_edge_list(gpath("c1_dataset.edgelist"), N)
    bm = S.blockmodel_t(g, Q, 0)
    st = S.bp_param_from_epsilon_c(bm, 0.1, 3.0)
    table = np.ones((N, Q))
    table[[3, 40, 77, 130, 499], 0] = 4.0      # five vertices of group 0 ...
    table[[500, 612, 733, 850, 999], 1] = 4.0  # ... and five of group 1, "probably" in their groups
    return N, Q, tc, g, bm, st, table


def test_replicas_stop_on_their_own_under_a_prior(S):
    N, Q, tc, g, bm, st, table = c1_instance(S)
    seeds = [0, 1, 2]
    b = S.ReplicaBatch(g, Q, 0, 3)
    b.init_messages(0, None, tc, seeds)
    b.set_params(st)
    b.set_vertex_prior(table)
    niter, last = b.converge(5e-6, 500, 1.0)
    print("batch niter under a shared prior:", list(niter), "last:", list(last))
    for r, s in enumerate(seeds):
        bp = S.bp_conditional()
        bp.init_messages(bm, 0, None, tc, s)
        bp.expand_bp_params(st)
        bp.set_vertex_prior(table)
        n1, l1 = bp.converge(5e-6, 500, 1.0)
        (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
        print("replica %d: niter %d / %d, state difference %.3g" % (r, niter[r], n1, max(np.abs(p1 - p2).max(), np.abs(m1 - m2).max())))
        assert niter[r] == n1 and n1 >= 0 and last[r] == l1
        assert np.array_equal(p1, p2) and np.array_equal(m1, m2), r
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. reductions
# ---------------------------------------------------------------------------------------------------------------------
def close(what, x, y, tol):
    x, y = np.asarray(x), np.asarray(y)
    d = np.abs(x - y) / np.maximum(1.0, np.abs(y))
    print("%s: max rel diff %.3g (tol %g)" % (what, d.max(), tol))
    return bool((d <= tol).all())


@pytest.mark.parametrize("Q,dc", [(4, 0), (8, 1), (9, 0)])
def test_reductions_under_priors(S, Q, dc):
    t, g, tabs, ordinary, b, singles, _ = swept(S, Q, dc)
    na_b, nna_b, cab_b, f_b, parts_b = b.em_step()
    again = b.em_step()
    assert all(np.array_equal(x, y) for x, y in zip((na_b, nna_b, cab_b, f_b, parts_b), again))
    f_r, parts_r = b.compute_free_energy(parts=True)
    assert close("em_step parts / per replica", parts_b, parts_r, 1e-11) and close("em_step f / per replica", f_b, f_r, 1e-11)
    ent = b.compute_entropy(parts=True) if dc == 0 else None
    for r, bp in enumerate(singles):
        na_r, nna_r, cab_r = b.em_expectations(r)
        tag = "Q %d dc %d replica %d " % (Q, dc, r)
        assert close(tag + "na", na_b[r], na_r, 1e-11) and close(tag + "nna", nna_b[r], nna_r, 1e-11) and close(tag + "cab", cab_b[r], cab_r, 1e-11)
        na_s, nna_s, cab_s = bp.em_expectations()
        f_s, parts_s = bp.compute_free_energy(parts=True)
        assert close(tag + "na / single", na_r, na_s, 1e-11) and close(tag + "nna / single", nna_r, nna_s, 1e-11)
        assert close(tag + "cab / single", cab_r, cab_s, 1e-11)
        assert close(tag + "parts / single", parts_r[r], parts_s, 1e-11) and close(tag + "f / single", f_r[r], f_s, 1e-11)
        if dc == 0:
            e_s, eparts_s = bp.compute_entropy(parts=True)
            assert np.isfinite(eparts_s).all()
            assert close(tag + "entropy parts / single", ent[1][r], eparts_s, 1e-11) and close(tag + "entropy / single", ent[0][r], e_s, 1e-11)
    # the tables are in the site term: the three replicas started from ONE state and differ in nothing else
    assert len({float(x) for x in parts_b[:, 0]}) == 3
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a uniform table is no table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", [(3, 0), (5, 1)])
def test_uniform_table_is_no_table(S, Q, dc):
    t = case(Q, dc)
    g = S.Graph.from_edges(t["pairs"], t["N"])
    c = np.random.default_rng(3).uniform(0.25, 4.0, size=t["N"])
    both = []
    for with_table in (False, True):
        b = S.ReplicaBatch(g, Q, dc, 2)
        b.init_messages(0, None, t["tc"], [t["seed"], t["seed"] + 1])
        b.set_params(S.bp_blockmodel_state(t["cab"], t["na"]))
        if with_table:
            b.set_vertex_prior(np.repeat(c[:, None], Q, 1))
        both.append(b)
    plain, b = both
    assert b.stats().bytes_per_sweep == plain.stats().bytes_per_sweep + 8.0 * Q * t["N"]
    for damp in DAMPS:
        d1, d2 = b.sweep(1, damp), plain.sweep(1, damp)
        assert np.abs(d1 - d2).max() <= 1e-13
    seen = max(np.abs(x - y).max() for r in range(2) for x, y in zip(b.get_state(r), plain.get_state(r)))
    print("uniform table Q %d dc %d: states %.3g" % (Q, dc, seen))
    assert seen <= 1e-13, seen
    for r in range(2):
        plain.set_state(r, *b.get_state(r))  # the reductions on ONE state
    shift = float(np.log(c).sum()) / t["N"]
    for what, (f1, p1), (f2, p2) in (("per replica", b.compute_free_energy(parts=True), plain.compute_free_energy(parts=True)),
                                     ("em_step", b.em_step()[3:], plain.em_step()[3:])):
        print("uniform table %s: f_site shift off by %.3g, other parts %.3g" % (what, np.abs((p1[:, 0] - p2[:, 0]) - shift).max(), np.abs(p1[:, 1:] - p2[:, 1:]).max()))
        assert np.abs((p1[:, 0] - p2[:, 0]) - shift).max() <= 1e-12 and np.abs(p1[:, 1:] - p2[:, 1:]).max() <= 1e-12, (what, p1, p2, shift)
        assert np.abs((f1 - f2) + shift).max() <= 1e-12
    b.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. learning with the priors held fixed
# ---------------------------------------------------------------------------------------------------------------------
def test_every_replica_learns_under_a_prior_as_a_single_engine_does(S):
    a = args_of(golden("c1_learn_515_seed0"))
    seeds = [0, 3, 4]
    table = c1_instance(S)[6]
    g = S.load_edge_list(a["path"], a["N"])
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    st = S.bp_param_from_direct(bm, a["pa"], a["cab_upper"])
    b = S.ReplicaBatch(g, a["Q"], a["dc"], len(seeds))
    b.init_messages(a["init_flag"], None, a["true_conf"], seeds, conditional=False)
    b.set_params(st, a["beta"])
    b.set_vertex_prior(table)
    res, eta, cab, best = b.learning(1e-6, 20, 0.2, 1.0)
    print("batch (steps, status, sweeps, f, overlap):", [(x.em_steps, x.status, x.total_sweeps, x.free_energy, x.overlap) for x in res], "best", best)
    for r, s in enumerate(seeds):
        bp = S.bp_basic()
        bp.init_messages(bm, a["init_flag"], None, a["true_conf"], s)
        bp.set_beta(a["beta"])
        bp.set_gather_mode(1)
        bp.set_vertex_prior(table)
        sres = bp.learning(bm, st, 1e-6, 20, 0.2, 1.0)
        scab, sna = bp.get_params()
        bcab, bna, _ = b.get_params(r)
        print("single seed %d (steps, status, sweeps, f, overlap):" % s, (sres.em_steps, sres.status, sres.total_sweeps, sres.free_energy, sres.overlap),
              "cab diff %.3g" % (np.abs(bcab - scab).max() / np.abs(scab).max()))
        assert (res[r].em_steps, res[r].status, res[r].total_sweeps) == (sres.em_steps, sres.status, sres.total_sweeps), r
        assert list(bna) == list(sna)
        assert np.abs(bcab - scab).max() <= 1e-9 * np.abs(scab).max()
        assert abs(res[r].free_energy - sres.free_energy) <= 1e-9 and abs(res[r].overlap - sres.overlap) <= 1e-9
    assert b.vertex_prior(1)[0] == 1 and np.array_equal(b.vertex_prior(1)[1], table)  # held fixed
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. life cycle
# ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle(S):
    N, Q, tc, g, bm, st, T1 = c1_instance(S)
    rng = np.random.default_rng(11)
    T2, T3 = rng.uniform(0.5, 2.0, size=(N, Q)), rng.uniform(0.5, 2.0, size=(N, Q))
    seeds = [5, 6, 7]
    tab = N * Q * 8

    def fresh(R=3):
        b = S.ReplicaBatch(g, Q, 0, R)
        b.init_messages(0, None, tc, seeds[:R])
        b.set_params(st)
        return b

    b, plain = fresh(), fresh()
    bytes0, dev0 = b.stats().bytes_per_sweep, b.stats().device_bytes
    assert [b.vertex_prior(r) for r in range(3)] == [(0, None)] * 3
    # shared: ONE table whatever R is
    b.set_vertex_prior(T1)
    assert all(b.vertex_prior(r)[0] == 1 and np.array_equal(b.vertex_prior(r)[1], T1) for r in range(3))
    assert b.stats().device_bytes == dev0 + tab and b.stats().bytes_per_sweep == bytes0 + 8.0 * Q * N
    one = fresh(1)
    d1 = one.stats().device_bytes
    one.set_vertex_prior(T1)
    assert one.stats().device_bytes == d1 + tab
    one.close()
    # own for replica 1: one more table
    b.set_vertex_prior(T2, 1)
    assert [b.vertex_prior(r)[0] for r in range(3)] == [1, 2, 1]
    assert np.array_equal(b.vertex_prior(1)[1], T2) and np.array_equal(b.vertex_prior(0)[1], T1)
    assert b.stats().device_bytes == dev0 + 2 * tab
    # the tables survive init_messages, set_params and set_state
    b.init_messages(0, None, tc, seeds)
    b.set_params(st)
    b.set_state(2, *plain.get_state(2))
    assert [b.vertex_prior(r)[0] for r in range(3)] == [1, 2, 1] and np.array_equal(b.vertex_prior(1)[1], T2)
    # (-1, T3): all shared with T3, the own table freed
    b.set_vertex_prior(T3)
    assert all(b.vertex_prior(r)[0] == 1 and np.array_equal(b.vertex_prior(r)[1], T3) for r in range(3))
    assert b.stats().device_bytes == dev0 + tab
    # (r, None): none for r; it now reads the batch's table of ones (one more table on the device)
    b.set_vertex_prior(None, 0)
    assert [b.vertex_prior(r)[0] for r in range(3)] == [0, 1, 1] and b.vertex_prior(0)[1] is None
    assert b.stats().device_bytes == dev0 + 2 * tab and b.stats().bytes_per_sweep == bytes0 + 8.0 * Q * N
    # bad rows and bad replica indices: -1, the vertex (and the replica) named, nothing changes
    lib = S.load_library()
    for value, word in ((-1.0, "negative"), (float("nan"), "NaN"), (float("inf"), "Inf")):
        bad = T1.copy()
        bad[17, 1] = value
        with pytest.raises(S.SbmbpError) as ei:
            b.set_vertex_prior(bad, 2)
        assert ei.value.code == -1 and "vertex 17" in str(ei.value) and "replica 2" in str(ei.value) and word in str(ei.value)
    bad = T1.copy()
    bad[23] = 0.0
    with pytest.raises(S.SbmbpError) as ei:
        b.set_vertex_prior(bad)
    assert ei.value.code == -1 and "vertex 23" in str(ei.value) and "replica" not in str(ei.value).split("vertex 23")[1]
    for r in (3, -2):
        with pytest.raises(S.SbmbpError) as ei:
            b.set_vertex_prior(T1, r)
        assert ei.value.code == -1 and "replica index" in str(ei.value)
    present = C.c_int(9)
    assert lib.sbmbp_batch_get_vertex_prior(b._h, 3, None, C.byref(present)) == -1 and present.value == 9
    with pytest.raises(ValueError):
        b.set_vertex_prior(T1[:-1])
    assert [b.vertex_prior(r)[0] for r in range(3)] == [0, 1, 1] and np.array_equal(b.vertex_prior(2)[1], T3)
    assert b.stats().device_bytes == dev0 + 2 * tab
    # (-1, None): the no-prior batch again, bit for bit, with its bytes
    b.sweep(2, 1.0)  # (under the tables: the state moves away from the plain batch's)
    b.set_vertex_prior(None)
    assert [b.vertex_prior(r) for r in range(3)] == [(0, None)] * 3
    assert b.stats().device_bytes == dev0 and b.stats().bytes_per_sweep == bytes0
    b.init_messages(0, None, tc, seeds)
    b.set_params(st)
    for damp in DAMPS:
        d1, d2 = b.sweep(1, damp), plain.sweep(1, damp)
        assert np.array_equal(d1, d2)
        assert all(np.array_equal(x, y) for r in range(3) for x, y in zip(b.get_state(r), plain.get_state(r)))
    n1, n2 = b.converge(5e-6, 500, 1.0), plain.converge(5e-6, 500, 1.0)
    assert np.array_equal(n1[0], n2[0]) and all(np.array_equal(x, y) for r in range(3) for x, y in zip(b.get_state(r), plain.get_state(r)))
    assert np.array_equal(b.em_step()[4], plain.em_step()[4])
    b.close()
    plain.close()
