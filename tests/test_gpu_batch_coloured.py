"""Replica batches in the coloured sweep order (include/sbmbp.h sbmbp_batch_set_sweep_order; csrc/kernels_batch.h
k_sweep_step_batch / k_step_finalize_batch, the step's hub pair per replica): every replica against a single engine in the
same order (the body, the fold order and the update rule are the single engine's, so the comparison is to the bit), against
the test-side definition of the order (tests/coloured_model.py), through switches between the orders with replicas on
different buffers, and through multi-start EM. Every instance has N <= 1000; every test needs the new entry points."""
import functools

import numpy as np
import pytest

import coloured_model as cm
import coloured_step_graph as cg
from conftest import args_of, golden
from test_gpu_batch import batch_from
from test_gpu_coloured import _clamped, _hub_instance
from test_gpu_parity import engine_from, oracle_from

pytestmark = pytest.mark.gpu

# The batch kernel includes the text k_sweep_step includes, the hub kernels and step_update ARE the single engine's, and the
# records are folded in the same order: replica and single engine are compared for equality. (The issue's fallback, should a
# compiler ever contract the two includers differently, is 1e-12, the figure of test_batch_equals_three_single_engines.)
TOL = 0.0


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _diff(x, y):
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    return float(np.abs(x - y).max()) if x.size else 0.0


class _Worst:
    """the largest difference of a case, printed at its end; every reading is asserted against TOL"""

    def __init__(self, label, tol=TOL):
        self.label, self.d, self.tol = label, 0.0, tol

    def __call__(self, x, y, what, tol=None):
        d = _diff(x, y)
        self.d = max(self.d, d)
        assert d <= (self.tol if tol is None else tol), (self.label, what, d)

    def report(self):
        print("%s: largest difference batch / single engine %.3g" % (self.label, self.d))


def _singles(S, a, seeds, scale=None, order=True, fraction=0.0):
    out = []
    for r, s in enumerate(seeds):
        _, _, bp, st = engine_from(S, a, seed=s)
        if scale and r in scale:
            bp.expand_bp_params(S.bp_blockmodel_state(st.cab * scale[r], st.na))
        bp.set_gather_mode(1)
        if order:
            bp.set_sweep_order("coloured", None, fraction)
        out.append(bp)
    return out


def _same_state(w, b, singles, what, field=True):
    for r, bp in enumerate(singles):
        (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
        w(p1, p2, ("marginals", what, r))
        w(m1, m2, ("messages", what, r))
        if field:
            w(b.h(r), bp.h(), ("field", what, r))


# ---------------------------------------------------------------------------------------------------------------------
# 1. every replica equals a single engine in the coloured order
# ---------------------------------------------------------------------------------------------------------------------
EQUAL = ["q4_tight_seed0", "c1_dc1_tight_seed0", "c1_dc2_tight_seed0", "c1_matched_beta08_seed0", "c1_matched_damped_seed0",
         "c1_planted_i1_seed0", "q10_tight_seed1"]


@pytest.mark.parametrize("fraction", [0.0, 1.0], ids=["eighth", "class"])
@pytest.mark.parametrize("name", EQUAL)
def test_every_replica_equals_a_single_engine(S, name, fraction):
    a = args_of(golden(name))
    damp = 0.5 if name == "c1_matched_damped_seed0" else 1.0
    seeds = [a["seed"], a["seed"] + 1, a["seed"] + 2]
    g, b, _ = batch_from(S, a, seeds, {2: 1.1})
    singles = _singles(S, a, seeds, {2: 1.1}, fraction=fraction)
    b.set_sweep_order("coloured", None, fraction)
    assert b.sweep_order == singles[0].sweep_order() and b.sweep_order[0] == 1
    if fraction == 1.0:
        assert b.sweep_order[1] == b.sweep_order[2]  # one step per class
    w = _Worst("%s, step_fraction %g" % (name, fraction))
    for k in range(3):
        d = b.sweep(1, damp)
        for r, bp in enumerate(singles):
            w(d[r], bp.sweep(1, damp), ("difference", k, r))
        _same_state(w, b, singles, k)
    assert all(b.relaxation(r) == (0, -1, 1.0, 1.0) for r in range(3))
    st = b.stats()
    assert st.sweeps == 9 and st.edge_msg_updates == 9 * g.E2 and st.psi_form_sweeps == 0
    w.report()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the model, not only against the sibling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q4_tight_seed0", "c1_dc2_tight_seed0"])
def test_replicas_against_the_model(S, orc, name):
    a = args_of(golden(name))
    seeds = [a["seed"], a["seed"] + 1, a["seed"] + 2]
    g, b, _ = batch_from(S, a, seeds)
    b.set_sweep_order("coloured")
    models = {}
    for r in (0, 2):
        og, ob, _ = oracle_from(orc, dict(a, seed=seeds[r]))
        models[r] = ob
    nc, ns, _, step = cm.plan(og.row_ptr, og.nbr)
    assert b.sweep_order == (1, nc, ns)
    for k in range(3):
        d = b.sweep(1, 1.0)
        for r, ob in models.items():
            d2 = cm.sweep(ob, step, 1.0, _clamped(a))
            psi, msg = b.get_state(r)
            opsi, omsg = ob.get_state()
            assert _diff(psi, opsi) < 1e-11 and _diff(msg, omsg) < 1e-11 and abs(d[r] - d2) < 1e-11, (k, r)  # tests/test_gpu_coloured.py's figure
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows above the segment capacity inside a step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dc", [0, 1])
def test_a_row_above_the_segment_capacity_inside_a_step(S, dc):
    """Q = 9: a segment holds 128 edges, so the row of 140 edges takes the step's fragment pair, launched per replica on
    offset pointers over one shared scratch. Every replica is read back after the launches of ALL replicas ran (replica 1
    after replica 2's), so a wrong offset shows as a foreign or a missing update"""
    Q, N, seeds = 9, 300, (3, 4, 5)
    pairs, cab, na, tc = _hub_instance(Q, N)
    if dc:
        cab = cab / 36.0
    g = S.Graph.from_edges(pairs, N)
    b = S.ReplicaBatch(g, Q, dc, 3)
    b.init_messages(0, None, tc, list(seeds))
    b.set_params(S.bp_blockmodel_state(cab, na))
    b.set_params(S.bp_blockmodel_state(cab * 1.1, na), 1.0, 2)
    assert b.stats().n_hub_rows == 1 and g.max_degree >= 140
    singles = []
    for r, s in enumerate(seeds):
        bp = S.bp_conditional()
        bp.init_messages(S.blockmodel_t(g, Q, dc), 0, None, tc, s)
        bp.expand_bp_params(S.bp_blockmodel_state(cab * (1.1 if r == 2 else 1.0), na))
        bp.set_sweep_order("coloured")
        singles.append(bp)
    b.set_sweep_order("coloured")
    w = _Worst("hub row in a step, dc %d" % dc)
    for k in range(3):
        d = b.sweep(1, 1.0)
        for r in (1, 0, 2):
            w(d[r], singles[r].sweep(1, 1.0), ("difference", k, r))
        _same_state(w, b, singles, k)
    assert _diff(b.get_state(0)[0], b.get_state(1)[0]) > 1e-3  # the replicas are different runs
    w.report()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. steps beyond step 0 and the capacity edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", cg.LAYOUTS)
@pytest.mark.parametrize("Q,dc", [(4, 2), (9, 1)])  # frame_cfg (512, 256) and (128, 64)
def test_later_steps_and_capacity_edges(S, Q, dc, layout):
    """the layouts of tests/coloured_step_graph.py (every boundary block a step of its own behind or before the pool's steps,
    steps cut inside segments, steps of hub rows alone) with the layout's colouring and step fraction, R = 2. The reference is
    the single engine sweeping one call per sweep, which tests/test_gpu_coloured_step.py pins row by row to the model"""
    t = cg.instance(Q, dc, layout)
    g = S.Graph.from_edges(t["pairs"], t["N"])
    seeds = (t["seed"], t["seed"] + 1)
    b = S.ReplicaBatch(g, Q, dc, 2)
    b.init_messages(t["flag"], t["conf"], t["tc"], list(seeds))
    b.set_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    b.set_params(S.bp_blockmodel_state(t["cab"] * 1.1, t["na"]), 1.0, 1)
    b.set_sweep_order("coloured", t["colour"], t["fraction"])
    assert b.sweep_order == (1, t["n_colours"], t["n_steps"])
    singles = []
    for r, s in enumerate(seeds):
        bp = S.bp_conditional()
        bp.init_messages(S.blockmodel_t(g, Q, dc), t["flag"], t["conf"], t["tc"], s)
        bp.expand_bp_params(S.bp_blockmodel_state(t["cab"] * (1.1 if r else 1.0), t["na"]))
        bp.set_sweep_order("coloured", t["colour"], t["fraction"])
        singles.append(bp)
    w = _Worst("steps of layout %s, Q %d dc %d" % (layout, Q, dc))
    for k, damp in enumerate((0.7, 1.0)):
        d = b.sweep(1, damp)
        for r, bp in enumerate(singles):
            w(d[r], bp.sweep(1, damp), ("difference", k, r))
        _same_state(w, b, singles, k)
    w.report()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. replicas stop on their own, in place
# ---------------------------------------------------------------------------------------------------------------------
STOP = dict(name="q10_tight_seed1", seeds=[7, 1, 0], crit=1e-13, limit=2000)  # tests/test_gpu_batch.py test_replicas_stop_on_their_own


@functools.lru_cache(maxsize=None)
def _single_converged(seed):
    """the single engine's coloured converge of the STOP fixture from `seed`: computed once, shared, read-only"""
    import sbm_bp_amd as S
    a = args_of(golden(STOP["name"]))
    _, _, bp, _ = engine_from(S, a, seed=seed)
    bp.set_sweep_order("coloured")
    niter, last = bp.converge(STOP["crit"], STOP["limit"], 1.0)
    psi, msg = bp.get_state()
    for x in (psi, msg):
        x.setflags(write=False)
    return dict(niter=niter, last=last, psi=psi, msg=msg, f=bp.compute_free_energy())


def test_replicas_stop_on_their_own_in_place(S):
    a = args_of(golden(STOP["name"]))
    seeds, crit, limit = STOP["seeds"], STOP["crit"], STOP["limit"]
    ref = [_single_converged(s) for s in seeds]
    print("single engine, coloured: niter for seeds %s: %s" % (seeds, [x["niter"] for x in ref]))
    assert all(x["niter"] >= 0 for x in ref) and len({x["niter"] for x in ref}) >= 2
    g, b, _ = batch_from(S, a, seeds)
    b.set_sweep_order("coloured")
    b.set_schedule(1.0, 1)  # the host reads the states after every sweep
    niter, last = b.converge(crit, limit, 1.0)
    assert list(niter) == [x["niter"] for x in ref] and (last < crit).all(), (niter, last)
    w = _Worst("stopping sweeps")
    for r, x in enumerate(ref):
        w(last[r], x["last"], ("last difference", r))
        psi, msg = b.get_state(r)
        w(psi, x["psi"], ("marginals", r))
        w(msg, x["msg"], ("messages", r))
    w(b.compute_free_energy(), [x["f"] for x in ref], "free energy", 1e-12)
    assert b.stats().sweeps == sum(x["niter"] + 1 for x in ref)
    # The replica that stops first, seen right behind the poll in which it stopped: a second batch, bit for bit the same run,
    # is given exactly the sweeps the early replica needs, so the call returns from that poll. What it holds then must be what
    # the first batch holds for it after the others went on sweeping over the same tables for the rest of the call.
    early = int(np.argmin(niter))
    assert niter[early] < niter.max()
    g2, b2, _ = batch_from(S, a, seeds)
    b2.set_sweep_order("coloured")
    b2.set_schedule(1.0, 1)
    n2, _ = b2.converge(crit, int(niter[early]) + 1, 1.0)
    assert n2[early] == niter[early] and all(n2[r] == -1 for r in range(3) if niter[r] > niter[early])
    for x, y in zip(b2.get_state(early), b.get_state(early)):
        assert np.array_equal(x, y)
    w.report()
    b.close()
    b2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. mixed parities
# ---------------------------------------------------------------------------------------------------------------------
def test_switching_orders_with_replicas_on_different_buffers(S):
    """a synchronous converge ends the replicas after different numbers of sweeps, hence on different buffers of their pairs;
    the coloured sweeps that follow work in place on whichever buffer a replica is on and leave it there; the synchronous
    sweep at the end reads that buffer. Single engines go through the same sequence; every stage at 1e-12, the figure of the
    synchronous batch against single engines (the synchronous kernels of the two are different instantiations)"""
    a = args_of(golden(STOP["name"]))
    seeds, crit, limit = STOP["seeds"], 1e-6, 2000
    g, b, _ = batch_from(S, a, seeds)
    singles = _singles(S, a, seeds, order=False)
    w = _Worst("mixed parities", 1e-12)
    niter, last = b.converge(crit, limit, 1.0)
    executed = [int(n) + 1 if n >= 0 else limit for n in niter]
    print("synchronous converge: executed sweeps %s" % executed)
    assert len({x & 1 for x in executed}) == 2, executed  # the replicas are on different buffers
    for r, bp in enumerate(singles):
        n, l = bp.converge(crit, limit, 1.0)
        assert n == niter[r]
        w(last[r], l, ("synchronous converge", r))
    _same_state(w, b, singles, "after the synchronous converge", field=False)
    b.set_sweep_order("coloured")
    for bp in singles:
        bp.set_sweep_order("coloured")
    for k in range(2):
        d = b.sweep(1, 1.0)
        for r, bp in enumerate(singles):
            w(d[r], bp.sweep(1, 1.0), ("coloured sweep", k, r))
        _same_state(w, b, singles, ("coloured sweep", k))
    b.set_sweep_order("jacobi")
    assert b.sweep_order == (0, 0, 0)
    for bp in singles:
        bp.set_sweep_order("jacobi")
    d = b.sweep(1, 1.0)
    for r, bp in enumerate(singles):
        w(d[r], bp.sweep(1, 1.0), ("synchronous sweep after the coloured ones", r))
    _same_state(w, b, singles, "after the last synchronous sweep", field=False)
    w.report()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. R = 1 equals the single engine
# ---------------------------------------------------------------------------------------------------------------------
def test_one_replica_equals_the_single_engine(S):
    a = args_of(golden("c1_dc1_tight_seed0"))
    g, b, _ = batch_from(S, a, [a["seed"]])
    bp = _singles(S, a, [a["seed"]])[0]
    b.set_sweep_order("coloured")
    w = _Worst("one replica")
    for k, damp in enumerate((0.7, 0.7, 1.0, 1.0)):
        w(b.sweep(1, damp)[0], bp.sweep(1, damp), ("difference", k))
        _same_state(w, b, [bp], k)
    n1, l1 = b.converge(a["crit"], a["tmax"], 1.0)
    n2, l2 = bp.converge(a["crit"], a["tmax"], 1.0)
    assert n1[0] == n2 and n2 >= 0
    w(l1[0], l2, "last difference")
    _same_state(w, b, [bp], "converged")
    w(b.compute_free_energy()[0], bp.compute_free_energy(), "free energy", 1e-12)
    for x, y in zip(b.em_expectations(0), bp.em_expectations()):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    # and the batched reductions of an EM step on the same state
    na, nna, cabe, f, _ = b.em_step()
    for x, y in zip((na[0], nna[0], cabe[0]), bp.em_expectations()):
        assert np.abs(x - y).max() <= 1e-11 * max(1.0, np.abs(y).max())  # tests/test_gpu_batch_learn.py: batched against per-replica
    assert abs(f[0] - bp.compute_free_energy()) <= 1e-11
    w.report()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. reproducible and isolated
# ---------------------------------------------------------------------------------------------------------------------
def test_reproducible_and_isolated(S):
    a = args_of(golden("q4_tight_seed0"))
    seeds = [0, 1, 2]
    out = []
    for _ in range(2):
        g, b, st = batch_from(S, a, seeds)
        b.set_sweep_order("coloured")
        niter, last = b.converge(a["crit"], a["tmax"], 1.0)
        out.append([b.get_state(r) + (b.h(r), niter[r], last[r]) for r in range(3)])
        b.close()
    for x, y in zip(out[0], out[1]):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # replica 1 with other parameters: replicas 0 and 2 do not notice
    g, b, st = batch_from(S, a, seeds)
    b.set_sweep_order("coloured")
    b.set_params(S.bp_blockmodel_state(st.cab * 1.3, st.na), 0.9, 1)
    n2, l2 = b.converge(a["crit"], a["tmax"], 1.0)
    for r in (0, 2):
        assert all(np.array_equal(u, v) for u, v in zip(b.get_state(r) + (b.h(r), n2[r], l2[r]), out[0][r])), r
    assert not np.array_equal(b.get_state(1)[0], out[0][1][0])
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. relaxation
# ---------------------------------------------------------------------------------------------------------------------
def test_no_relaxation_where_the_synchronous_batch_climbs_the_ladder(S):
    a = args_of(golden("hub_dc0_tight_seed0"))
    seeds = [0, 1, 2]
    g, b, _ = batch_from(S, a, seeds)
    b.set_sweep_order("coloured")
    assert all(b.relaxation(r) == (0, -1, 1.0, 1.0) for r in range(3))
    b.converge(a["crit"], 5, 1.0)  # in the middle of the run
    assert all(b.relaxation(r) == (0, -1, 1.0, 1.0) for r in range(3))
    niter, last = b.converge(a["crit"], a["tmax"], 1.0)
    print("coloured batch on the hub graph: niter %s, last %s" % (list(niter), list(last)))
    assert all(b.relaxation(r) == (0, -1, 1.0, 1.0) for r in range(3))
    b.close()
    g, b, _ = batch_from(S, a, seeds)
    b.converge(a["crit"], a["tmax"], 1.0)
    levels = [b.relaxation(r)[:2] for r in range(3)]
    print("synchronous batch on the hub graph: levels", levels)
    assert any(x != (0, -1) for x in levels)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. multi-start EM
# ---------------------------------------------------------------------------------------------------------------------
def test_multi_start_em_in_the_coloured_order(S):
    """q4_learn_seed2 from seeds 0, 2, 3. Seed 2 is the poor start: the synchronous order ends in a saddle at f = -2.5168, the
    coloured order in the reference's basin (-2.716306 on the single engine)"""
    a = args_of(golden("q4_learn_seed2"))
    seeds = (0, 2, 3)
    g = S.load_edge_list(a["path"], a["N"])
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    st = S.bp_param_from_direct(bm, a["pa"], a["cab_upper"])
    b = S.ReplicaBatch(g, a["Q"], a["dc"], len(seeds))
    b.init_messages(a["init_flag"], None, a["true_conf"], list(seeds), conditional=False)
    b.set_params(st, a["beta"])
    b.set_sweep_order("coloured")
    res, eta, cab, best = b.learning(a["lcrit"], a["tmax"], a["lr"], a["damp"])
    print("batch (steps, status, sweeps, f):", [(x.em_steps, x.status, x.total_sweeps, x.free_energy) for x in res], "best", best)
    assert all(b.relaxation(r) == (0, -1, 1.0, 1.0) for r in range(3))
    for r, s in enumerate(seeds):
        bp = S.bp_basic()
        bp.init_messages(bm, a["init_flag"], None, a["true_conf"], s)
        bp.set_beta(a["beta"])
        bp.set_sweep_order("coloured")
        sres = bp.learning(bm, st, a["lcrit"], a["tmax"], a["lr"], a["damp"])
        print("single seed %d (steps, status, sweeps, f):" % s, (sres.em_steps, sres.status, sres.total_sweeps, sres.free_energy))
        scab, sna = bp.get_params()
        bcab, bna, _ = b.get_params(r)
        assert (res[r].status, res[r].em_steps) == (sres.status, sres.em_steps) and list(bna) == list(sna), r
        assert np.abs(bcab - scab).max() <= 1e-9 * np.abs(scab).max() and abs(res[r].free_energy - sres.free_energy) <= 1e-9, r
    assert res[1].free_energy < -2.71, res[1].free_energy
    steps = [x.em_steps for x in res]
    assert len(set(steps)) >= 2, steps  # a replica that has finished sits through the others' rounds frozen
    assert b.stats().sweeps == sum(x.total_sweeps for x in res)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(S):
    a = args_of(golden("q4_tight_seed0"))
    g, b, _ = batch_from(S, a, [0, 1, 2])
    prior = np.ones((a["N"], a["Q"]))
    prior[5] = [1.0, 0.0, 2.0, 1.0]
    # a prior, then the order
    b.set_vertex_prior(prior, 1)
    with pytest.raises(S.SbmbpError) as ei:
        b.set_sweep_order("coloured")
    assert ei.value.code == -6 and "prior" in str(ei.value) and "coloured" in str(ei.value)
    assert b.sweep_order == (0, 0, 0)
    b.set_sweep_order("jacobi")
    assert np.isfinite(b.sweep(1, 1.0)).all()  # usable, the prior still there
    assert b.vertex_prior(1)[0] == 2
    b.set_vertex_prior(None)
    # the order, then a prior: one replica's own and the shared one
    b.set_sweep_order("coloured")
    for replica in (1, -1):
        with pytest.raises(S.SbmbpError) as ei:
            b.set_vertex_prior(prior, replica)
        assert ei.value.code == -6 and "prior" in str(ei.value) and "coloured" in str(ei.value)
    assert b.sweep_order[0] == 1 and all(b.vertex_prior(r)[0] == 0 for r in range(3))
    b.set_vertex_prior(None)  # removing what is not there stays allowed
    assert np.isfinite(b.sweep(1, 1.0)).all()
    # an improper colouring: two adjacent vertices of one colour
    rp, nbr, _ = g.csr()
    bad = S.coloured_plan(g)[2].copy()
    i = next(v for v in range(g.N) if rp[v + 1] > rp[v] and int(nbr[int(rp[v])]) != v)
    bad[i] = bad[int(nbr[int(rp[i])])]
    with pytest.raises(S.SbmbpError) as ei:
        b.set_sweep_order("coloured", bad)
    assert ei.value.code == -1
    with pytest.raises(S.SbmbpError) as ei:
        b.set_sweep_order(2)
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        b.set_sweep_order("coloured", bad[:-1])
    b.set_sweep_order("jacobi")
    assert b.sweep_order == (0, 0, 0) and np.isfinite(b.sweep(1, 1.0)).all()
    b.set_vertex_prior(prior)  # and under order 0 a prior is taken again
    assert np.isfinite(b.sweep(1, 1.0)).all()
    b.close()
