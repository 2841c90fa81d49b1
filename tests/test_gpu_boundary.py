"""Every kernel family ON the segment, row-length and fragment thresholds: the boundary graphs of tests/boundary_graph.py (a
row of CAP and of CAP + 1 edges, segments of exactly RCAP rows with CAP, RCAP and no edges, rows of 31 / 32 / 33 and 7 / 8 / 9
edges, hub rows of whole fragments and one edge more or less, isolated rows, a hub as first and as last row) against the
oracle, the way tests/test_gpu_label_counts.py, test_gpu_coloured.py, test_gpu_batch*.py and test_gpu_wide.py compare random
graphs. Every case first checks that the engine segments the graph as the model does, so a change of CAP, RCAP or the packing
fails here instead of quietly moving the rows off the thresholds. tests/test_boundary_cpu.py holds the CPU side: the cases
are in the plan, and the oracle is finite and converges on every case run here.
Tolerances are the project's: 1e-11 per sweep and between the engine's own reduction paths, 1e-9 against the oracle's exact
terms and on converged marginals. Each case prints the largest differences it saw."""
import numpy as np
import pytest

import boundary_graph as bg
import coloured_model as cm
from test_gpu_batch import _check_initial

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _rel(a, b):
    """max |a - b| / max(1, max |b|) over the entries where b is finite; a must be finite there"""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    assert np.isfinite(a[fin]).all(), (a, b)
    return float(np.abs(a[fin] - b[fin]).max() / max(1.0, np.abs(b[fin]).max())) if fin.any() else 0.0


class _Seen:
    """the largest differences of one case, printed at its end"""

    def __init__(self, label):
        self.label, self.sweep, self.own, self.oracle = label, 0.0, 0.0, 0.0

    def per_sweep(self, x, what):
        self.sweep = max(self.sweep, float(x))
        assert x < 1e-11, (what, x)

    def own_paths(self, a, b, what):
        d = _rel(a, b)
        self.own = max(self.own, d)
        assert d <= 1e-11, (what, d, a, b)

    def against_oracle(self, a, b, what):
        d = _rel(a, b)
        self.oracle = max(self.oracle, d)
        assert d <= 1e-9, (what, d, a, b)

    def report(self, extra=""):
        print("boundary %s: per sweep %.3g, between the engine's own paths %.3g, against the oracle's exact terms %.3g%s"
              % (self.label, self.sweep, self.own, self.oracle, extra))


def _assert_plan(st, t, hubs=True):
    assert st.n_blocks == t["n_blocks"], (st.n_blocks, t["n_blocks"])
    if hubs:
        assert st.n_hub_rows == len(t["hubs"]) and st.hub_edges == t["hub_edges"], (st.n_hub_rows, st.hub_edges, len(t["hubs"]), t["hub_edges"])


def _engine(S, t, g):
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(g, t["Q"], t["dc"]), t["flag"], t["conf"], t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    return bp


def _compare_state(seen, bp_state, ob, k):
    (psi, msg), (opsi, omsg) = bp_state, ob.get_state()
    seen.per_sweep(np.abs(psi - opsi).max(), "marginals after sweep %d" % k)
    seen.per_sweep(np.abs(msg - omsg).max(), "messages after sweep %d" % k)


def _converge_both(seen, bp, ob, key):
    n1, l1 = bp.converge(1e-10, 600, 1.0)
    n2, l2 = ob.converge_sync(1e-10, 600, 1.0)
    assert n1 == n2, (n1, n2, l1, l2)  # the same sweep
    if key in bg.NOT_CONVERGING:  # (both at the limit: a chaotic trajectory, nothing more to compare)
        assert n1 < 0
        return n1
    assert n1 >= 0 and l1 < 1e-10
    seen.against_oracle(bp.get_state()[0], ob.get_state()[0], "converged marginals")
    return n1


# ---------------------------------------------------------------------------------------------------------------------
# the single engine, Q <= 16: k_sweep / k_sweep_psi, the hub fragment kernels, the frame reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "gather", "clamped"])
@pytest.mark.parametrize("Q,dc", bg.SINGLE)
def test_single_engine_on_the_boundary_graph(S, orc, Q, dc, variant):
    t = bg.instance(Q, dc, clamp=variant == "clamped")
    seen = _Seen("single cap %d Q %d dc %d %s" % (t["cap"], Q, dc, variant))
    g = S.Graph.from_edges(t["pairs"], t["N"])
    og, ob = bg.oracle_of(orc, t, msg_form=variant == "gather")
    assert g.E2 == og.E2 == 2 * len(t["pairs"]) and (og.deg == t["deg"]).all()
    bp = _engine(S, t, g)
    _assert_plan(bp.stats(), t)
    if variant == "gather":
        bp.set_gather_mode(1)
    psi0 = bp.get_state()[0]
    bp.reset_stats()
    for k, damp in enumerate(bg.SINGLE_DAMPS):
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        _compare_state(seen, bp.get_state(), ob, k)
        seen.per_sweep(abs(d1 - d2), "difference of sweep %d" % k)
    # the undamped sweeps run in the marginal-gather form (k_sweep_psi), all but the first; never with deg_corr_flag 2 or
    # when the messages are asked for
    assert bp.stats().psi_form_sweeps == (0 if variant == "gather" or dc == 2 else 2)
    if variant == "clamped":
        rows = bg.clamp_rows(t["cap"], t["rcap"])
        assert len(rows) == 10 and np.array_equal(np.flatnonzero(t["conf"] != -1), rows)
        assert np.array_equal(bp.get_state()[0][rows], psi0[rows])
        assert (psi0[rows, t["tc"][rows]] == 1.0).all()
    niter = _converge_both(seen, bp, ob, ("single", Q, dc, variant))
    if variant == "clamped":
        assert np.array_equal(bp.get_state()[0][rows], psi0[rows])
    # the reductions on the state reached: the fused pass against the separate kernels (message-gather mode) ...
    bp.set_gather_mode(0)
    f, fp = bp.compute_free_energy(parts=True)
    e, ep = bp.compute_entropy(parts=True)
    em = bp.em_expectations()
    bp.set_gather_mode(1)
    f_s, fp_s = bp.compute_free_energy(parts=True)
    e_s, ep_s = bp.compute_entropy(parts=True)
    em_s = bp.em_expectations()
    bp.set_gather_mode(0)
    seen.own_paths(fp, fp_s, "free energy parts, fused / separate")
    for a, b in zip(em, em_s):
        seen.own_paths(a, b, "EM expectations, fused / separate")
    if dc:
        assert np.isnan(e) and np.isnan(e_s)
    else:
        assert np.isfinite(ep).all() and np.isfinite(ep_s).all()
        seen.own_paths(ep, ep_s, "entropy parts, fused / separate")
    # ... and against the oracle's exact terms on the engine's state
    ob.set_state(*bp.get_state())
    ob.compute_h()
    seen.against_oracle(fp, ob.free_energy(0)[1], "free energy parts")
    if dc:
        assert np.isnan(ob.entropy(0)[0])
    else:
        # the reference's site entropy multiplies a row's factors directly and is NaN once a hub row underflows: the finite
        # parts are compared. Its exact non-edge entropy is O(N^2 Q^2) - seconds above Q = 8 -, so only the default variant
        # compares that part there; the others compare the site and edge parts.
        exact = variant == "default" or Q <= 8
        eop = ob.entropy(0 if exact else 2)[1]
        assert np.isfinite(eop[1:]).all()
        seen.against_oracle(ep if exact else ep[:2], eop if exact else eop[:2], "entropy parts")
    for a, b in zip(em, ob.em_expect()):
        seen.against_oracle(a, b, "EM expectations")
    seen.report(", converged at sweep %d" % niter)


# ---------------------------------------------------------------------------------------------------------------------
# the coloured order: k_sweep_step / k_hub_step_cavity over class 0 = every structured row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", bg.COLOURED)
def test_coloured_order_with_the_structured_rows_in_one_class(S, orc, Q, dc):
    t = bg.instance(Q, dc)
    seen = _Seen("coloured cap %d Q %d dc %d" % (t["cap"], Q, dc))
    g = S.Graph.from_edges(t["pairs"], t["N"])
    og, ob = bg.oracle_of(orc, t)
    bp = _engine(S, t, g)
    _assert_plan(bp.stats(), t)
    colour = bg.structured_colouring(t, og.row_ptr, og.nbr)
    bp.set_sweep_order("coloured", colour, 1.0)
    nc, ns, _, step = cm.plan(og.row_ptr, og.nbr, colour, 1.0)
    assert bp.sweep_order() == (1, nc, ns) and ns == nc  # one step per class: step 0 holds the structured degree sequence
    assert (step[:t["ns"]] == 0).all() and (t["deg"][step == 0][:t["ns"]] == bg.boundary_degrees(t["cap"], t["rcap"])).all()
    gi = t["deg"].astype(float) if dc else np.ones(t["N"])
    for k in range(3):
        d1, d2 = bp.sweep(1, 1.0), cm.sweep(ob, step, 1.0)
        _compare_state(seen, bp.get_state(), ob, k)
        seen.per_sweep(abs(d1 - d2), "difference of sweep %d" % k)
        h, href = bp.h(), bp.get_params()[0].T @ (gi[:, None] * bp.get_state(True, False)[0]).sum(0)  # the field moved step by step
        assert np.abs(h - href).max() <= 1e-12 * max(1.0, np.abs(href).max()), (k, h, href)
    assert bp.stats().psi_form_sweeps == 0
    seen.report()


# ---------------------------------------------------------------------------------------------------------------------
# the replica batch at every label count it is compiled for
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", bg.BATCH)
def test_replica_batch_at_every_label_count(S, orc, Q, dc):
    t = bg.instance(Q, dc)
    seen = _Seen("batch cap %d Q %d dc %d" % (t["cap"], Q, dc))
    g = S.Graph.from_edges(t["pairs"], t["N"])
    params, seeds = bg.three_params(t), list(bg.BATCH_SEEDS)
    oracles = [bg.oracle_of(orc, t, True, seeds[r], cab, na)[1] for r, (cab, na) in enumerate(params)]

    def make():
        b = S.ReplicaBatch(g, Q, dc, 3)
        b.init_messages(0, None, t["tc"], seeds, conditional=True)
        for r, (cab, na) in enumerate(params):
            b.set_params(S.bp_blockmodel_state(cab, na), 1.0, r)
        b.set_nonedge_mode(1, 0)  # exact
        return b

    # two batches in the same states (the sweeps are reproducible bit for bit): the per-replica reductions run on the second
    b, b2 = make(), make()
    _assert_plan(b.stats(), t)
    for r, ob in enumerate(oracles):
        _check_initial(S, b, r, ob)  # the 2 Q 2^-53 rule for the restored message component
    for k, damp in enumerate(bg.BATCH_DAMPS):
        d = b.sweep(1, damp)
        b2.sweep(1, damp)
        for r, ob in enumerate(oracles):
            do = ob.sweep_sync(damp)
            _compare_state(seen, b.get_state(r), ob, k)
            seen.per_sweep(abs(d[r] - do), "difference of sweep %d, replica %d" % (k, r))
    st = b.stats()
    assert st.sweeps == 3 * len(bg.BATCH_DAMPS) and st.edge_msg_updates == st.sweeps * g.E2 and st.psi_form_sweeps == 0
    # one EM step on the states reached, and on those of a second pair of batches whose field is relaxed (as
    # tests/test_gpu_batch_learn.py: the field is stale after the sweeps, so k_field_refresh_batch runs first)
    c, c2 = make(), make()
    for x in (c, c2):
        x.set_schedule(field_mix=0.5)
        assert (x.sweep(3, 1.0) > 1e-6).all()  # not converged
    for x, x2 in ((b, b2), (c, c2)):
        assert all(np.array_equal(u, v) for r in range(3) for u, v in zip(x.get_state(r), x2.get_state(r)))
        na_b, nna_b, cab_b, f_b, parts_b = x.em_step()
        f_r, parts_r = x2.compute_free_energy(parts=True)
        for r in range(3):
            for a, y in zip((na_b[r], nna_b[r], cab_b[r]), x2.em_expectations(r)):
                seen.own_paths(a, y, "em_step / per-replica EM expectations, replica %d" % r)
        seen.own_paths(parts_b, parts_r, "em_step / per-replica free energy parts")
        seen.own_paths(f_b, f_r, "em_step / per-replica free energy")
        again = x.em_step()
        assert all(np.array_equal(u, v) for u, v in zip((na_b, nna_b, cab_b, f_b, parts_b), again))  # fixed summation order
        for r, ob in enumerate(oracles):
            ob.set_state(*x.get_state(r))
            ob.compute_h()
            for a, y in zip((na_b[r], nna_b[r], cab_b[r]), ob.em_expect()):
                seen.against_oracle(a, y, "EM expectations, replica %d" % r)
            fo, oparts = ob.free_energy(0)
            seen.against_oracle(parts_b[r], oparts, "free energy parts, replica %d" % r)
            seen.against_oracle(f_b[r], fo, "free energy, replica %d" % r)
    c.close()
    c2.close()
    b.close()
    b2.close()
    seen.report()


# ---------------------------------------------------------------------------------------------------------------------
# label counts above 16: the matrix-core kernels on the (64, 16) graph, whole and partial last trips of k_wem
# ---------------------------------------------------------------------------------------------------------------------
def _wide_pair(S, orc, t, whole=False):
    g = S.Graph.from_edges(t["pairs"], t["N"])
    og, ob = bg.oracle_of(orc, t, msg_form=True)  # the wide path reports 1-step differences on every sweep
    bp = _engine(S, t, g)
    _assert_plan(bp.stats(), t, hubs=False)  # (above Q = 16 a long row is walked inside the sweep kernel: no fragment tables)
    assert (g.E2 % 64 == 0) == whole
    return g, bp, ob


@pytest.mark.parametrize("Q,dc,whole", bg.WIDE)
def test_wide_kernels_on_the_boundary_graph(S, orc, Q, dc, whole):
    t = bg.instance(Q, dc, whole_trips=whole)
    assert (t["cap"], t["rcap"]) == (64, 16)
    seen = _Seen("wide cap 64 Q %d dc %d %s" % (Q, dc, "whole trips" if whole else "partial last trip"))
    g, bp, ob = _wide_pair(S, orc, t, whole)
    psi0, msg0 = bp.get_state()
    opsi0, omsg0 = ob.get_state()
    assert np.array_equal(psi0, opsi0) and np.array_equal(msg0, omsg0)
    for k, damp in enumerate(bg.WIDE_DAMPS):
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        _compare_state(seen, bp.get_state(), ob, k)
        seen.per_sweep(abs(d1 - d2), "difference of sweep %d" % k)
    seen.per_sweep(abs(bp.compute_overlap() - ob.overlap()), "overlap")
    ob.compute_h()
    f, fp = bp.compute_free_energy(parts=True)
    # the oracle's exact non-edge term is O(N^2 Q^2) without degree correction: 3.5 s at Q = 64, so there the site and edge
    # parts are compared
    if dc or Q <= 33:
        seen.against_oracle(fp, ob.free_energy(0)[1], "free energy parts")
    else:
        seen.against_oracle(fp[:2], ob.free_energy(2)[1][:2], "free energy parts (site, edge)")
    e, ep = bp.compute_entropy(parts=True)
    if dc:
        assert np.isnan(e) and np.isnan(ob.entropy(0)[0])
    elif Q == 17:  # the exact entropy of the oracle takes 13 s at Q = 33 and 50 s at Q = 64
        assert np.isfinite(ep).all()
        seen.against_oracle(ep, ob.entropy(0)[1], "entropy parts")
    else:
        assert np.isfinite(ep).all()
    for a, x in zip(bp.em_expectations(), ob.em_expect()):  # the numerators: a labels x labels product over the edges (k_wem)
        seen.against_oracle(a, x, "EM expectations")
    niter = _converge_both(seen, bp, ob, ("wide", Q, dc, whole))
    assert bp.stats().psi_form_sweeps == 0
    seen.report(", converged at sweep %d" % niter)


def test_wide_clamped_rows_on_the_boundary_graph(S, orc):
    t = bg.instance(bg.WIDE_CLAMPED_Q, 0, clamp=True)
    seen = _Seen("wide cap 64 Q %d dc 0 clamped" % t["Q"])
    g, bp, ob = _wide_pair(S, orc, t)
    rows = bg.clamp_rows(64, 16)
    psi0 = bp.get_state()[0]
    for k, damp in enumerate(bg.WIDE_DAMPS):
        d1, d2 = bp.sweep(1, damp), ob.sweep_sync(damp)
        _compare_state(seen, bp.get_state(), ob, k)
        seen.per_sweep(abs(d1 - d2), "difference of sweep %d" % k)
    assert np.array_equal(bp.get_state()[0][rows], psi0[rows]) and (psi0[rows, t["tc"][rows]] == 1.0).all()
    ob.compute_h()
    seen.against_oracle(bp.compute_free_energy(parts=True)[1], ob.free_energy(0)[1], "free energy parts")
    for a, x in zip(bp.em_expectations(), ob.em_expect()):
        seen.against_oracle(a, x, "EM expectations")
    niter = _converge_both(seen, bp, ob, ("wide", t["Q"], 0, "clamped"))
    assert np.array_equal(bp.get_state()[0][rows], psi0[rows])
    seen.report(", converged at sweep %d" % niter)
