"""The coloured order beyond step 0: k_sweep_step, k_hub_step_cavity, the step form of k_hub_frag_product_msg and
k_step_finalize on the layouts of tests/coloured_step_graph.py - every block of the boundary graphs a step of its own behind
(or before) the pool's steps, steps cut inside segments, steps of hubs alone first and last, a step of 256 and of 257 records -
against the test-side definition of the order (tests/coloured_model.py). tests/test_coloured_step_cpu.py holds the CPU side:
where every condition shows, the step tables against the model, and that the model is finite (and converges) on every case
run here.
Every case first checks that the engine segments the graph as the model does and plans the colours and steps of the model.
Sweeps run one call each AND queued in one call: the field sums are recomputed at the start of a call and moved by
differences inside it, so only the second sweep of a call reads a field that has moved through a whole sweep.
Tolerances are the project's: 1e-11 per sweep, 1e-12 relative on the field, 1e-9 on converged marginals. Each case prints the
largest differences it saw."""
import numpy as np
import pytest

import boundary_graph as bg
import coloured_model as cm
import coloured_step_graph as cg
from test_gpu_boundary import _Seen, _assert_plan, _compare_state, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _pair(S, orc, t):
    """(graph, engine in the coloured order of the layout, oracle); the plan of both asserted against the models"""
    g = S.Graph.from_edges(t["pairs"], t["N"])
    og, ob = bg.oracle_of(orc, t)
    assert g.E2 == og.E2 == 2 * len(t["pairs"]) and np.array_equal(og.row_ptr, t["row_ptr"]) and np.array_equal(og.nbr, t["nbr"])
    bp = _engine(S, t, g)
    _assert_plan(bp.stats(), t)
    bp.set_sweep_order("coloured", t["colour"], t["fraction"])
    nc, ns, _, step = cm.plan(og.row_ptr, og.nbr, t["colour"], t["fraction"])
    assert bp.sweep_order() == (1, nc, ns) and (nc, ns) == (t["n_colours"], t["n_steps"]) and np.array_equal(step, t["step"])
    return g, bp, ob


def _field(seen, bp, t, what):
    """h() - moved step by step inside a call - against a fresh cab^T sum_i g_i psi_i of the engine's own marginals"""
    gi = t["deg"].astype(float) if t["dc"] else np.ones(t["N"])
    h, href = bp.h(), bp.get_params()[0].T @ (gi[:, None] * bp.get_state(True, False)[0]).sum(0)
    d = np.abs(h - href).max() / max(1.0, np.abs(href).max())
    seen.field = max(getattr(seen, "field", 0.0), d)
    assert d <= 1e-12, (what, h, href)


def _sweeps_one_by_one_then_queued(S, orc, t, label):
    """four sweeps (damping 0.7, 0.7, 1, 1) one call each against the model, state, reported maximum and field after every
    sweep; then the same sweeps on a second engine as two calls of two, state and field compared after each call"""
    seen = _Seen(label)
    clamped = None if t["conf"] is None else t["conf"] != -1
    g, bp, ob = _pair(S, orc, t)
    psi0 = bp.get_state()[0]
    ref = []
    for k, damp in enumerate(cg.DAMPS):
        d1, d2 = bp.sweep(1, damp), cm.sweep(ob, t["step"], damp, clamped)
        _compare_state(seen, bp.get_state(), ob, k)
        seen.per_sweep(abs(d1 - d2), "difference of sweep %d" % k)
        _field(seen, bp, t, "field after sweep %d" % k)
        ref.append(ob.get_state() + (d2,))
    assert bp.stats().psi_form_sweeps == 0
    _, bq, _ = _pair(S, orc, t)
    done = 0
    for n, damp in cg.CALLS:
        assert cg.DAMPS[done:done + n] == (damp,) * n
        d1 = bq.sweep(n, damp)
        done += n
        psi, msg = bq.get_state()
        opsi, omsg, d2 = ref[done - 1]
        seen.per_sweep(np.abs(psi - opsi).max(), "marginals after %d queued sweeps" % done)
        seen.per_sweep(np.abs(msg - omsg).max(), "messages after %d queued sweeps" % done)
        seen.per_sweep(abs(d1 - d2), "difference of queued sweep %d" % (done - 1))
        _field(seen, bq, t, "field after %d queued sweeps" % done)
    if clamped is not None:  # clamped rows stay bit for bit as initialised, on both engines
        rows = np.flatnonzero(clamped)
        assert np.array_equal(rows, bg.clamp_rows(t["cap"], t["rcap"])) and (psi0[rows, t["tc"][rows]] == 1.0).all()
        assert np.array_equal(bp.get_state()[0][rows], psi0[rows]) and np.array_equal(bq.get_state()[0][rows], psi0[rows])
    seen.report(", field %.3g" % seen.field)


@pytest.mark.parametrize("Q,dc", cg.LAST)
def test_blocks_last_at_every_label_count(S, orc, Q, dc):
    t = cg.instance(Q, dc, "last")
    _sweeps_one_by_one_then_queued(S, orc, t, "coloured steps, blocks last, cap %d Q %d dc %d" % (t["cap"], Q, dc))


@pytest.mark.parametrize("name", ["first", "cut"])
@pytest.mark.parametrize("Q,dc", cg.OTHER)
def test_blocks_first_and_the_cut_layout(S, orc, Q, dc, name):
    t = cg.instance(Q, dc, name)
    _sweeps_one_by_one_then_queued(S, orc, t, "coloured steps, %s, cap %d Q %d dc %d" % (name, t["cap"], Q, dc))


@pytest.mark.parametrize("Q", cg.CLAMPED_Q)
def test_clamped_rows_in_later_steps(S, orc, Q):
    t = cg.instance(Q, 0, "last", clamp=True)
    _sweeps_one_by_one_then_queued(S, orc, t, "coloured steps, blocks last, cap %d Q %d clamped" % (t["cap"], Q))


@pytest.mark.parametrize("Q,dc,records", cg.RING)
def test_a_step_of_256_and_of_257_records(S, orc, Q, dc, records):
    t = cg.instance(Q, dc, "ring%d" % records)
    seen = _Seen("coloured steps, ring of %d records, Q %d dc %d" % (records, Q, dc))
    g, bp, ob = _pair(S, orc, t)
    tb = t["tables"]
    assert tb["seg0"][1] - tb["seg0"][0] == records == tb["max_rec"]
    d1 = bp.sweep(4, 1.0)
    for _ in range(4):
        d2 = cm.fast_sweep(ob, t["step"], 1.0)
    assert d2 > 1e-6  # still moving
    _compare_state(seen, bp.get_state(), ob, 3)
    seen.per_sweep(abs(d1 - d2), "difference of the fourth sweep")
    _field(seen, bp, t, "field after four sweeps in one call")
    seen.report(", field %.3g" % seen.field)


@pytest.mark.parametrize("Q,dc", cg.CONVERGE)
def test_converge_on_blocks_last(S, orc, Q, dc):
    t = cg.instance(Q, dc, "last")
    seen = _Seen("coloured steps, converge, cap %d Q %d dc %d" % (t["cap"], Q, dc))
    g, bp, ob = _pair(S, orc, t)
    n1, l1 = bp.converge(1e-10, cg.CONVERGE_SWEEPS, 1.0)
    n2, l2 = cm.converge(ob, t["step"], 1e-10, cg.CONVERGE_SWEEPS, 1.0, fast=True)
    if (Q, dc) in cg.NOT_CONVERGING:
        assert n1 < 0 and n2 < 0, (n1, n2, l1, l2)
        return
    assert n1 >= 0 and n2 >= 0 and l1 < 1e-10 and abs(n1 - n2) <= 1, (n1, n2, l1, l2)  # the margin of tests/test_gpu_coloured.py for this order
    seen.against_oracle(bp.get_state()[0], ob.get_state()[0], "converged marginals")
    _field(seen, bp, t, "field after converge")
    seen.report(", converged at sweep %d, the model at %d" % (n1, n2))
