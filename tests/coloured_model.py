"""TEST INFRASTRUCTURE - the coloured sweep order (include/sbmbp.h sbmbp_set_sweep_order) restated
for the tests: the plan in a few lines of Python, and one sweep assembled from oracle calls only (no arithmetic of its own).

A step updates its rows at once from the state at the start of the step: for every unclamped row i of the step the marginals
are put back to those of the step's start (set_state(psi0, None)), the field is rebuilt from them (init_h: the field frozen
at the step's start, which includes every earlier step of the sweep), and node_update(i) - the reference's own update of
one vertex - forms row i's marginal and out-messages. Messages are written in place: rows of a step are pairwise
non-adjacent, so none reads what another writes. After the last row the step's new marginals are put in together.
Cost: one state copy per row; meant for N <= 1000 (a few sweeps) and N <= 400 (whole convergence runs)."""
import math

import numpy as np


def plan(row_ptr, nbr, colour=None, step_fraction=0.0):
    """(n_colours, n_steps, colour[N], step[N]). Colouring: vertices in order (degree descending, index ascending) take the
    smallest colour no neighbour holds, self-loops ignored. Steps: classes in colour order, rows ascending, consecutive
    chunks of at most B = max(1, ceil(step_fraction N)) rows (step_fraction 0 = 1/8)."""
    N = len(row_ptr) - 1
    deg = np.diff(np.asarray(row_ptr, dtype=np.int64))
    if colour is None:
        colour = np.full(N, -1, dtype=np.int64)
        for i in sorted(range(N), key=lambda v: (-deg[v], v)):
            taken = {int(colour[l]) for l in nbr[int(row_ptr[i]):int(row_ptr[i + 1])] if l != i}
            colour[i] = next(c for c in range(N + 1) if c not in taken)
    colour = np.asarray(colour, dtype=np.int64)
    B = max(1, math.ceil((step_fraction if step_fraction else 0.125) * N))
    step = np.zeros(N, dtype=np.int64)
    n_steps = 0
    for c in range(int(colour.max()) + 1 if N else 0):
        rows = np.flatnonzero(colour == c)
        step[rows] = n_steps + np.arange(len(rows)) // B
        n_steps += (len(rows) + B - 1) // B
    return (int(colour.max()) + 1 if N else 0), n_steps, colour, step


def is_proper(row_ptr, nbr, colour):
    src = np.repeat(np.arange(len(row_ptr) - 1), np.diff(np.asarray(row_ptr, dtype=np.int64)))
    nbr = np.asarray(nbr, dtype=np.int64)
    return bool(((colour[src] != colour[nbr]) | (src == nbr)).all())


def _psi(ob):
    """the oracle's marginals alone (OracleBP.get_state copies the messages too)"""
    import oracle
    psi = np.zeros((ob.g.N, ob.Q))
    oracle.lib().orc_bp_get_state(ob._h, psi.ctypes.data_as(oracle.c_dp), None)
    return psi


def _row_by_sync_sweep(ob, psi0, msg, i, damp):
    """row i's update from (psi0, msg) by the oracle's synchronous sweep: the same equations as node_update's small-degree
    path, evaluated with rescaled products (bp_oracle.cpp sweep_sync). Leaves ob at (psi0, msg with row i's new out-messages);
    returns (row i's new marginal, its undamped 1-step difference)"""
    k0, k1 = int(ob.g.row_ptr[i]), int(ob.g.row_ptr[i + 1])
    ob.set_state(psi0, msg)
    ob.sweep_sync(damp)
    psi1, msg1 = ob.get_state()
    d = np.abs(msg1[k0:k1] - msg[k0:k1]).max(initial=0.0) / damp  # a damped message moves by damp * (new - old)
    msg[k0:k1] = msg1[k0:k1]
    ob.set_state(psi0, msg)
    return psi1[i].copy(), d


def sweep(ob, step, damp=1.0, clamped=None):
    """one coloured sweep on the oracle `ob` (oracle.OracleBP with state and parameters set), in place; returns the maximum
    over the updated rows of node_update's undamped 1-step difference (0 when nothing has an edge).
    node_update's small-degree path multiplies a row's factors as they are, and on a row of several hundred edges that
    product leaves the double range (0/0). The reference itself switches to a log-domain path at degree 50, which drops beta
     and is not what the engine computes; a row whose small-degree update comes back non-finite is therefore
    taken from the oracle's synchronous sweep instead (same equations, rescaled products), from the same frozen state."""
    step = np.asarray(step)
    md = 0.0
    for s in range(int(step.max()) + 1 if len(step) else 0):
        rows = [int(i) for i in np.flatnonzero(step == s) if clamped is None or not clamped[i]]
        if not rows:
            continue
        psi0 = _psi(ob)
        new = {}
        for i in rows:
            ob.set_state(psi0, None)
            ob.init_h()
            long_row = int(ob.g.row_ptr[i + 1] - ob.g.row_ptr[i]) >= 50  # only such rows can leave the range: keep their old messages
            before = ob.get_state()[1] if long_row else None
            d = ob.node_update(i, damp, large=False)
            row = _psi(ob)[i]
            if long_row and not (np.isfinite(row).all() and np.isfinite(d)):
                row, d = _row_by_sync_sweep(ob, psi0, before, i, damp)
            md = max(md, d)
            new[i] = row
        for i, v in new.items():
            psi0[i] = v
        ob.set_state(psi0, None)
    ob.init_h()
    return md


def fast_sweep(ob, step, damp=1.0, clamped=None):
    """sweep() with one oracle call per STEP instead of a state copy per row: the state of the step's start is put back
    (set_state) and the field rebuilt from it (init_h), ONE synchronous sweep updates every row from that frozen state, and
    only the marginals and out-messages of the step's unclamped rows are kept - _row_by_sync_sweep for the whole step. Same
    equations as sweep(); the products are rescaled (bp_oracle.cpp sweep_sync), so the two agree to rounding, not bit for bit
    (tests/test_coloured_step_cpu.py). For graphs of tens of thousands of rows and for whole convergence
    runs."""
    step = np.asarray(step)
    row_ptr = np.asarray(ob.g.row_ptr, dtype=np.int64)
    edge_step = np.repeat(step, np.diff(row_ptr))
    keep = np.ones(len(step), dtype=bool) if clamped is None else ~np.asarray(clamped, dtype=bool)
    edge_keep = np.repeat(keep, np.diff(row_ptr))
    md = 0.0
    psi0, msg0 = ob.get_state()
    for s in range(int(step.max()) + 1 if len(step) else 0):
        rows, edges = (step == s) & keep, (edge_step == s) & edge_keep
        if not rows.any():
            continue
        ob.set_state(psi0, msg0)
        ob.init_h()
        ob.sweep_sync(damp)
        psi1, msg1 = ob.get_state()
        md = max(md, np.abs(msg1[edges] - msg0[edges]).max(initial=0.0) / damp)  # a damped message moves by damp * (new - old)
        psi0[rows] = psi1[rows]
        msg0[edges] = msg1[edges]
    ob.set_state(psi0, msg0)
    ob.init_h()
    return float(md)


def converge(ob, step, crit, tmax, damp=1.0, clamped=None, fast=False):
    """(niter, last difference): 0-based index of the first sweep whose difference is below crit, or -1 after tmax sweeps"""
    last = 0.0
    for it in range(tmax):
        last = (fast_sweep if fast else sweep)(ob, step, damp, clamped)
        if last < crit:
            return it, last
    return -1, last


def sequential_sweep(ob, order, damp=1.0, clamped=None):
    """the reference's schedule with a fixed vertex order: node_update one vertex at a time, the field kept current by
    node_update itself (bp.cpp:1088-1095)"""
    md = 0.0
    for i in order:
        if clamped is None or not clamped[i]:
            md = max(md, ob.node_update(int(i), damp, large=False))
    return md
