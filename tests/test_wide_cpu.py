"""The instances of tests/wide_cases.py checked on the oracle alone, before tests/test_gpu_wide_relax.py relies on them: every
run on the hub graph ends on the levels and with the status the table states, and does so again - same levels, sweep count
within 2 - from an initial state perturbed by a relative 1e-13 (a run that a rounding error can push onto another branch of the
convergence machine says nothing about the engine's copy of it); the ring graphs sit on the segment counts that put the fold
on, at and just above its two-stage threshold, and the oracle converges on them."""
import numpy as np
import pytest

import boundary_graph as bg
import wide_cases as wc

ALL = wc.FIELD + wc.DAMPED + wc.PROBE + wc.EXHAUSTED + wc.NO_AUTO + wc.FIXED_MIX


def test_ladders_restate_the_oracles():
    """ar_t of oracle/bp_oracle.cpp: FIELD, GMIX, GDAMP"""
    assert wc.FIELD_CAP == (1.0, 0.25, 0.1, 0.05)
    assert [wc.GEN_MIX[g] for g in range(7)] == [0.5, 0.25, 0.5, 0.25, 0.1, 0.25, 0.1]
    assert [wc.GEN_DAMP[g] for g in range(7)] == [1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25]
    assert wc.mix_damp(0, -1) == (1.0, 1.0) and wc.mix_damp(1, -1) == (0.25, 1.0) and wc.mix_damp(0, 2) == (0.5, 0.5)
    assert wc.mix_damp(0, 4) == (0.1, 0.5) and wc.mix_damp(0, 6) == (0.1, 0.25) and wc.mix_damp(0, -1, 0.25) == (0.25, 1.0)


def test_the_cases_cover_every_tile_count_and_branch():
    assert sorted({(c.Q + 15) // 16 for c in wc.FIELD}) == [2, 3, 4] and {c.Q % 2 for c in wc.FIELD} == {0, 1}
    assert all(c.levels == (1, -1) for c in wc.FIELD)
    assert all(c.levels[1] >= 2 and wc.mix_damp(*c.levels)[1] < 1.0 for c in wc.DAMPED + wc.PROBE + wc.EXHAUSTED)
    assert {(c.Q + 15) // 16 for c in wc.DAMPED} == {2, 3, 4}
    assert len({c.id for c in ALL}) == len(ALL)
    for c in ALL:
        cab, na, tc = c.arrays()
        assert cab.shape == (c.Q, c.Q) and (cab == cab.T).all() and (cab > 0).all() and na.sum() == wc.HUB_N and na.min() >= 600 // c.Q
        assert c.Q > 16


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_oracle_levels_and_stability(orc, case):
    ob, n, last = case.run_oracle(orc)
    print("wide relax %s: oracle %d sweeps, levels %s, last %.3g" % (case.id, n, ob.ar_levels(), last))
    assert n == case.niter and ob.ar_levels() == case.levels, (n, ob.ar_levels())
    assert np.isfinite(last) and (last < wc.CRIT) == case.converges
    if not case.converges:
        assert last > 1e3 * wc.CRIT  # nowhere near the criterion at the limit: no sweep more or less changes the status
    psi = ob.get_state()[0]
    for seed in wc.PERTURB_SEEDS:
        ob2, n2, last2 = case.run_oracle(orc, perturb=seed)
        assert ob2.ar_levels() == case.levels, (seed, n2, ob2.ar_levels())
        assert (n2 >= 0) == case.converges and (abs(n2 - n) <= 2 if case.converges else n2 == -1), (seed, n, n2)
        if case.converges:  # the same fixed point
            assert np.abs(ob2.get_state()[0] - psi).max() < 1e-7, seed


def test_plain_jacobi_does_not_converge_on_any_relaxing_case(orc):
    """without the machine every case but the one listed stays far from the criterion: what the engine's copy of it does
    decides the outcome"""
    seen = set()
    for c in wc.FIELD + wc.DAMPED + wc.PROBE:
        if c.id in wc.JACOBI_CONVERGES or (c.family, c.cin, c.cout, c.Q, c.seed) in seen:
            continue
        seen.add((c.family, c.cin, c.cout, c.Q, c.seed))
        og, ob = c.oracle(orc)
        ob.set_auto_relax(False)
        n, last = ob.converge_sync(wc.CRIT, 60, 1.0)
        assert n == -1 and last > 1e-4, (c.id, n, last)


@pytest.mark.parametrize("N", sorted(wc.RING_SIZES))
def test_ring_segment_counts(N):
    pairs = wc.ring_pairs(N)
    deg = np.bincount(pairs.astype(np.int64).ravel(), minlength=N)
    assert (pairs[:, 0] != pairs[:, 1]).all() and len(np.unique(np.sort(pairs.astype(np.int64), 1) @ [N, 1])) == len(pairs)
    assert set(deg) == {2, 3} and len(pairs) == N + N // 2 - (N // 2 + 2) // 3
    assert bg.caps_for(17) == bg.caps_for(64) == (wc.WCAP, wc.WRCAP) and wc.WRCAP * 3 <= wc.WCAP  # the row limit closes every segment
    bounds, hubs = bg.segment_model(deg, wc.WCAP, wc.WRCAP)
    segs, chunk, nb, last = wc.RING_SIZES[N]
    assert not hubs and len(bounds) - 1 == segs == -(-N // wc.WRCAP) and (np.diff(bounds)[:-1] == wc.WRCAP).all()
    assert wc.fold_model(segs) == (chunk, nb, last)
    assert (segs > 4 * wc.FOLD_BLOCKS) == (chunk > 0) and nb <= wc.FOLD_BLOCKS
    # the reductions' records are segments too, and their strides are within the staged fold's limit (engine.hip FOLD_STRIDE_MAX)
    assert 64 + 1 <= 128


def test_ring_sizes_straddle_the_threshold():
    assert sorted(s[0] for s in wc.RING_SIZES.values()) == [4 * wc.FOLD_BLOCKS, 4 * wc.FOLD_BLOCKS + 1, 4 * wc.FOLD_BLOCKS + 3]
    assert {(Q, dc) for Q, dc, N in wc.RING if N == 16432} == {(17, 0), (17, 1), (33, 0), (64, 0)}
    assert {N for Q, dc, N in wc.RING if (Q, dc) == (17, 0)} == set(wc.RING_SIZES)


@pytest.mark.parametrize("Q,dc,N", [r for r in wc.RING if r[0] < 64 and r[2] == 16432])
def test_oracle_converges_on_the_ring(orc, Q, dc, N):
    """(Q = 64 is compared over four sweeps only: 0.3 s per sweep on the oracle)"""
    t = wc.ring_instance(Q, dc, N)
    og, ob = wc.ring_oracle(orc, t)
    assert og.E2 == 2 * len(t["pairs"]) and (og.deg == t["deg"]).all()
    for damp in wc.RING_DAMPS:
        assert np.isfinite(ob.sweep_sync(damp))
    n, last = ob.converge_sync(wc.CRIT, 600, 1.0)
    print("wide ring Q %d dc %d N %d: oracle %d sweeps after the four compared ones, levels %s" % (Q, dc, N, n, ob.ar_levels()))
    assert 0 <= n < 200 and last < wc.CRIT and ob.ar_levels() == (0, -1)
    psi = ob.get_state()[0]
    assert np.isfinite(psi).all() and np.abs(psi[t["conf"] == -1] - 1.0 / Q).max() > 0.05  # not the trivial fixed point
