"""CPU side of tests/test_gpu_batch_scale.py and of the tile-shape cases of tests/test_gpu_agreement.py: the recipes of
tests/batch_scale_graph.py have exactly the segment counts they are named for (the next smaller ring has one less) and no hub
row, the launch arithmetic puts every case on the intended side of its threshold, the agreement cases reach every tile shape,
the constants of the model are those of the two source files, and the oracle is finite and insensitive to rounding over the
compared sweeps of every sweep case. No GPU and no engine."""
import os
import re

import numpy as np
import pytest

import batch_scale_graph as sc
import boundary_graph as bg
import coloured_step_graph as cg
from conftest import ROOT

CSRC = os.path.join(ROOT, "sbm-bp_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# the constants are the kernels' and the host's
# ---------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    kb = open(os.path.join(CSRC, "kernels_batch.h")).read()
    eng = open(os.path.join(CSRC, "engine.hip")).read()
    hr = open(os.path.join(CSRC, "host_reduce.h")).read()
    assert "constexpr int AG_V = %d, AG_TPB = %d, AG_MAXN = %d, AG_CPMAX = %d;" % (sc.AG_V, sc.AG_TPB, sc.AG_MAXN, sc.AG_CPMAX) in kb
    assert "constexpr int EM_FRAME_QMAX = %d;" % sc.EM_FRAME_QMAX in kb
    assert "for (uint32_t r = threadIdx.x & 63; r < rows; r += %d)" % sc.FOLD_LANES in kb  # k_fold_batch
    assert "return (CP & 16u) ? CP : CP + 16u;" in kb and "((n + 7u) & ~7u)" in kb         # S and LN
    assert re.search(r"constexpr int BLOCK = %d;" % sc.BLOCK, open(os.path.join(CSRC, "kernels.h")).read())
    # batch_reductions: the row chunks appear in the grid AND as the kernel's argument
    red = eng[eng.index("int batch_reductions("):eng.index("// ---- agreement of replicas")]
    assert "nbf = std::max<uint32_t>(1, (N + %d) / %d), rows = e->n_blk + e->n_hub;" % (sc.FIELD_ROWS - 1, sc.FIELD_ROWS) in red
    assert "R, N, %du, int(e->dc != 0), b->d_em_part[0]));" % sc.FIELD_ROWS in red
    assert "nbm = std::max<uint32_t>(1, (N + %d) / %d);" % (sc.MOMENT_ROWS - 1, sc.MOMENT_ROWS) in red
    assert "int(Q), K, %du, int(Tm)," % sc.MOMENT_ROWS in red
    assert "nbe = uint32_t(std::min<uint64_t>(%d, std::max<uint64_t>(1, (e->E2 + BLOCK - 1) / BLOCK)));" % sc.EDGE_GRID_CAP in red
    assert "g = (N + BLOCK - 1) / BLOCK" in red
    ag = eng[eng.index("// ---- agreement of replicas"):]
    assert "constexpr size_t AG_PART_BUDGET = size_t(%d) << 20;" % (sc.AG_PART_BUDGET >> 20) in ag
    assert "constexpr uint32_t AG_GRID = %d;" % sc.AG_GRID in ag
    assert "const int tpw = CT * CT <= 4 ? 1 : (CT * CT <= 16 ? 4 : 16);" in ag
    assert "tile_rows = std::min<uint32_t>(CT, uint32_t(4 * tpw) / CT)" in ag and sc.AG_TPB // 64 == 4
    assert "std::min<size_t>({size_t((n_trips + 3) / 4), size_t(AG_GRID / gy), AG_PART_BUDGET / (size_t(CP) * CP)})" in ag
    assert "(mode == 0 && N <= %d)" % sc.EXACT_MAX_N in hr


# ---------------------------------------------------------------------------------------------------------------------
# the rings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(sc.RING_N))
def test_ring_sizes_are_the_smallest_with_their_segment_count(key):
    cap, rcap, half, segments = key
    N = sc.RING_N[key]
    assert N % 4 == 0 and sc.ring_size(cap, rcap, half, segments) == N
    assert sc.ring_counts(N, half, cap, rcap) == (segments, 0)          # no hub row
    assert sc.ring_counts(N - 4, half, cap, rcap) == (segments - 1, 0)  # the neighbour has one less
    pairs = sc.graph(N, half, cap, rcap)["pairs"].astype(np.int64)
    assert (pairs[:, 0] != pairs[:, 1]).all() and len(np.unique(np.sort(pairs, 1) @ [N, 1])) == len(pairs)


def test_the_table_of_sizes():
    """the figures DESIGN.md quotes"""
    got = {k: (sc.RING_N[k], sc.graph(sc.RING_N[k], k[2], k[0], k[1])["E2"]) for k in sc.RING_N if k[3] >= 256}
    assert got == {(128, 64, 1, 256): (13008, 32520), (128, 64, 1, 257): (13060, 32650), (128, 64, 1, 513): (26116, 65290),
                   (512, 256, 4, 256): (15304, 130084), (512, 256, 4, 257): (15364, 130594)}
    d = sc.DENSE
    gr = sc.graph(d["N"], d["half"], 128, 64)
    assert (gr["n_blocks"], len(gr["hubs"]), gr["E2"]) == (d["segments"], 0, d["E2"])
    assert int(gr["deg"].max()) <= 128  # no hub row in the class of Q = 9 .. 16


def test_sweep_cases_straddle_the_fold_of_256_records():
    seen = set()
    for Q, dc, segs in sc.SWEEP:
        t = sc.segments_instance(Q, dc, segs)
        assert (t["n_blocks"], t["hubs"]) == (segs, [])
        seen.add(((t["cap"], t["rcap"]), segs, t["launch"]["finalize_trips"]))
    assert {(c, s) for c, s, _ in seen} == {((128, 64), 256), ((128, 64), 257), ((128, 64), 513), ((512, 256), 256), ((512, 256), 257)}
    assert {s: n for _, s, n in seen} == {256: 1, 257: 2, 513: 3}  # one whole trip; one record more; a third trip of one record
    assert {(Q, dc) for Q, dc, _ in sc.SWEEP} == {(9, 0), (9, 1), (16, 0), (3, 0), (4, 2)}
    Q, dc, segs, r = sc.SINGLE_ENGINE
    assert (Q, dc, segs) in sc.SWEEP and segs == 257 and 0 < r < sc.R


def test_coloured_cases_are_steps_of_256_and_257_records():
    for Q, dc, n in sc.COLOURED:
        tb = cg.layout(128, 64, "ring%d" % n)["tables"]
        assert tb["seg0"][1] - tb["seg0"][0] == n == tb["max_rec"] and bg.caps_for(Q) == (128, 64)
    assert {n for _, _, n in sc.COLOURED} == {256, 257} and {dc for _, dc, _ in sc.COLOURED} == {0, 1}


def test_em_cases_sit_on_their_thresholds():
    # the frame fold: 64 / 65 / 128 / 129 rows = 1 / 2 / 2 / 3 trips of the lanes, in the class of either label count
    for Q, dc, rows in sc.EM_FOLD:
        t, mode, K = sc.em_instance("fold", Q, dc, rows)
        L = t["launch"]
        assert L["rows"] == rows and t["hubs"] == [] and L["frame_fold_trips"] == {64: 1, 65: 2, 128: 2, 129: 3}[rows]
        assert (mode, K) == ((2, sc.SERIES_K) if dc == 0 else (0, 0))
        assert L["em_edges"] == (Q > 8)
        if dc == 0:  # the forced series: the moments' fold is short here (the long one is EM_SERIES)
            assert sc.series_order_model(Q, t["N"], t["cab"], K) == sc.SERIES_K and L["moment_fold_trips"] == 1
    assert {Q for Q, _, _ in sc.EM_FOLD} == {5, 12} and {bg.caps_for(5), bg.caps_for(12)} == {(256, 128), (128, 64)}
    # the field refresh: one and two chunks of 4096 rows
    assert [sc.em_instance("field", *c)[0]["launch"]["nbf"] for c in sc.EM_FIELD] == [1, 2]
    assert all(dc != 0 for _, dc, _ in sc.EM_FIELD)
    # the exact non-edge term: 8 x 8 and 9 x 9 workgroups, 64 and 81 rows in the fold
    ex = [sc.em_instance("exact", *c) for c in sc.EM_EXACT]
    assert [(t["launch"]["g"], t["launch"]["exact_fold_trips"], mode) for t, mode, _ in ex] == [(8, 1, 1), (9, 2, 1)]
    assert all(t["N"] ** 2 * t["Q"] ** 2 <= 7e8 for t, _, _ in ex)  # the oracle's exact loop stays well under a second
    # the automatic series above the switch: 65 rows in the moments' fold
    for c in sc.EM_SERIES:
        t, mode, K = sc.em_instance("series", *c)
        assert mode == 0 and K == 0 and not t["launch"]["exact_auto"] and (t["launch"]["nbm"], t["launch"]["moment_fold_trips"]) == (65, 2)
        orders = [sc.series_order_model(t["Q"], t["N"], cab) for cab, _ in bg.three_params(t)]
        assert orders == [3, 3, 3], orders
    assert sc.launch_model(32768, 0, 1, 0, 4)["exact_auto"] and sc.launch_model(32768, 0, 1, 0, 4)["nbm"] == 64
    # the dense ring: the cap of 1024 workgroups decides, and 32 workgroups take a second trip
    for Q, dc in sc.EM_DENSE:
        t, mode, K = sc.em_instance("dense", Q, dc, None)
        L = t["launch"]
        assert t["E2"] == 270336 > 262144 and L["em_edges"] and L["edge_capped"] and L["nbe"] == 1024 and L["edge_blocks_twice"] == 32
        assert L["edge_fold_trips"] == 16 and t["hubs"] == [] and dc != 0
    assert {(Q, dc == 2) for Q, dc in sc.EM_DENSE} == {(9, False), (16, False), (12, True)}
    # and every smaller EM case is on the other side of the cap
    assert not any(sc.em_instance("fold", *c)[0]["launch"]["edge_capped"] for c in sc.EM_FOLD)


def test_launch_model_at_its_edges():
    m = sc.launch_model
    assert [m(N, 10, 1, 0, 3)["nbf"] for N in (1, 4095, 4096, 4097, 8192, 8193)] == [1, 1, 1, 2, 2, 3]
    assert [m(10, E2, 1, 0, 9)["nbe"] for E2 in (0, 1, 256, 257, 262144, 262145, 10 ** 7)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert [m(10, E2, 1, 0, 9)["edge_blocks_twice"] for E2 in (262144, 262145, 270336)] == [0, 1, 32]
    assert m(10, 10, 7, 2, 9)["rows"] == 9 and not m(10, 10, 1, 0, 8)["em_edges"] and m(10, 10, 1, 0, 9)["em_edges"]


# ---------------------------------------------------------------------------------------------------------------------
# the agreement launch
# ---------------------------------------------------------------------------------------------------------------------
def test_agree_plan_covers_every_tile_shape():
    by_ct = {}
    for CT in range(1, 17):
        p = sc.agree_plan(1, 16) if CT == 1 else sc.agree_plan(CT, 16)
        assert p["CT"] == CT and p["CP"] == 16 * CT and sum(p["split"]) == CT and max(p["split"]) == p["tile_rows"]
        assert 4 * p["TPW"] >= p["tile_rows"] * CT  # the accumulators hold a workgroup row
        by_ct[CT] = p
    assert [by_ct[CT]["TPW"] for CT in range(1, 17)] == [1, 1, 4, 4] + [16] * 12
    assert {CT: by_ct[CT]["split"] for CT in range(9, 17)} == {9: (7, 2), 10: (6, 4), 11: (5, 5, 1), 12: (5, 5, 2), 13: (4, 4, 4, 1),
                                                                 14: (4, 4, 4, 2), 15: (4, 4, 4, 3), 16: (4, 4, 4, 4)}
    assert all(by_ct[CT]["split"] == (CT,) for CT in range(1, 9))
    # S: the one of CP and CP + 16 that is 16 mod 32 - CP for an odd tile count, CP + 16 for an even one
    assert all(by_ct[CT]["S"] == 16 * CT + (0 if CT % 2 else 16) and by_ct[CT]["S"] % 32 == 16 for CT in by_ct)
    assert [sc.agree_plan(n, 2)["LN"] for n in (1, 8, 9, 16, 17, 127, 128)] == [8, 8, 16, 16, 24, 128, 128]


def test_the_agreement_cases_reach_every_shape():
    """a condition on the case list of tests/test_gpu_agreement.py, not a measurement"""
    before = [sc.agree_plan(n, Q) for n, Q in sc.AGREE_BEFORE]
    assert sorted({p["CT"] for p in before}) == [1, 2, 5, 16]  # what the file reached before
    new = [sc.agree_plan(n, Q) for n, Q in sc.AGREE]
    assert len(set(sc.AGREE)) == len(sc.AGREE) and not set(sc.AGREE) & set(sc.AGREE_BEFORE)
    assert sorted({p["CT"] for p in before + new}) == list(range(1, 17))
    assert {p["TPW"] for p in new} == {4, 16} and {p["TPW"] for p in before + new} == {1, 4, 16}
    assert sorted({p["CT"] for p in new if p["TPW"] == 4}) == [3, 4]  # k_agree<KIND, 4>
    want = {(7, 2), (6, 4), (5, 5, 1), (5, 5, 2), (4, 4, 4, 1), (4, 4, 4, 2), (4, 4, 4, 3), (4, 4, 4, 4)}
    assert want <= {p["split"] for p in new}
    assert {p["S"] == p["CP"] for p in new} == {True, False}  # both parities of S
    pads = {p["CT"]: set() for p in new}
    for p in new:
        pads[p["CT"]].add(p["pad"])
    assert any({0, 15} <= v for v in pads.values())   # an exact multiple of 16 and one column over it, at the same tile count
    assert any({0, 1} <= v for v in pads.values())    # ... and one column under
    assert {0, 1, 2, 15} <= set().union(*pads.values())
    n_max = max(n for n, _ in sc.AGREE)
    assert n_max == sc.AG_MAXN and sc.agree_plan(n_max, 2)["LN"] == 128 and sc.agree_plan(n_max, 2)["CP"] == sc.AG_CPMAX
    assert any(n > 16 and sc.agree_plan(n, Q)["LN"] > n for n, Q in sc.AGREE)  # label rows with padding bytes
    assert sum(n > sc.AG_TPB // 4 for n, _ in sc.AGREE) >= 2                   # s_slot filled by more than one wave
    # one thread fills one slot: above 64 replicas the second wave takes part, at 128 two whole waves
    assert any(64 < n < 128 for n, _ in sc.AGREE)


def test_the_budget_decides_the_grid_of_the_budget_case():
    N, n, Q = sc.AGREE_BUDGET
    p = sc.agree_plan(n, Q)
    assert (p["CP"], p["gy"]) == (256, 4)
    assert sc.agree_gx_terms(N, p["CP"], p["gy"]) == (157, 256, 128) and sc.agree_gx(N, p["CP"], p["gy"]) == 128
    # every other agreement case of the suite is decided by the trips
    for N2, cases in ((777, sc.AGREE + sc.AGREE_BEFORE), (20011, [(5, 4)])):
        for n2, Q2 in cases:
            q = sc.agree_plan(n2, Q2)
            terms = sc.agree_gx_terms(N2, q["CP"], q["gy"])
            assert terms[0] < min(terms[1:]), (N2, n2, Q2, terms)
    assert sc.agree_gx(16384, 256, 4) == 128 and sc.agree_gx_terms(16384, 256, 4)[0] == 128  # the budget decides above N = 16 384
    assert sc.agree_gx_terms(16385, 256, 4)[0] == 129


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU file: the reference is finite and insensitive to rounding over the compared sweeps
# ---------------------------------------------------------------------------------------------------------------------
def _oracles(orc, t, msg_form=True):
    return [bg.oracle_of(orc, t, msg_form, bg.BATCH_SEEDS[r], cab, na)[1] for r, (cab, na) in enumerate(bg.three_params(t))]


@pytest.mark.parametrize("Q,dc,segs", sc.SWEEP)
def test_sweep_cases_are_finite_stable_and_converge(orc, Q, dc, segs):
    """every replica of every sweep case: finite over the four compared sweeps; a start perturbed by a relative 1e-13 (three
    seeds, as tests/test_wide_cpu.py) ends them within 1e-12; and converge_sync stops, not by a margin that rounding could
    move, at the same sweep (+- 2) from the perturbed starts"""
    t = sc.segments_instance(Q, dc, segs)
    worst, counts = 0.0, []
    for r, ob in enumerate(_oracles(orc, t)):
        start = ob.get_state()
        for k, damp in enumerate(bg.BATCH_DAMPS):
            d = ob.sweep_sync(damp)
            assert np.isfinite(d) and d > 1e-6 and all(np.isfinite(x).all() for x in ob.get_state()), (r, k, d)  # still moving
        base = ob.get_state()
        n, last = ob.converge_sync(1e-10, sc.CONVERGE_SWEEPS, 1.0)
        assert n >= 0 and last < 0.999e-10 and ob.ar_levels() == (0, -1), (r, n, last)  # plain sweeps: no relaxation engaged
        counts.append(n + len(bg.BATCH_DAMPS))
        for seed in (1, 2, 3):
            ob2 = _oracles(orc, t)[r]
            ob2.set_state(*sc.perturbed(start, seed))
            for damp in bg.BATCH_DAMPS:
                ob2.sweep_sync(damp)
            dev = max(float(np.abs(a - b).max()) for a, b in zip(ob2.get_state(), base))
            worst = max(worst, dev)
            assert dev <= 10 * 1e-13, (r, seed, dev)
            n2, _ = ob2.converge_sync(1e-10, sc.CONVERGE_SWEEPS, 1.0)
            assert n2 >= 0 and abs(n2 - n) <= 2, (r, seed, n, n2)
    print("batch scale Q %d dc %d, %d segments: amplification of a relative 1e-13 over the compared sweeps %.3g; oracle sweeps to 1e-10: %s"
          % (Q, dc, segs, worst / 1e-13, counts))


@pytest.mark.parametrize("kind,case", [("fold", c) for c in sc.EM_FOLD] + [("field", c) for c in sc.EM_FIELD] + [("exact", c) for c in sc.EM_EXACT] +
                         [("series", c) for c in sc.EM_SERIES] + [("dense", c + (None,)) for c in sc.EM_DENSE])
def test_em_cases_are_finite_and_still_moving(orc, kind, case):
    """three sweeps with the field relaxed by 0.5, as the GPU test runs them: finite, and not converged"""
    t, _, _ = sc.em_instance(kind, *case)
    for r, ob in enumerate(_oracles(orc, t)):
        ob.set_field_mix(0.5)
        for k in range(3):
            d = ob.sweep_sync(1.0)
            assert np.isfinite(d) and d > 1e-6 and all(np.isfinite(x).all() for x in ob.get_state()), (kind, case, r, k, d)


@pytest.mark.parametrize("first", sc.LEARN_FIRST_OUT)
def test_one_replica_of_the_learning_case_leaves_the_mask_first(orc, first):
    """the oracle's synchronous learning on the two-chunk ring: every BP run converges, and the replica started at the larger
    cab ends at least two EM steps before the others, so the reductions of those rounds run with it masked out"""
    t, _, _ = sc.em_instance("field", *sc.LEARN_CASE)
    assert t["launch"]["nbf"] == 2
    steps = []
    for r in range(sc.R):
        scale = sc.LEARN_EARLY if r == first else sc.LEARN_SCALES[r]
        ob = bg.oracle_of(orc, t, True, bg.BATCH_SEEDS[r], t["cab"] * scale, t["na"])[1]
        n, f = ob.learning(*sc.LEARN_ARGS, None, sync=True, series_K=0)
        assert np.isfinite(f) and ob.learn_unconverged() == 0 and 0 < n < sc.LEARN_ARGS[1], (r, n, f)
        steps.append(n)
    print("batch scale learning, replica %d first: oracle EM steps %s" % (first, steps))
    assert all(steps[first] + 2 <= s for r, s in enumerate(steps) if r != first), steps
