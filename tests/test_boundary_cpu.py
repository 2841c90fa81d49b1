"""The boundary graph recipe (tests/boundary_graph.py) checked on the CPU, before tests/test_gpu_boundary.py relies on it:
every threshold case is present in the segment plan of every capacity class (and disappears when its block is left out), the
Python segment model equals the C++ segment_plan on these degree sequences (through tests/sanitize/host_sanitize.cpp, built
with the sanitizers), and on every case of the GPU file the oracle stays finite over the compared sweeps and converges."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import boundary_graph as bg
import coloured_model as cm
from conftest import ROOT, gpath


@pytest.mark.parametrize("cap,rcap", bg.CLASSES)
def test_caps_restate_the_table(cap, rcap):
    qs = [Q for Q in range(2, 65) if bg.caps_for(Q) == (cap, rcap)]
    assert qs == {512: list(range(2, 5)), 256: list(range(5, 9)), 128: list(range(9, 17)), 64: list(range(17, 65))}[cap]


@pytest.mark.parametrize("whole_trips", [False, True])
@pytest.mark.parametrize("cap,rcap", bg.CLASSES)
def test_every_threshold_case_is_in_the_plan(cap, rcap, whole_trips):
    g = bg.graph(cap, rcap, whole_trips)
    pairs, N, ns, deg = g["pairs"], g["N"], g["ns"], g["deg"]
    assert ns == len(bg.boundary_degrees(cap, rcap)) and N == ns + 900 + 4
    assert (deg[:ns] == bg.boundary_degrees(cap, rcap)).all()  # distinct neighbours: the degrees are the recipe's
    assert (deg[N - 4:N - 1] == 0).all() and deg[N - 1] == cap + 1
    assert (pairs[:, 0] != pairs[:, 1]).all() and len(np.unique(pairs.astype(np.int64) @ [N, 1])) == len(pairs)
    structured = np.concatenate([np.arange(ns), [N - 1]])
    assert not (np.isin(pairs[:, 0], structured) & np.isin(pairs[:, 1], structured)).any()  # an independent set
    pool = (pairs[:, 0] >= ns) & (pairs[:, 0] < N - 4) & (pairs[:, 1] >= ns) & (pairs[:, 1] < N - 4)
    assert 1700 <= pool.sum() <= 1800  # about 2 pool random pairs inside the pool: not bipartite
    assert deg[ns:N - 4].max() <= 64 and deg[ns:N - 4].min() >= 1  # no pool vertex is a hub in any class
    assert ((2 * len(pairs)) % 64 == 0) == whole_trips  # k_wem: whole trips / a partial last trip
    for name, ok in bg.conditions(deg, cap, rcap, ns).items():
        assert ok, name
    # the hub rows, by degree: row 0, six separators and the last row at cap + 1; the three rows of the fragment block
    hubs = g["hubs"]
    assert sorted(int(d) for d in deg[hubs]) == sorted([cap + 1] * 8 + [bg.hub_whole(cap), 3 * 256 + 1, 3 * 256 - 1])
    assert bg.hub_whole(cap) % 256 == 0 and bg.hub_whole(cap) > cap + 1
    assert g["hub_edges"] == 8 * (cap + 1) + bg.hub_whole(cap) + 6 * 256
    print("cap %d rcap %d: N %d, %d segments, %d hub rows, %d hub edges, %d directed edges" % (cap, rcap, N, g["n_blocks"], len(hubs), g["hub_edges"], 2 * len(pairs)))


# what each block is there for: without it exactly these named conditions fail
NEEDS = {
    "smallest_hub": {"row 0 is a hub of cap + 1"},
    "full_row": {"segment (1, cap)"},
    "two_rows_fill": {"segment (2, cap)"},
    "both_caps": {"segment (rcap, cap)"},
    "no_edges": {"segment (rcap, 0)"},
    "row_limit_first": {"segment (rcap, rcap)"},
    "row_lengths": {"degree %d in a segment" % d for d in (31, 32, 33, 7, 8, 9)},
    "hub_fragments": {"hub of whole fragments", "hub of whole fragments + 1", "hub of whole fragments - 1", "adjacent hubs"},
}


@pytest.mark.parametrize("drop", bg.BLOCKS)
@pytest.mark.parametrize("cap,rcap", bg.CLASSES)
def test_a_dropped_block_fails_its_named_conditions(cap, rcap, drop):
    pairs, N, ns = bg.build(cap, rcap, drop=drop)
    missing = {k for k, ok in bg.conditions(bg.degrees(pairs, N), cap, rcap, ns).items() if not ok}
    assert missing == NEEDS[drop]


@pytest.mark.parametrize("cap,rcap", bg.CLASSES)
def test_class_zero_of_the_coloured_order_meets_the_shapes(cap, rcap):
    """the coloured order sets hub rows aside without closing the open segment (coloured_step_tables), so class 0 - all
    structured rows - packs differently from the synchronous plan. What it still meets: a full one-row segment, the two rows
    that fill one, a segment of rcap rows, rows of every named length, and all eleven hub rows in one step."""
    g = bg.graph(cap, rcap)
    deg, N, ns = g["deg"], g["N"], g["ns"]
    rows = list(range(ns)) + list(range(N - 4, N))
    segs, hubs = bg.step_segment_model(deg, rows, cap, rcap)
    shapes = {(len(s), int(deg[s].sum())) for s in segs}
    assert hubs == g["hubs"]
    assert (1, cap) in shapes and (2, cap) in shapes and any(r == rcap for r, _ in shapes)
    assert all(len(s) <= rcap and deg[s].sum() <= cap for s in segs)
    assert {31, 32, 33, 7, 8, 9} <= {int(deg[i]) for s in segs for i in s}


def test_segment_model_equals_segment_plan_under_the_sanitizers(tmp_path):
    """host_sanitize.cpp reads `cap rcap n, degrees, boundaries, hub rows` per plan and compares segment_plan with it; the
    degree sequences are the eight boundary graphs, each also without one block, and the structured rows alone"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    plans = []
    for cap, rcap in bg.CLASSES:
        for whole in (False, True):
            plans.append((cap, rcap, bg.graph(cap, rcap, whole)["deg"]))
        plans.append((cap, rcap, np.array(bg.boundary_degrees(cap, rcap))))
        for drop in bg.BLOCKS:
            pairs, N, _ = bg.build(cap, rcap, drop=drop)
            plans.append((cap, rcap, bg.degrees(pairs, N)))
    path = tmp_path / "plans.txt"
    with open(path, "w") as f:
        for cap, rcap, deg in plans:
            bounds, hubs = bg.segment_model(deg, cap, rcap)
            f.write("%d %d %d %d %d\n" % (cap, rcap, len(deg), len(bounds), len(hubs)))
            for v in (deg, bounds, hubs):
                f.write(" ".join(str(int(x)) for x in v) + "\n")
    exe = tmp_path / "host_sanitize"
    src = [os.path.join(ROOT, "tests", "sanitize", "host_sanitize.cpp"), os.path.join(ROOT, "sbm-bp_amd", "csrc", "host_graph.cpp"),
           os.path.join(ROOT, "oracle", "bp_oracle.cpp")]
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-mavx2", "-pthread",
                    "-o", str(exe)] + src, check=True, timeout=600)
    env = dict(os.environ, TMPDIR=str(tmp_path), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--plans", str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert pr.returncode == 0 and "host_sanitize ok: %d plans" % len(plans) in pr.stdout, (pr.stdout[-500:], pr.stderr[-3000:])
    assert "runtime error" not in pr.stderr and "AddressSanitizer" not in pr.stderr and "LeakSanitizer" not in pr.stderr
    # a plan that is off by one row is refused
    bad = tmp_path / "bad.txt"
    deg = bg.boundary_degrees(64, 16)
    bounds, hubs = bg.segment_model(deg, 64, 16)
    bounds[3] += 1
    with open(bad, "w") as f:
        f.write("64 16 %d %d %d\n" % (len(deg), len(bounds), len(hubs)))
        for v in (deg, bounds, hubs):
            f.write(" ".join(str(int(x)) for x in v) + "\n")
    pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--plans", str(bad)], capture_output=True, text=True, timeout=600, env=env)
    assert pr.returncode != 0 and "plan 0" in pr.stderr


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU file: the reference is finite over the compared sweeps and converges
# ---------------------------------------------------------------------------------------------------------------------
def _finite_then_converges(ob, damps, key):
    for k, damp in enumerate(damps):
        d = ob.sweep_sync(damp)
        psi, msg = ob.get_state()
        assert np.isfinite(d) and np.isfinite(psi).all() and np.isfinite(msg).all(), (key, k)
    n, last = ob.converge_sync(1e-10, 600, 1.0)
    print("%s: converge_sync niter %d, last %.3g" % (key, n, last))
    if key in bg.NOT_CONVERGING:
        assert n < 0, (key, "is listed as not converging, but converges")
    else:
        assert n >= 0 and last < 0.999e-10, (key, n, last)  # converged, and not by a margin that rounding could move
    return n


@pytest.mark.parametrize("variant", ["default", "gather", "clamped"])
@pytest.mark.parametrize("Q,dc", bg.SINGLE)
def test_single_cases_are_finite_and_converge(orc, Q, dc, variant):
    t = bg.instance(Q, dc, clamp=variant == "clamped")
    if variant == "clamped":  # ten rows, one-hot from the start
        rows = bg.clamp_rows(t["cap"], t["rcap"])
        assert len(set(rows)) == 10 and sorted(t["deg"][rows])[:4] == [0, 0, 1, 1] and {32, 33, t["cap"], bg.hub_whole(t["cap"])} <= set(t["deg"][rows])
    _, ob = bg.oracle_of(orc, t, msg_form=variant == "gather")  # set_gather_mode(1): 1-step differences on every sweep
    if variant == "clamped":
        assert (ob.get_state()[0][rows, t["tc"][rows]] == 1.0).all()
    _finite_then_converges(ob, bg.SINGLE_DAMPS, ("single", Q, dc, variant))


@pytest.mark.parametrize("Q,dc", bg.COLOURED)
def test_coloured_cases_are_finite(orc, Q, dc):
    t = bg.instance(Q, dc)
    og, ob = bg.oracle_of(orc, t)
    colour = bg.structured_colouring(t, og.row_ptr, og.nbr)
    assert cm.is_proper(og.row_ptr, og.nbr, colour) and (colour[:t["ns"]] == 0).all() and (colour[t["N"] - 4:] == 0).all()
    nc, ns_, _, step = cm.plan(og.row_ptr, og.nbr, colour, 1.0)
    assert ns_ == nc and (step == colour).all()  # step_fraction 1: one step per class
    for k in range(3):
        d = cm.sweep(ob, step, 1.0)
        psi, msg = ob.get_state()
        assert np.isfinite(d) and np.isfinite(psi).all() and np.isfinite(msg).all(), k
    _, ob = bg.oracle_of(orc, t)
    _finite_then_converges(ob, (), ("coloured", Q, dc))


@pytest.mark.parametrize("Q,dc", bg.BATCH)
def test_batch_cases_are_finite_and_converge(orc, Q, dc):
    t = bg.instance(Q, dc)
    for r, ((cab, na), seed) in enumerate(zip(bg.three_params(t), bg.BATCH_SEEDS)):
        _, ob = bg.oracle_of(orc, t, True, seed, cab, na)
        _finite_then_converges(ob, bg.BATCH_DAMPS, ("batch", Q, dc, r))


@pytest.mark.parametrize("Q,dc,whole", bg.WIDE + [(bg.WIDE_CLAMPED_Q, 0, "clamped")])
def test_wide_cases_are_finite_and_converge(orc, Q, dc, whole):
    t = bg.instance(Q, dc, whole_trips=whole is True, clamp=whole == "clamped")
    _, ob = bg.oracle_of(orc, t, True)
    _finite_then_converges(ob, bg.WIDE_DAMPS, ("wide", Q, dc, whole))
