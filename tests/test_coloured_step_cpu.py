"""The layouts of tests/coloured_step_graph.py checked on the CPU, before tests/test_gpu_coloured_step.py relies on them: every
colouring is proper; every named condition shows in a named layout and step of every capacity class, by the step-plan model
alone, and disappears when its block is left out or the sibling layout is taken; the model equals the C++
coloured_step_tables on every layout (tests/sanitize/host_sanitize.cpp --step-plans, built with the sanitizers); the rings have
steps of 256 and 257 records; the fast step of tests/coloured_model.py equals its row-by-row sweep; and on every case of the
GPU file the model stays finite over the compared sweeps, and the converge cases converge or are listed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import boundary_graph as bg
import coloured_model as cm
import coloured_step_graph as cg
from conftest import ROOT, gpath


def test_step_plan_model_on_a_hand_worked_case():
    """cap 4, rcap 3: the case of tests/sanitize/host_sanitize.cpp test_step_tables"""
    t = bg.step_plan_model([1, 5, 2, 2, 1, 0, 6, 1, 1], [1, 0, 1, 1, 1, 2, 0, 1, 1], 4, 3)
    assert t == dict(rows=[0, 2, 3, 4, 7, 8, 5], loff=[0, 1, 3, 0, 2, 3, 4, 0, 1, 0, 0], seg_row0=[0, 2, 5, 6, 7], hub_row=[1, 6], hub_rec=[0, 1],
                     frag_hub=[0, 1], hub_frag0=[0, 1, 2], seg0=[0, 0, 3, 4], hub0=[0, 2, 2, 2], frag0=[0, 2, 2, 2], max_rec=3)
    # one step over all rows is step_segment_model; a hub of 2 fragments + 1 edge
    deg = np.array([3, 600, 1, 4, 513, 2])
    t = bg.step_plan_model(deg, np.zeros(6, dtype=int), 4, 3)
    segs, hubs = bg.step_segment_model(deg, range(6), 4, 3)
    assert [t["rows"][a:b] for a, b in zip(t["seg_row0"][:-1], t["seg_row0"][1:])] == segs and t["hub_row"] == hubs
    assert t["hub_rec"] == [len(segs), len(segs) + 1] and t["hub_frag0"] == [0, 3, 6] and t["frag_hub"] == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("name", cg.LAYOUTS)
@pytest.mark.parametrize("cap,rcap", cg.CLASSES)
def test_every_layout_is_a_proper_colouring_of_the_boundary_graph(cap, rcap, name):
    L, g = cg.layout(cap, rcap, name), bg.graph(cap, rcap)
    assert np.array_equal(L["pairs"], g["pairs"]) and L["N"] == g["N"] and L["n_blocks"] == g["n_blocks"] and L["hubs"] == g["hubs"]
    assert cm.is_proper(L["row_ptr"], L["nbr"], L["colour"]) and L["colour"].min() == 0
    nc, ns, colour, step = cm.plan(L["row_ptr"], L["nbr"], L["colour"], L["fraction"])  # the plan of the model the engine is compared with
    assert (nc, ns) == (L["n_colours"], L["n_steps"]) and np.array_equal(step, L["step"])
    t, N, nst = L["tables"], L["N"], L["ns"]
    if name == "cut":
        B = np.bincount(step).max()
        assert B == rcap and ns > nc  # steps of RCAP rows
        assert (L["colour"][:nst] == 0).all() and (L["colour"][N - 4:] == 0).all()
    else:
        assert ns == nc and np.array_equal(step, L["colour"])  # one step per class
        first = name == "first"
        base = 0 if first else nc - 10
        for k, (_, a, b) in enumerate(L["blocks"]):
            assert (L["colour"][a:b] == base + k).all()
        assert (L["colour"][N - 4:N - 1] == base + 8).all() and L["colour"][N - 1] == base + 9
        pool = L["colour"][nst:N - 4]
        assert (pool >= 10).all() if first else (pool < base).all()
    print("cap %d %s: %d classes, %d steps, max_rec %d; (segments, hubs, fragments) per step %s"
          % (cap, name, nc, ns, t["max_rec"], [(t["seg0"][s + 1] - t["seg0"][s], t["hub0"][s + 1] - t["hub0"][s], t["frag0"][s + 1] - t["frag0"][s]) for s in range(ns)]))
    assert t["frag0"][-1] == sum(-(-int(L["deg"][h]) // 256) for h in L["hubs"])  # the engine's own fragment count (n_frag)


# where every condition shows: layout -> step, counted from the first block's step (`last`: the pool's classes come before
# it, as many as the greedy colouring needs; `first`: step 0) or, for the cut layout, the steps themselves per class
# (512, 256) / (256, 128) / (128, 64)
BLOCK_STEP = {name: k for k, name in enumerate(bg.BLOCKS)}  # + 8: the isolated rows, + 9: the last hub row
WHERE = {
    "first step holds hubs and no segment": [("first", "smallest_hub")],
    "last step holds hubs and no segment": [("last", 9)],
    "step whose only segment has no edge": [("last", 8), ("first", 8)],
    "segment (1, cap) at seg_base > 0": [("last", "full_row")],
    "segment (2, cap) at seg_base > 0": [("last", "two_rows_fill"), ("first", "two_rows_fill")],
    "segment (rcap, cap) at seg_base > 0": [("last", "both_caps"), ("first", "both_caps")],
    "segment (rcap, 0) at seg_base > 0": [("last", "no_edges"), ("first", "no_edges")],
    "segment (rcap, rcap) before the overflowing row at seg_base > 0": [("last", "row_limit_first"), ("first", "row_limit_first")],
    "rows of 31, 32 and 33 edges at seg_base > 0": [("last", "row_lengths"), ("first", "row_lengths")],
    "rows of 7, 8 and 9 edges at seg_base > 0": [("last", "row_lengths"), ("first", "row_lengths")],
    "hub of one fragment at frag_first > 0": [("last", "two_rows_fill"), ("last", 9), ("first", "two_rows_fill")],  # at (128, 64) only
    "hub of whole fragments at frag_first > 0": [("last", "hub_fragments"), ("first", "hub_fragments"), ("cut", 3)],
    "hub of whole fragments + 1 at frag_first > 0": [("last", "hub_fragments"), ("first", "hub_fragments"), ("cut", 3)],
    "hub of whole fragments - 1 at frag_first > 0": [("last", "hub_fragments"), ("first", "hub_fragments"), ("cut", 3)],
    "hub record behind segments, earlier hubs before it": [("last", "two_rows_fill"), ("last", "row_lengths"), ("first", "both_caps"), ("cut", 1)],
    "cut inside a segment of the one-step plan": [("cut", 1), ("cut", 2), ("cut", 3)],
    "class whose last step holds a single row": [("cut", {512: 5, 256: 6, 128: 9})],
    "step of 256 records": [("ring256", 0)],
    "step of 257 records": [("ring257", 0)],
}
_found = {}


def _conditions(cap, rcap, name):
    if (cap, rcap, name) not in _found:
        _found[(cap, rcap, name)] = cg.conditions(cg.layout(cap, rcap, name))
    return _found[(cap, rcap, name)]


def _step_of(L, where):
    if isinstance(where, dict):
        return where[L["cap"]]
    if L["layout"] in ("last", "first"):
        base = 0 if L["layout"] == "first" else L["n_colours"] - 10
        return base + (BLOCK_STEP[where] if isinstance(where, str) else where)
    return where


@pytest.mark.parametrize("cap,rcap", cg.CLASSES)
def test_every_condition_shows_in_its_named_layout_and_step(cap, rcap):
    assert set(WHERE) == set(cg.CONDITIONS)
    for cond, places in WHERE.items():
        for name, where in places:
            if name.startswith("ring") and cap != 128:
                continue
            if cond == "hub of one fragment at frag_first > 0" and cap != 128:  # a hub of CAP + 1 edges has one fragment at (128, 64) only
                assert not any(_conditions(cap, rcap, x)[cond] for x in cg.LAYOUTS)
                continue
            L = cg.layout(cap, rcap, name)
            s = _step_of(L, where)
            assert s in _conditions(cap, rcap, name)[cond], (cond, name, where, s, _conditions(cap, rcap, name)[cond])
            print("cap %d: %s: layout %s, step %d of %d" % (cap, cond, name, s, L["n_steps"]))
    # the block steps of `last` lie behind the pool's: every one has seg_base > 0, and from the second hub on frag_first and
    # the step's first hub are above 0
    L = cg.layout(cap, rcap, "last")
    t, base = L["tables"], L["n_colours"] - 10
    assert base >= 3 and t["seg0"][base] > 0 and t["hub0"][base] == 0 and t["hub0"][base + 1] == 1
    assert all(t["hub0"][s] > 0 and t["frag0"][s] > 0 for s in range(base + 1, L["n_steps"]))
    # every committed layout shows something
    for name in cg.LAYOUTS:
        assert any(name == p[0] for places in WHERE.values() for p in places)


# what each block is there for: without it exactly these conditions are gone from `last`
NEEDS = {
    "smallest_hub": set(),  # (every later hub still has the separators before it; its own condition is `first`'s step 0)
    "full_row": {"segment (1, cap) at seg_base > 0"},
    "two_rows_fill": {"segment (2, cap) at seg_base > 0"},
    "both_caps": {"segment (rcap, cap) at seg_base > 0"},
    "no_edges": {"segment (rcap, 0) at seg_base > 0"},
    "row_limit_first": {"segment (rcap, rcap) before the overflowing row at seg_base > 0"},
    "row_lengths": {"rows of 31, 32 and 33 edges at seg_base > 0", "rows of 7, 8 and 9 edges at seg_base > 0"},
    "hub_fragments": {"hub of whole fragments at frag_first > 0", "hub of whole fragments + 1 at frag_first > 0", "hub of whole fragments - 1 at frag_first > 0"},
}
# The conditions a layout makes, not a block of rows: each is absent from these sibling layouts of the same graph - `last`
# begins with the pool and `first` ends with it; every step of the cut layout that has a segment has rows with edges in it;
# a layout of one step per class has no cut, and no class of two steps; a hub record behind segments with earlier hubs needs
# a second hub (the ring has none); the ring of 256 records has no step of 257 and the other way round.
ABSENT = {
    "first step holds hubs and no segment": ["last", "cut"],
    "last step holds hubs and no segment": ["first", "cut"],
    "step whose only segment has no edge": ["cut"],
    "cut inside a segment of the one-step plan": ["last", "first"],
    "class whose last step holds a single row": ["last", "first"],
    "hub of one fragment at frag_first > 0": ["ring256"],
    "hub record behind segments, earlier hubs before it": ["ring256"],
    "step of 256 records": ["ring257", "last"],
    "step of 257 records": ["ring256", "last"],
}


def test_every_condition_has_a_negative_control():
    assert {c for lost in NEEDS.values() for c in lost} | set(ABSENT) == set(cg.CONDITIONS)
    assert set(NEEDS) == set(bg.BLOCKS)


@pytest.mark.parametrize("drop", bg.BLOCKS)
@pytest.mark.parametrize("cap,rcap", cg.CLASSES)
def test_a_dropped_block_loses_its_named_conditions(cap, rcap, drop):
    got = cg.conditions(cg.build(cap, rcap, "last", drop=drop))
    full = _conditions(cap, rcap, "last")
    lost = {k for k in cg.CONDITIONS if full[k] and not got[k]}
    assert lost == NEEDS[drop] and not {k for k in cg.CONDITIONS if got[k] and not full[k]}
    if drop == "smallest_hub":  # and `first` without it begins with the row of CAP edges: a segment in step 0
        assert not cg.conditions(cg.build(cap, rcap, "first", drop=drop))["first step holds hubs and no segment"]


@pytest.mark.parametrize("cap,rcap", cg.CLASSES)
def test_layout_made_conditions_are_absent_from_their_sibling_layouts(cap, rcap):
    for cond, layouts in ABSENT.items():
        for name in layouts:
            if name.startswith("ring") and cap != 128:
                continue
            assert not _conditions(cap, rcap, name)[cond], (cond, name)


@pytest.mark.parametrize("records", cg.RING_RECORDS)
def test_rings_have_a_step_of_256_and_of_257_records(records):
    L = cg.layout(128, 64, "ring%d" % records)
    t = L["tables"]
    assert (L["deg"] == 2).all() and cm.is_proper(L["row_ptr"], L["nbr"], L["colour"]) and L["n_colours"] == L["n_steps"] == 3
    assert (L["colour"] == 0).sum() == records * 64 and L["N"] % 2 == 1  # an odd cycle
    assert [t["seg0"][s + 1] - t["seg0"][s] for s in range(3)] == [records, records, 1] and t["max_rec"] == records and not t["hub_row"]
    assert all(t["seg_row0"][b + 1] - t["seg_row0"][b] == 64 and t["loff"][t["seg_row0"][b + 1] + b] == 128 for b in range(2 * records))
    # k_step_finalize folds a step's records with 256 threads: 256 records are one each, the 257th is the first second trip
    assert -(-records // 256) == {256: 1, 257: 2}[records]


def _all_plans():
    plans = []
    for cap, rcap in cg.CLASSES:
        for name in cg.LAYOUTS:
            plans.append(cg.layout(cap, rcap, name))
            if (cap, rcap) != (128, 64):  # (every label-count case runs at its own capacities only; the models of the others cost nothing)
                L = cg.layout(cap, rcap, name)
                plans.append(dict(L, cap=128, rcap=64, tables=bg.step_plan_model(L["deg"], L["step"], 128, 64)))
        for drop in bg.BLOCKS:
            plans.append(cg.build(cap, rcap, "last", drop=drop))
        for name in ("ring256", "ring257"):
            plans.append(cg.ring(int(name[4:]), cap, rcap))
    return plans


def test_step_plan_model_equals_coloured_step_tables_under_the_sanitizers(tmp_path):
    """host_sanitize.cpp --step-plans reads cap, rcap, degrees and the step of every row followed by the model's tables and
    requires coloured_step_tables to reproduce them: every layout and ring of every class, every layout also at the smallest
    capacities, blocks last also without each block; a file with one wrong entry is refused"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    plans = _all_plans()
    path = tmp_path / "step_plans.txt"
    with open(path, "w") as f:
        for L in plans:
            f.write(" ".join(str(x) for x in cg.plan_numbers(L)) + "\n")
    exe = tmp_path / "host_sanitize"
    src = [os.path.join(ROOT, "tests", "sanitize", "host_sanitize.cpp"), os.path.join(ROOT, "sbm-bp_amd", "csrc", "host_graph.cpp"),
           os.path.join(ROOT, "oracle", "bp_oracle.cpp")]
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-mavx2", "-pthread",
                    "-o", str(exe)] + src, check=True, timeout=600)
    env = dict(os.environ, TMPDIR=str(tmp_path), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--step-plans", str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert pr.returncode == 0 and "host_sanitize ok: %d step plans" % len(plans) in pr.stdout, (pr.stdout[-500:], pr.stderr[-3000:])
    assert "runtime error" not in pr.stderr and "AddressSanitizer" not in pr.stderr and "LeakSanitizer" not in pr.stderr
    # a hub record without the segments of its step before it, and a block of loff that starts one entry early, are refused
    L = cg.layout(128, 64, "last")
    for table, at in (("hub_rec", 3), ("loff", 70)):
        t = dict(L["tables"])
        t[table] = list(t[table])
        t[table][at] -= 1 if table == "hub_rec" else -1
        assert t[table] != L["tables"][table]
        with open(tmp_path / "bad.txt", "w") as f:
            f.write(" ".join(str(x) for x in cg.plan_numbers(L, t)) + "\n")
        pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--step-plans", str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=600, env=env)
        assert pr.returncode != 0 and "plan 0" in pr.stderr and table + " differs" in pr.stderr, (table, pr.stderr[-500:])
    # the tables the engine built before the construction moved (tests/sanitize/parent_step_tables.inc, compared by the
    # program's default run in tests/test_capi_cpu.py) are those of these two layouts: the model gives the same numbers
    text = open(os.path.join(ROOT, "tests", "sanitize", "parent_step_tables.inc")).read()
    recorded = [int(x) for line in text.splitlines() if not line.startswith("//") for x in line.replace(",", " ").split()]
    assert recorded == cg.plan_numbers(cg.layout(128, 64, "last")) + cg.plan_numbers(cg.layout(512, 256, "cut"))


# ---------------------------------------------------------------------------------------------------------------------
# the fast step of the model, and the conditions on the inputs of the GPU file
# ---------------------------------------------------------------------------------------------------------------------
# Per sweep. DESIGN.md section 2 compares the two restatements at 1e-14; these graphs have hub rows, and above 32 edges the
# synchronous sweep finishes a row in the log domain (a sum of hundreds of logarithms, so an absolute error of some 1e-13
# in the exponent), where node_update multiplies the factors as they are. Measured over two sweeps on the
# three layouts at Q = 2, 3, 4, 5, 6, 8, 9, 11, 13, 16 and every deg_corr_flag: at most 3.8e-13 (Q = 11, dc 2, cut; the
# messages of a hub row of 129 edges); with a margin of ten, 4e-12 over two sweeps.
FAST_TOL = 2e-12


@pytest.mark.parametrize("name", cg.LAYOUTS)
@pytest.mark.parametrize("Q,dc", [(3, 1), (6, 0), (11, 2)])  # one label count per capacity class, every deg_corr_flag
def test_fast_step_equals_the_row_by_row_sweep(orc, Q, dc, name):
    t = cg.instance(Q, dc, name)
    _, slow = bg.oracle_of(orc, t)
    _, fast = bg.oracle_of(orc, t)
    worst = 0.0
    for k, damp in enumerate((0.7, 1.0)):
        d1, d2 = cm.sweep(slow, t["step"], damp), cm.fast_sweep(fast, t["step"], damp)
        (p1, m1), (p2, m2) = slow.get_state(), fast.get_state()
        assert np.isfinite(p2).all() and np.isfinite(m2).all()
        worst = max(worst, np.abs(p1 - p2).max(), np.abs(m1 - m2).max(), abs(d1 - d2))
        assert worst <= FAST_TOL * (k + 1), (k, worst)
        assert np.abs(slow.h() - fast.h()).max() <= 1e-12 * max(1.0, np.abs(slow.h()).max())
    print("fast step, cap %d Q %d dc %d %s: largest difference from the row-by-row sweep over two sweeps %.3g" % (t["cap"], Q, dc, name, worst))


def _finite(ob, t, damps, key, clamped=None):
    for k, damp in enumerate(damps):
        d = cm.fast_sweep(ob, t["step"], damp, clamped)
        psi, msg = ob.get_state()
        assert np.isfinite(d) and d > 1e-6 and np.isfinite(psi).all() and np.isfinite(msg).all(), (key, k, d)  # finite and still moving


@pytest.mark.parametrize("Q,dc", cg.LAST)
def test_blocks_last_cases_are_finite(orc, Q, dc):
    t = cg.instance(Q, dc, "last")
    _finite(bg.oracle_of(orc, t)[1], t, cg.DAMPS, ("last", Q, dc))


@pytest.mark.parametrize("name", ["first", "cut"])
@pytest.mark.parametrize("Q,dc", cg.OTHER)
def test_blocks_first_and_cut_cases_are_finite(orc, Q, dc, name):
    t = cg.instance(Q, dc, name)
    _finite(bg.oracle_of(orc, t)[1], t, cg.DAMPS, (name, Q, dc))


@pytest.mark.parametrize("Q", cg.CLAMPED_Q)
def test_clamped_cases_are_finite(orc, Q):
    t = cg.instance(Q, 0, "last", clamp=True)
    rows = bg.clamp_rows(t["cap"], t["rcap"])
    assert len(set(rows)) == 10 and {0, 1, 32, 33, t["cap"], bg.hub_whole(t["cap"])} <= set(t["deg"][rows])
    # a clamped hub in a step of hubs alone, clamped rows first and last in the three segments of RCAP rows
    L = t["tables"]
    assert bg.named_rows(t["cap"], t["rcap"])["hub_whole"] in L["hub_row"]
    seg_ends = {L["rows"][L["seg_row0"][b]] for b in range(len(L["seg_row0"]) - 1)} | {L["rows"][L["seg_row0"][b + 1] - 1] for b in range(len(L["seg_row0"]) - 1)}
    assert {bg.named_rows(t["cap"], t["rcap"])[k] for k in ("rcap_first", "rcap_last", "zero_first", "zero_last", "ones_first", "ones_last")} <= seg_ends
    _, ob = bg.oracle_of(orc, t)
    psi0 = ob.get_state()[0]
    assert (psi0[rows, t["tc"][rows]] == 1.0).all()
    _finite(ob, t, cg.DAMPS, ("clamped", Q), t["conf"] != -1)
    assert np.array_equal(ob.get_state()[0][rows], psi0[rows])


@pytest.mark.parametrize("Q,dc,records", cg.RING)
def test_ring_cases_are_finite(orc, Q, dc, records):
    t = cg.instance(Q, dc, "ring%d" % records)
    _finite(bg.oracle_of(orc, t)[1], t, (1.0,) * 4, ("ring", Q, dc, records))


@pytest.mark.parametrize("Q,dc", cg.CONVERGE)
def test_converge_cases_converge_or_are_listed(orc, Q, dc):
    t = cg.instance(Q, dc, "last")
    _, ob = bg.oracle_of(orc, t)
    n, last = cm.converge(ob, t["step"], 1e-10, cg.CONVERGE_SWEEPS, 1.0, fast=True)
    print("converge, blocks last, cap %d Q %d dc %d: model niter %d, last %.3g" % (t["cap"], Q, dc, n, last))
    if (Q, dc) in cg.NOT_CONVERGING:
        assert n < 0, ((Q, dc), "is listed as not converging, but converges")
    else:
        assert n >= 0 and last < 0.999e-10, (Q, dc, n, last)  # converged, and not by a margin that rounding could move


def test_converge_cases_cover_every_class_and_degree_correction():
    left = [c for c in cg.CONVERGE if c not in cg.NOT_CONVERGING]
    assert {bg.caps_for(Q) for Q, _ in left} == set(cg.CLASSES) and any(dc == 1 for _, dc in left)
    assert set(cg.NOT_CONVERGING) <= set(cg.CONVERGE)
