"""The shard recipes (tests/shard_boundary_graph.py) checked on the CPU, before tests/test_gpu_shard_boundary.py relies on them:
every section of a recipe is a rank of the partition; every named condition shows in a named case, rank and chunk of every
capacity class, by the plan model and the chunked segment model alone, and disappears when its block is left out; the chunked
segment model equals the C++ segment_plan on the rows of every rank (tests/sanitize/host_sanitize.cpp, built with the
sanitizers); the rings have 64, 65 and 129 segments on rank 0 and are the smallest that do; and on every case of the GPU file
the oracle stays finite over the compared sweeps and converges."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plan_model as pm
import shard_boundary_graph as sg
from boundary_graph import caps_for, segment_model
from conftest import ROOT, gpath


def test_chunked_model_on_hand_worked_tables():
    """cap 4, rcap 3: the tables of tests/sanitize/host_sanitize.cpp test_segment_plan, and without chunks the unchunked model"""
    deg = [1, 1, 1, 1, 5, 1]
    for chunks, blk, cblk, chub in [([0, 6], [0, 3, 4, 5, 6], [0, 4], [0, 1]),
                                    ([0, 2, 6], [0, 2, 4, 5, 6], [0, 1, 4], [0, 0, 1]),      # a boundary inside a would-be segment
                                    ([0, 0, 6], [0, 3, 4, 5, 6], [0, 0, 4], [0, 0, 1]),      # an empty leading chunk
                                    ([0, 6, 6], [0, 3, 4, 5, 6], [0, 4, 4], [0, 1, 1]),      # an empty trailing chunk
                                    ([0, 4, 5, 6], [0, 3, 4, 5, 6], [0, 2, 3, 4], [0, 0, 1, 1]),  # boundaries around the hub
                                    ([0, 4, 4, 5, 6], [0, 3, 4, 5, 6], [0, 2, 2, 3, 4], [0, 0, 0, 1, 1])]:  # an empty chunk inside
        assert sg.chunked_segment_model(deg, 4, 3, chunks) == (blk, [4], cblk, chub), chunks
    rng = np.random.default_rng(5)
    for _ in range(20):
        d = rng.choice([0, 1, 2, 3, 4, 5, 9], size=int(rng.integers(1, 40)))
        blk, hubs, cblk, chub = sg.chunked_segment_model(d, 4, 3, [0, len(d)])
        assert (blk, hubs) == segment_model(d, 4, 3) and cblk == [0, len(blk) - 1] and chub == [0, len(hubs)]


@pytest.mark.parametrize("world", [2, 3, 4, 5])
@pytest.mark.parametrize("cap,rcap", sg.CLASSES)
def test_every_section_is_a_rank(cap, rcap, world):
    g = sg.graph(cap, rcap, world)
    assert g["N"] < 20000 and len(g["names"]) == g["N"]
    bounds = pm.partition_rows(g["row_ptr"], world)
    assert list(bounds[:-1]) == g["row0"] and bounds[-1] == g["N"]
    w = np.add.reduceat(g["deg"] + 2, bounds[:-1])
    assert w.max() - w.min() <= 10, w  # equal weights, up to the padding's step
    print("cap %d world %d: N %d, %d directed edges, rows per rank %s" % (cap, world, g["N"], 2 * len(g["pairs"]), list(np.diff(bounds))))


# where every condition shows: (world, n_chunks, rank), the same in every capacity class. The chunk is read off the model
# and printed; for the conditions made by one row it is asserted below.
WHERE = {
    "segment with 2 rcap send slots": [(3, 1, 1), (3, 4, 1), (4, 4, 1)],
    "segment with 2 rcap - 1 send slots": [(3, 1, 1), (4, 1, 1)],
    "segment (rcap, 0) without a send slot in a rank > 0": [(3, 1, 1), (4, 1, 1)],
    "segment (1, cap) in a rank > 0": [(3, 1, 1), (4, 1, 1)],
    "plain row read by every other rank": [(3, 1, 1), (3, 4, 1)],
    "hub row read by every other rank": [(3, 1, 1), (3, 4, 1), (5, 4, 2)],
    "hub first row of a rank > 0": [(3, 1, 1), (4, 4, 1), (5, 4, 2)],
    "hub last row of a rank": [(3, 1, 1), (3, 4, 1), (5, 4, 2)],
    "hub first row of a chunk > 0": [(2, 4, 0)],
    "hub last row of an inner chunk": [(2, 4, 0)],
    "hub with halo neighbours only": [(2, 4, 0), (3, 1, 1), (5, 4, 2)],
    "hub fragment boundary between own and halo neighbours": [(2, 1, 0), (2, 4, 0)],
    "rank of one hub row, three empty chunks": [(5, 4, 2)],
    "chunk boundary closes an open segment": [(3, 4, 0), (4, 4, 0)],
    "chunk with more than 8 segments, no multiple of 8": [(3, 1, 0), (4, 1, 0)],
    "chunk with 1 to 7 segments": [(2, 4, 0), (5, 4, 0)],
    "empty chunk between two others": [(2, 4, 0)],
    "rank without an edge": [(4, 1, 3), (4, 4, 3)],
    "two ranks with edges exchange nothing": [(3, 1, 0), (3, 4, 0), (4, 4, 0)],
}
_found = {}


def _conditions(cap, rcap, world, n_chunks):
    key = (cap, rcap, world, n_chunks)
    if key not in _found:
        g = sg.graph(cap, rcap, world)
        _found[key] = sg.conditions(g["row_ptr"], g["nbr"], world, n_chunks, cap, rcap)
    return _found[key]


@pytest.mark.parametrize("cap,rcap", sg.CLASSES)
def test_every_condition_shows_in_its_named_case(cap, rcap):
    assert set(WHERE) == set(sg.CONDITIONS)
    for name, places in WHERE.items():
        for world, n_chunks, rank in places:
            assert (world, n_chunks) in sg.LAYOUTS
            hits = [x for x in _conditions(cap, rcap, world, n_chunks)[name] if x[0] == rank]
            assert hits, (name, "world %d, %d chunks, rank %d" % (world, n_chunks, rank))
            print("cap %d: %s: world %d, %d chunks, rank %d, chunk %s" % (cap, name, world, n_chunks, rank, sorted({x[1] for x in hits})))
    # every committed layout shows something no layout with fewer ranks or chunks shows in that rank
    for world, n_chunks in sg.LAYOUTS:
        assert any((world, n_chunks) == p[:2] for places in WHERE.values() for p in places)
    # the chunks of the conditions that one row makes (world 2, four chunks): chunk 0 ends with the hub M, chunk 1 is empty,
    # chunk 2 is the hub M2 alone, chunk 3 the leaves behind it
    f = _conditions(cap, rcap, 2, 4)
    assert (0, 1) in f["empty chunk between two others"] and (0, 2) in f["hub first row of a chunk > 0"]
    assert {(0, 0), (0, 2)} <= set(f["hub last row of an inner chunk"]) and (0, 0) in f["hub fragment boundary between own and halo neighbours"]
    # the exchange-free pair of three ranks is the two pools; with a fourth rank the row that all peers read cannot exist
    assert (0, 2) in _conditions(cap, rcap, 3, 1)["two ranks with edges exchange nothing"]
    assert not _conditions(cap, rcap, 4, 1)["hub row read by every other rank"] and not _conditions(cap, rcap, 4, 1)["plain row read by every other rank"]


def test_per_rank_counts_of_the_committed_cases():
    """segments, hub rows and hub edges of every rank, as DESIGN.md section 5 quotes them"""
    for cap, rcap in sg.CLASSES:
        for world, n_chunks in sg.LAYOUTS:
            g = sg.graph(cap, rcap, world)
            _, ranks = sg.rank_models(g["row_ptr"], g["nbr"], world, n_chunks, cap, rcap)
            print("cap %d world %d chunks %d: segments %s, hub rows %s, hub edges %s, send slots of the fullest segment %d"
                  % (cap, world, n_chunks, [m["n_blocks"] for m in ranks], [m["n_hub_rows"] for m in ranks], [m["hub_edges"] for m in ranks],
                     max(int(np.diff(m["plan"].snd_ptr.astype(np.int64)[m["blk"]]).max(initial=0)) for m in ranks)))
            for m in ranks:  # no segment has more send slots than the kernel's list holds (CAP = 2 RCAP: one slot per cut edge)
                hub = set(m["hubs"])
                per_seg = np.diff(m["plan"].snd_ptr.astype(np.int64)[m["blk"]])
                assert all(s <= 2 * rcap for a, s in zip(m["blk"], per_seg) if a not in hub)


# what each block is there for: without it exactly these (condition, rank) pairs are gone from the case, looking at EVERY rank
NEEDS = {
    (3, 1, "head_sep"): {("hub first row of a rank > 0", 1)},
    (3, 1, "tail_sep"): {("hub last row of a rank", 1)},
    (3, 1, "full_slots"): {("segment with 2 rcap send slots", 1)},
    (3, 1, "almost_full_slots"): {("segment with 2 rcap - 1 send slots", 1)},
    (3, 1, ("full_slots", "almost_full_slots")): {("segment with 2 rcap send slots", 1), ("segment with 2 rcap - 1 send slots", 1),
                                                  ("plain row read by every other rank", 1)},
    (3, 1, "no_slots"): {("segment (rcap, 0) without a send slot in a rank > 0", 1), ("segment (1, cap) in a rank > 0", 1)},
    (3, 1, "all_peers"): {("hub row read by every other rank", 1)},
    (3, 1, "pool_gap"): {("two ranks with edges exchange nothing", 0)},
    (4, 1, "empty_rank"): {("rank without an edge", 3)},
    (4, 4, "empty_rank"): {("rank without an edge", 3)},
    (2, 4, "mid_hub"): {("hub fragment boundary between own and halo neighbours", 0), ("hub first row of a chunk > 0", 0)},  # (M2 alone still spans two cuts)
    (2, 4, "next_hub"): {("hub first row of a chunk > 0", 0), ("hub with halo neighbours only", 0)},
    (2, 4, ("mid_hub", "next_hub")): {("hub fragment boundary between own and halo neighbours", 0), ("hub first row of a chunk > 0", 0),
                                      ("hub with halo neighbours only", 0), ("hub last row of an inner chunk", 0), ("empty chunk between two others", 0)},
    (5, 4, "lone_hub"): {("rank of one hub row, three empty chunks", 2), ("hub row read by every other rank", 2), ("hub first row of a rank > 0", 2),
                         ("hub last row of a rank", 2), ("hub with halo neighbours only", 2)},
}
# The three conditions that the chunk cuts make, not a block of rows: each is absent from every rank of a sibling layout of
# the same recipe - a boundary can close a segment only where there is one (one chunk: none); a chunk of more than 8 segments
# needs a rank of more than 8 (the five-rank layout has at most 8 a rank, in four chunks); a chunk of 1 to 7 segments is not
# found where the only chunk is a rank of 13 segments or more.
ABSENT = {
    "chunk boundary closes an open segment": [(2, 1), (3, 1), (4, 1)],
    "chunk with more than 8 segments, no multiple of 8": [(5, 4), (2, 4)],
    "chunk with 1 to 7 segments": [(3, 1), (4, 1)],
}


def test_every_condition_has_a_negative_control():
    controlled = {name for lost in NEEDS.values() for name, _ in lost} | set(ABSENT)
    assert controlled == set(sg.CONDITIONS)
    assert {b for w, _, d in NEEDS for b in ((d,) if isinstance(d, str) else d)} == {b for bl in sg.BLOCKS.values() for b in bl}
    with pytest.raises(ValueError):
        sg.build(128, 64, 5, drop="full_slots")  # a block the layout does not have is refused, not ignored


@pytest.mark.parametrize("world,n_chunks,drop", list(NEEDS))
@pytest.mark.parametrize("cap,rcap", sg.CLASSES)
def test_a_dropped_block_loses_its_named_conditions(cap, rcap, world, n_chunks, drop):
    pairs, N, _, _ = sg.build(cap, rcap, world, drop=drop)
    row_ptr, nbr = sg.csr(pairs, N)
    got = sg.conditions(row_ptr, nbr, world, n_chunks, cap, rcap)
    here = lambda f: {(k, x[0]) for k, v in f.items() for x in v}  # (condition, rank) over all ranks
    lost = here(_conditions(cap, rcap, world, n_chunks)) - here(got)
    assert lost == NEEDS[(world, n_chunks, drop)], (lost, here(got) - here(_conditions(cap, rcap, world, n_chunks)))
    for name, rank in lost:  # and each was in the full case where WHERE says
        assert (world, n_chunks, rank) in WHERE[name] or any(x[0] == rank for x in _conditions(cap, rcap, world, n_chunks)[name])


@pytest.mark.parametrize("cap,rcap", sg.CLASSES)
def test_chunk_made_conditions_are_absent_from_their_sibling_layouts(cap, rcap):
    for name, layouts in ABSENT.items():
        assert any(_conditions(cap, rcap, w, c)[name] for w, c, _ in WHERE[name])
        for world, n_chunks in layouts:
            assert (world, n_chunks) in sg.LAYOUTS and not _conditions(cap, rcap, world, n_chunks)[name], (name, world, n_chunks)


@pytest.mark.parametrize("segments", [64, 65, 129])
@pytest.mark.parametrize("cap,rcap", sg.CLASSES)
def test_rings_have_the_segments_the_fold_needs(cap, rcap, segments):
    g = sg.ring_graph(cap, rcap, segments)
    N = g["N"]
    assert N < 20000 and N % 4 == 0
    got = sg.ring_segments(N, cap, rcap)
    assert got[0] == segments and sg.ring_segments(N - 4, cap, rcap)[0] < segments  # exactly, and the smallest ring
    _, ranks = sg.rank_models(g["row_ptr"], g["nbr"], 2, 1, cap, rcap)
    assert [m["n_blocks"] for m in ranks] == got and not any(m["n_hub_rows"] for m in ranks)
    # the stride of the fold over this rank's partials (ceil(segments / 64)): 1, 2, 3
    assert -(-segments // sg.FOLD_ROWS) == {64: 1, 65: 2, 129: 3}[segments]
    deg = g["deg"]
    assert set(deg) == {cap // 64, cap // 64 + 1, cap // 64 + 2} or set(deg) == {cap // 64, cap // 64 + 1}
    assert (deg > cap // 64).sum() >= N // 4  # a fourth of the rows carry chords (and the rows they reach)
    cut = (np.searchsorted(pm.partition_rows(g["row_ptr"], 2), g["nbr"], side="right") - 1) != np.repeat(np.arange(N) >= ranks[0]["plan"].n_own, deg)
    print("ring cap %d, %d segments: N %d, segments per rank %s, %d cut edges" % (cap, segments, N, got, cut.sum()))
    assert cut.sum() >= N // 8


def test_chunked_model_equals_segment_plan_under_the_sanitizers(tmp_path):
    """host_sanitize.cpp --chunk-plans reads `cap rcap n n_chunks n_bounds n_hubs`, degrees, chunk boundaries, segment
    boundaries, hub rows, chunk_blk, chunk_hub per plan and compares segment_plan(..., chunk_row, ...) with it: the rows of
    every rank of every committed case, every recipe also under each class's capacities other than its own, and the rings"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    plans = []
    for cap, rcap in sg.CLASSES:
        for world, n_chunks in sg.LAYOUTS + [(3, 2)]:
            g = sg.graph(cap, rcap, world)
            for c2, r2 in ([(cap, rcap)] if (cap, rcap) != (128, 64) else sg.CLASSES):  # (the label-count test runs the (128, 64) recipe in every class)
                for m in sg.rank_models(g["row_ptr"], g["nbr"], world, n_chunks, c2, r2)[1]:
                    plans.append((c2, r2, m["plan"].deg, m["plan"].chunk_row, m["blk"], m["hubs"], m["chunk_blk"], m["chunk_hub"]))
        for segments in (64, 65, 129):
            g = sg.ring_graph(cap, rcap, segments)
            for n_chunks in (1, 3):
                for m in sg.rank_models(g["row_ptr"], g["nbr"], 2, n_chunks, cap, rcap)[1]:
                    plans.append((cap, rcap, m["plan"].deg, m["plan"].chunk_row, m["blk"], m["hubs"], m["chunk_blk"], m["chunk_hub"]))

    def write(path, plans):
        with open(path, "w") as f:
            for cap, rcap, deg, chunks, blk, hubs, cblk, chub in plans:
                f.write("%d %d %d %d %d %d\n" % (cap, rcap, len(deg), len(chunks) - 1, len(blk), len(hubs)))
                for v in (deg, chunks, blk, hubs, cblk, chub):
                    f.write(" ".join(str(int(x)) for x in v) + "\n")

    path = tmp_path / "chunk_plans.txt"
    write(path, plans)
    exe = tmp_path / "host_sanitize"
    src = [os.path.join(ROOT, "tests", "sanitize", "host_sanitize.cpp"), os.path.join(ROOT, "sbm-bp_amd", "csrc", "host_graph.cpp"),
           os.path.join(ROOT, "oracle", "bp_oracle.cpp")]
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-mavx2", "-pthread",
                    "-o", str(exe)] + src, check=True, timeout=600)
    env = dict(os.environ, TMPDIR=str(tmp_path), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--chunk-plans", str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert pr.returncode == 0 and "host_sanitize ok: %d chunked plans" % len(plans) in pr.stdout, (pr.stdout[-500:], pr.stderr[-3000:])
    assert "runtime error" not in pr.stderr and "AddressSanitizer" not in pr.stderr and "LeakSanitizer" not in pr.stderr
    # a chunk table that is off by one segment, and a boundary that is off by one row, are refused
    for field in (6, 4):
        bad = [list(plans[1])]
        bad[0][field] = list(bad[0][field])
        bad[0][field][1] += 1
        write(tmp_path / "bad.txt", bad)
        pr = subprocess.run([str(exe), gpath("c1_dataset.edgelist"), "--chunk-plans", str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=600, env=env)
        assert pr.returncode != 0 and "plan 0" in pr.stderr, (field, pr.stderr[-500:])


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU file: the reference is finite over the compared sweeps and converges
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(orc, t, msg_form=False):
    og = orc.Graph.from_edges(t["pairs"], t["N"])
    assert np.array_equal(og.row_ptr, t["row_ptr"]) and np.array_equal(og.nbr, t["nbr"])  # the recipe's CSR is the oracle's
    ob = orc.OracleBP(og, t["Q"], t["dc"])
    ob.init_messages(t["flag"], t["conf"], t["tc"], orc.Rng(t["seed"]))
    ob.set_params(t["cab"], t["na"], 1.0)
    if msg_form:
        ob.set_msg_form(True)
    return ob


def _finite_then_converges(ob, damps, key):
    for k, damp in enumerate(damps):
        d = ob.sweep_sync(damp)
        psi, msg = ob.get_state()
        assert np.isfinite(d) and np.isfinite(psi).all() and np.isfinite(msg).all(), (key, k)
    n, last = ob.converge_sync(1e-10, 600, 1.0)
    print("%s: converge_sync niter %d, last %.3g" % (key, n, last))
    if key in sg.NOT_CONVERGING:
        assert n < 0, (key, "is listed as not converging, but converges")
    else:
        assert n >= 0 and last < 0.999e-10, (key, n, last)  # converged, and not by a margin that rounding could move


@pytest.mark.parametrize("world", [2, 3, 4, 5])
@pytest.mark.parametrize("Q,dc", sg.THRESHOLD)
def test_threshold_cases_are_finite_and_converge(orc, Q, dc, world):
    _finite_then_converges(_oracle(orc, sg.instance(Q, dc, world)), sg.DAMPS, ("threshold", Q, dc, world))


@pytest.mark.parametrize("Q", sg.CLAMPED_Q)
def test_clamped_cases_are_finite_and_converge(orc, Q):
    t = sg.instance(Q, 0, 3, clamp=True)
    rows = sg.clamp_rows(t)
    assert len(set(rows)) == 10 and {0, 2, t["cap"], t["cap"] + 1, sg.BIG_HUB} <= set(t["deg"][rows])
    ob = _oracle(orc, t, msg_form=True)  # on shards a clamped run takes the message-gather form throughout
    assert (ob.get_state()[0][rows, t["tc"][rows]] == 1.0).all()
    _finite_then_converges(ob, sg.DAMPS, ("clamped", Q, 0, 3))


def test_gather_case_is_finite_and_converges(orc):
    _finite_then_converges(_oracle(orc, sg.instance(8, 1, 3), msg_form=True), sg.DAMPS, ("gather", 8, 1, 3))


@pytest.mark.parametrize("Q", [Q for Q in sg.KNOB_Q + (9,) if (Q, 1) not in sg.THRESHOLD])
def test_knob_cases_are_finite_and_converge(orc, Q):
    _finite_then_converges(_oracle(orc, sg.instance(Q, 1, 3)), sg.DAMPS, ("threshold", Q, 1, 3))


@pytest.mark.parametrize("Q,dc", sg.LABELS)
def test_label_count_cases_are_finite(orc, Q, dc):
    t = sg.instance(Q, dc, 3, cls=(128, 64))
    ob = _oracle(orc, t)
    for k, damp in enumerate(sg.DAMPS[1:]):
        d = ob.sweep_sync(damp)
        assert np.isfinite(d) and all(np.isfinite(x).all() for x in ob.get_state()), (Q, dc, k)
    # a hub row in a rank other than 0 at the capacities of this label count
    _, ranks = sg.rank_models(t["row_ptr"], t["nbr"], 3, 2, *caps_for(Q))
    assert ranks[1]["n_hub_rows"] > 0


@pytest.mark.parametrize("Q,segments,clamp", sg.FOLD)
def test_fold_cases_are_finite(orc, Q, segments, clamp):
    t = sg.instance(Q, 0, 2, clamp=clamp, ring=segments)
    ob = _oracle(orc, t, msg_form=clamp)
    for k in range(4):
        d = ob.sweep_sync(1.0)
        assert np.isfinite(d) and d > 1e-6 and all(np.isfinite(x).all() for x in ob.get_state()), (Q, segments, k)  # still moving
