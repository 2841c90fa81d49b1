"""TEST INFRASTRUCTURE - caller's colourings that put the step tables of the coloured order (csrc/host_graph.cpp
coloured_step_tables; kernels k_sweep_step, k_hub_step_cavity, k_hub_frag_product_msg, k_step_finalize) ON their thresholds in
steps other than the first. Never imported by the product; imports nothing from the engine.

The graphs are the boundary graphs of tests/boundary_graph.py (structured rows block by block, a pool, three isolated rows, a
last hub row), one per capacity class below Q = 17. The layouts:

  last    the pool coloured greedily from 0; then one class per block of boundary_blocks (its separator hub included), one for
          the three isolated rows, one for the last hub row; step_fraction 1. Every block is a step of its own far behind step
          0: its segments start at seg_base > 0, its hub writes the record behind them, every hub but the first has earlier
          hubs and fragments before it. The sweep ends on a step of one hub and no segment.
  first   the same classes before the pool: step 0 is the block smallest_hub, one hub and no segment.
  cut     boundary_graph.structured_colouring (all structured rows in class 0, the pool greedily from 1) with a step_fraction
          that makes steps of B = RCAP rows: the cuts fall inside runs of rows that one step would pack into one segment. The
          tail of class 1 is a class of its own (one_row_tail), so that class 1 has a multiple of RCAP rows and one more.
  ring    at (128, 64): a ring of degree 2, 2 n0 + 1 rows coloured 0 1 0 1 ... 0 1 2, so class 0 has n0 = 256 * 64 or 257 * 64
          rows = 256 or 257 segments of RCAP rows and CAP edges in one step (k_step_finalize folds the step's records with 256
          threads)."""
import math

import numpy as np

import boundary_graph as bg
from boundary_graph import FRAG

CLASSES = bg.CLASSES[:3]  # (512, 256), (256, 128), (128, 64)
LAYOUTS = ("last", "first", "cut")
RING_RECORDS = (256, 257)


def csr(pairs, N):
    """(row_ptr, nbr) with ascending neighbours in every row, as the engine's and the oracle's graph builders give it"""
    p = np.asarray(pairs, dtype=np.int64)
    src, dst = np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]])
    order = np.lexsort((dst, src))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int64)
    return row_ptr, dst[order]


def block_rows(cap, rcap, drop=None):
    """[(name, first row, one past the last row)] of the structured blocks in row order"""
    out, at = [], 0
    for name, d in bg.boundary_blocks(cap, rcap):
        if name != drop:
            out.append((name, at, at + len(d)))
            at += len(d)
    return out


def _greedy_pool(colour, row_ptr, nbr, lo, hi, base):
    """rows lo .. hi - 1 in row order take the smallest colour >= base that no neighbour holds"""
    for i in range(lo, hi):
        taken = {int(colour[l]) for l in nbr[int(row_ptr[i]):int(row_ptr[i + 1])]}
        colour[i] = next(c for c in range(base, len(colour) + base + 1) if c not in taken)


def block_colouring(N, ns, row_ptr, nbr, blocks, blocks_first):
    """one class per block, one for the isolated rows, one for the last hub row; the pool greedily, before or behind them"""
    colour = np.full(N, -1, dtype=np.int64)
    nb = len(blocks) + 2
    if blocks_first:
        base = 0
        _greedy_pool(colour, row_ptr, nbr, ns, N - 4, nb)
    else:
        _greedy_pool(colour, row_ptr, nbr, ns, N - 4, 0)
        base = int(colour.max()) + 1
    for k, (_, a, b) in enumerate(blocks):
        colour[a:b] = base + k
    colour[N - 4:N - 1] = base + len(blocks)
    colour[N - 1] = base + len(blocks) + 1
    return colour


def cut_fraction(N, rcap):
    """a step_fraction whose B = max(1, ceil(step_fraction N)) is rcap: step_fraction N = rcap - 1/2, half a row away from
    either neighbour of the ceiling, where the rounding of the product (relative 2^-52) cannot reach"""
    f = (rcap - 0.5) / N
    assert math.ceil(f * N) == rcap and abs(f * N - (rcap - 0.5)) < 1e-6
    return f


def one_row_tail(colour, c, B):
    """the last rows of class c moved to a new last class of their own (rows of one class: still independent), as many as
    leave class c with one row more than a multiple of B: its last step then holds a single row. (No class of
    structured_colouring has such a size in any capacity class.)"""
    rows = np.flatnonzero(colour == c)
    move = (len(rows) - 1) % B
    assert len(rows) - move > B
    colour = colour.copy()
    if move:
        colour[rows[len(rows) - move:]] = colour.max() + 1
    return colour


def plan(colour, step_fraction):
    """tests/coloured_model.py plan for a given colouring: (n_colours, n_steps, step[N])"""
    colour = np.asarray(colour, dtype=np.int64)
    N = len(colour)
    B = max(1, math.ceil(step_fraction * N))
    step, n_steps = np.zeros(N, dtype=np.int64), 0
    for c in range(int(colour.max()) + 1):
        rows = np.flatnonzero(colour == c)
        step[rows] = n_steps + np.arange(len(rows)) // B
        n_steps += (len(rows) + B - 1) // B
    return int(colour.max()) + 1, n_steps, step


def build(cap, rcap, layout, drop=None):
    """the layout on the boundary graph of this class (drop = a block left out of the graph): dict with the graph, its CSR,
    the colouring, step_fraction, the plan and the model's step tables"""
    pairs, N, ns = bg.build(cap, rcap, drop=drop)
    deg = bg.degrees(pairs, N)
    row_ptr, nbr = csr(pairs, N)
    blocks = block_rows(cap, rcap, drop)
    assert blocks[-1][2] == ns
    if layout == "cut":
        colour = one_row_tail(bg.structured_colouring(dict(N=N, ns=ns), row_ptr, nbr), 1, rcap)
        fraction = cut_fraction(N, rcap)
    else:
        colour = block_colouring(N, ns, row_ptr, nbr, blocks, layout == "first")
        fraction = 1.0
    nc, n_steps, step = plan(colour, fraction)
    bounds, hubs = bg.segment_model(deg, cap, rcap)
    return dict(pairs=pairs, N=N, ns=ns, deg=deg, row_ptr=row_ptr, nbr=nbr, blocks=blocks, colour=colour, fraction=fraction, n_colours=nc,
                n_steps=n_steps, step=step, tables=bg.step_plan_model(deg, step, cap, rcap), cap=cap, rcap=rcap, layout=layout,
                n_blocks=len(bounds) - 1, hubs=hubs, hub_edges=int(deg[hubs].sum()))


def ring(records, cap=128, rcap=64):
    """the ring whose class 0 is one step of `records` segments of rcap rows"""
    assert cap == 2 * rcap  # rcap rows of two edges fill a segment exactly
    n0 = records * rcap
    N = 2 * n0 + 1
    a = np.arange(N, dtype=np.int64)
    pairs = np.stack([a, (a + 1) % N], 1).astype(np.uint32)
    colour = a % 2
    colour[N - 1] = 2
    deg = bg.degrees(pairs, N)
    row_ptr, nbr = csr(pairs, N)
    nc, n_steps, step = plan(colour, 1.0)
    bounds, hubs = bg.segment_model(deg, cap, rcap)
    return dict(pairs=pairs, N=N, ns=0, deg=deg, row_ptr=row_ptr, nbr=nbr, blocks=[], colour=colour, fraction=1.0, n_colours=nc,
                n_steps=n_steps, step=step, tables=bg.step_plan_model(deg, step, cap, rcap), cap=cap, rcap=rcap, layout="ring%d" % records,
                n_blocks=len(bounds) - 1, hubs=hubs, hub_edges=0)


_LAYOUTS = {}


def layout(cap, rcap, name):
    """build / ring once per process; the arrays are read-only"""
    key = (cap, rcap, name)
    if key not in _LAYOUTS:
        L = ring(int(name[4:]), cap, rcap) if name.startswith("ring") else build(cap, rcap, name)
        for v in L.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _LAYOUTS[key] = L
    return _LAYOUTS[key]


# ---------------------------------------------------------------------------------------------------------------------
# what the model finds on a layout: {condition: sorted steps in which it shows}
# ---------------------------------------------------------------------------------------------------------------------
CONDITIONS = (
    "first step holds hubs and no segment", "last step holds hubs and no segment", "step whose only segment has no edge",
    "segment (1, cap) at seg_base > 0", "segment (2, cap) at seg_base > 0", "segment (rcap, cap) at seg_base > 0",
    "segment (rcap, 0) at seg_base > 0", "segment (rcap, rcap) before the overflowing row at seg_base > 0",
    "rows of 31, 32 and 33 edges at seg_base > 0", "rows of 7, 8 and 9 edges at seg_base > 0",
    "hub of one fragment at frag_first > 0", "hub of whole fragments at frag_first > 0", "hub of whole fragments + 1 at frag_first > 0",
    "hub of whole fragments - 1 at frag_first > 0", "hub record behind segments, earlier hubs before it",
    "cut inside a segment of the one-step plan", "class whose last step holds a single row", "step of 256 records", "step of 257 records",
)


def conditions(L):
    t, deg, cap, rcap, ns, step = L["tables"], L["deg"], L["cap"], L["rcap"], L["ns"], L["step"]
    out = {k: set() for k in CONDITIONS}
    n_steps = L["n_steps"]
    for s in range(n_steps):
        b0, b1, h0, h1 = t["seg0"][s], t["seg0"][s + 1], t["hub0"][s], t["hub0"][s + 1]
        nseg, nh = b1 - b0, h1 - h0
        segs = [t["rows"][t["seg_row0"][b]:t["seg_row0"][b + 1]] for b in range(b0, b1)]
        shape = [(len(r), int(deg[r].sum())) for r in segs]
        if nseg == 0 and nh and s == 0:
            out["first step holds hubs and no segment"].add(s)
        if nseg == 0 and nh and s == n_steps - 1:
            out["last step holds hubs and no segment"].add(s)
        if nseg == 1 and shape[0][1] == 0:
            out["step whose only segment has no edge"].add(s)
        if nseg + nh == 256:
            out["step of 256 records"].add(s)
        if nseg + nh == 257:
            out["step of 257 records"].add(s)
        if b0 > 0:
            for k, (r, sh) in enumerate(zip(segs, shape)):
                d = [int(deg[i]) for i in r]
                if sh == (1, cap):
                    out["segment (1, cap) at seg_base > 0"].add(s)
                if d == [cap - 1, 1]:
                    out["segment (2, cap) at seg_base > 0"].add(s)
                if sh == (rcap, cap):
                    out["segment (rcap, cap) at seg_base > 0"].add(s)
                if sh == (rcap, 0):
                    out["segment (rcap, 0) at seg_base > 0"].add(s)
                if sh == (rcap, rcap) and k + 1 < nseg and int(deg[segs[k + 1][0]]) + rcap > cap:  # the next row fails BOTH tests
                    out["segment (rcap, rcap) before the overflowing row at seg_base > 0"].add(s)
                mine = {int(deg[i]) for i in r if i < ns}  # (a pool row may have 7, 8 or 9 edges by chance)
                if {31, 32, 33} <= mine:
                    out["rows of 31, 32 and 33 edges at seg_base > 0"].add(s)
                if {7, 8, 9} <= mine:
                    out["rows of 7, 8 and 9 edges at seg_base > 0"].add(s)
        for h in range(h0, h1):
            d, f0 = int(deg[t["hub_row"][h]]), t["hub_frag0"][h]
            assert t["hub_rec"][h] == nseg + h - h0
            if f0 > 0:
                if d <= FRAG:
                    out["hub of one fragment at frag_first > 0"].add(s)
                if d == bg.hub_whole(cap):
                    out["hub of whole fragments at frag_first > 0"].add(s)
                if d == 3 * FRAG + 1:
                    out["hub of whole fragments + 1 at frag_first > 0"].add(s)
                if d == 3 * FRAG - 1:
                    out["hub of whole fragments - 1 at frag_first > 0"].add(s)
            if nseg > 0 and h0 > 0:
                out["hub record behind segments, earlier hubs before it"].add(s)
    # the cuts: two consecutive rows of a class in different steps that one step over the whole class packs into one segment
    colour = L["colour"]
    for c in range(L["n_colours"]):
        rows = np.flatnonzero(colour == c)
        seg_of = {}
        for k, seg in enumerate(bg.step_segment_model(deg, rows, cap, rcap)[0]):
            for i in seg:
                seg_of[i] = k
        plain = [int(i) for i in rows if int(i) in seg_of]
        for a, b in zip(plain[:-1], plain[1:]):
            if step[a] != step[b] and seg_of[a] == seg_of[b]:
                out["cut inside a segment of the one-step plan"].add(int(step[b]))
        last = int(step[rows[-1]])
        if int(step[rows[0]]) != last and (step == last).sum() == 1:
            out["class whose last step holds a single row"].add(last)
    return {k: sorted(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_coloured_step.py; tests/test_coloured_step_cpu.py checks on the CPU that the model is finite
# over the compared sweeps on every one, and which of the converge cases converge
# ---------------------------------------------------------------------------------------------------------------------
DAMPS = (0.7, 0.7, 1.0, 1.0)              # one call each; then as two calls of two sweeps
CALLS = ((2, 0.7), (2, 1.0))
LAST = list(bg.BATCH)                     # (a) every label count, dc rotating
OTHER = [(Q, dc) for Q in (2, 5, 9, 16) for dc in (0, 1)] + [(Q, 2) for Q in (2, 5, 9)]  # (b) on `first` and `cut`
CLAMPED_Q = (3, 8, 13)                    # (c)
RING = [(9, dc, n) for dc in (0, 1) for n in RING_RECORDS]  # (d)
CONVERGE = [(2, 0), (4, 1), (5, 0), (8, 1), (9, 0), (12, 1), (16, 0)]  # (e) on `last`: two or three per capacity class, dc 0 and 1
CONVERGE_SWEEPS = 400
# Cases of CONVERGE whose model run does not converge within 400 sweeps at 1e-10 (the GPU test then requires -1 of both
# sides). tests/test_coloured_step_cpu.py fails if a case belongs here and is not listed, or is listed and converges.
NOT_CONVERGING = set()


def instance(Q, dc, name, clamp=False):
    cap, rcap = (128, 64) if name.startswith("ring") else bg.caps_for(Q)
    L = layout(cap, rcap, name)
    cab, na, tc = bg.params(Q, L["N"], dc, L["pairs"])
    conf = None
    if clamp:
        conf = np.full(L["N"], -1, dtype=np.int32)
        rows = bg.clamp_rows(cap, rcap)
        conf[rows] = tc[rows]
    return dict(L, Q=Q, dc=dc, cab=cab, na=na, tc=tc, flag=1 if clamp else 0, conf=conf, seed=Q)


def plan_numbers(L, tables=None):
    """a layout as tests/sanitize/host_sanitize.cpp --step-plans reads it: cap rcap n n_steps max_rec, the lengths of the ten
    tables, the degrees, the step of every row, the tables"""
    t = L["tables"] if tables is None else tables
    out = [L["cap"], L["rcap"], L["N"], L["n_steps"], t["max_rec"]] + [len(t[k]) for k in bg.STEP_TABLES]
    for v in [L["deg"], L["step"]] + [t[k] for k in bg.STEP_TABLES]:
        out += [int(x) for x in v]
    return out
