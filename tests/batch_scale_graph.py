"""TEST INFRASTRUCTURE - recipes that take a REPLICA BATCH beyond the first trip of its folds and the first row of its grids,
and the launch arithmetic of csrc/engine.hip (batch_reductions, batch_agreement) restated, so that every case can say on which
side of which threshold it sits. Never imported by the product; imports nothing from the engine.

The graphs are shard_boundary_graph.ring_pairs(N, half): a ring lattice (row i joined to i +- 1 .. i +- half) with a chord on
every fourth row - odd cycles, 2 half or 2 half + 1 edges a row, no hub row at any label count. The number of segments grows
with N, so a segment count is reached by choosing N: ring_size searches the smallest N (a multiple of 4) with a given count in
a capacity class, RING_N holds what it finds, and tests/test_batch_scale_cpu.py asserts the two against each other.

What the sizes are for (kernels of csrc/kernels_batch.h):
  256 / 257 / 513 segments   k_finalize_batch folds a replica's records with 256 threads: one whole trip, one record more, a
                             third trip of one record, each at the replica's offset into the records
  64 / 65 / 128 / 129        k_fold_batch over the frame pass's rows (segments + hub rows): lanes stride the rows by 64
  N = 2048 / 2052            exact non-edge term: a g x g grid with g = 8 / 9, 64 / 81 rows in its fold
  N = 4096 / 4100            field refresh: 1 / 2 chunks of 4096 rows a replica (k_psi_sum_batch, k_field_refresh_batch); at
                             4100 also multi-start EM, where one replica leaves the mask of the reductions first
  N = 32 772                 above the exact / series switch: the automatic series with 65 rows in the fold of k_moments_batch
  N = 16 384, half 8         270 336 directed edges: k_em_edges_batch at its cap of 1024 workgroups, the first 32 of which
                             take a second trip of the grid-stride loop"""
import numpy as np

import boundary_graph as bg
from shard_boundary_graph import ring_pairs

# ---------------------------------------------------------------------------------------------------------------------
# the constants of the launches (tests/test_batch_scale_cpu.py reads them out of the two source files)
# ---------------------------------------------------------------------------------------------------------------------
BLOCK = 256            # threads of the reduction kernels; records a trip of fold_rows takes
FOLD_LANES = 64        # k_fold_batch: one wave per column, lanes stride the rows
FIELD_ROWS = 4096      # rows per workgroup of k_psi_sum_batch
MOMENT_ROWS = 512      # rows per workgroup of k_moments_batch
EDGE_GRID_CAP = 1024   # most workgroups of k_em_edges_batch
EM_FRAME_QMAX = 8      # above it the EM numerators come from k_em_edges_batch
EXACT_MAX_N = 32768    # automatic non-edge mode: exact up to here, the moment series above
AG_V, AG_TPB, AG_MAXN, AG_CPMAX = 32, 256, 128, 256
AG_GRID = 1024
AG_PART_BUDGET = 8 << 20  # doubles


def launch_model(N, E2, n_blk, n_hub, Q):
    """the grids and fold lengths of batch_reductions and batch_launch_sweep (csrc/engine.hip) for a graph of N rows, E2
    directed edges, n_blk segments (hub rows included, as stats().n_blocks counts them) and n_hub hub rows"""
    nbf = max(1, (N + FIELD_ROWS - 1) // FIELD_ROWS)
    rows = n_blk + n_hub
    blocks = max(1, (E2 + BLOCK - 1) // BLOCK)
    nbe = min(EDGE_GRID_CAP, blocks)
    g = (N + BLOCK - 1) // BLOCK
    nbm = max(1, (N + MOMENT_ROWS - 1) // MOMENT_ROWS)
    trips = lambda n, per: (n + per - 1) // per
    return dict(nbf=nbf, rows=rows, nbe=nbe, g=g, nbm=nbm,
                em_edges=Q > EM_FRAME_QMAX,                 # k_em_edges_batch runs at all
                edge_capped=blocks > EDGE_GRID_CAP,         # the cap decides the grid
                edge_blocks_twice=max(0, blocks - nbe),     # workgroups whose grid-stride loop has a thread with a second trip
                finalize_trips=trips(n_blk, BLOCK),         # fold_rows in k_finalize_batch
                frame_fold_trips=trips(rows, FOLD_LANES),   # k_fold_batch over the frame pass
                exact_fold_trips=trips(g * g, FOLD_LANES),  # ... over k_nonedge_exact_batch's grid
                moment_fold_trips=trips(nbm, FOLD_LANES),   # ... over k_moments_batch
                edge_fold_trips=trips(nbe, FOLD_LANES),     # ... over k_em_edges_batch
                exact_auto=N <= EXACT_MAX_N)


def series_order_model(Q, N, cab, requested=0):
    """host_reduce.h series_order at beta = 1 (w = cab): the lowest order whose truncation error is below 1e-12, at most the
    highest order the moment kernel holds (4 up to Q = 8, 3 up to 16)"""
    kmax, T, sz = 0, 0, 1
    while kmax < 4 and T + sz * Q <= 5120:
        sz *= Q
        T += sz
        kmax += 1
    if requested > 0:
        return min(requested, kmax)
    wmax = max(float((N * (1.0 - (1.0 - np.asarray(cab) / N))).max()), float(np.max(cab)))
    return next((K for K in range(1, kmax + 1) if N * (wmax / N) ** (K + 1) / (2.0 * (K + 1)) < 1e-12), kmax)


def agree_plan(n, Q):
    """the launch of k_agree for n listed replicas of Q labels (batch_agreement): dict with CT (16-wide column tiles), TPW
    (accumulator tiles per wave), tile_rows (tile rows per workgroup row), split (tile rows of every workgroup row: the last
    one ragged), S (row stride of the staged image in doubles: the one of CP and CP + 16 that is 16 mod 32) and LN (label
    bytes per vertex)"""
    nQ = n * Q
    assert 1 <= n <= AG_MAXN and nQ <= AG_CPMAX
    CT = (nQ + 15) // 16
    CP = 16 * CT
    TPW = 1 if CT * CT <= 4 else (4 if CT * CT <= 16 else 16)
    tile_rows = min(CT, (AG_TPB // 64) * TPW // CT)
    gy = (CT + tile_rows - 1) // tile_rows
    split = tuple(min(tile_rows, CT - y * tile_rows) for y in range(gy))
    S = CP if CP & 16 else CP + 16
    return dict(CT=CT, CP=CP, TPW=TPW, tile_rows=tile_rows, gy=gy, split=split, S=S, LN=(n + 7) & ~7, pad=CP - nQ)


def agree_gx_terms(N, CP, gy):
    """the three terms whose minimum is the number of workgroups along the vertices: four trips each, the launch's grid, the
    budget of the partial tables"""
    n_trips = max(1, (N + AG_V - 1) // AG_V)
    return (n_trips + 3) // 4, AG_GRID // gy, AG_PART_BUDGET // (CP * CP)


def agree_gx(N, CP, gy):
    return max(1, min(agree_gx_terms(N, CP, gy)))


# the (n, Q) cases of tests/test_gpu_agreement.py test_every_tile_shape_against_the_model; with the seven cases that file
# had before (AGREE_BEFORE) they reach every CT from 1 to 16
AGREE_BEFORE = [(1, 2), (3, 5), (4, 4), (3, 6), (8, 4), (5, 13), (16, 16)]
AGREE = [(3, 11), (3, 16), (7, 7), (4, 16), (6, 16), (7, 16), (9, 14), (8, 16), (43, 3), (9, 16), (10, 16), (11, 16), (12, 16),
         (13, 16), (14, 16), (15, 16), (17, 15), (85, 3), (128, 2)]
AGREE_BUDGET = (20011, 16, 16)  # (N, n, Q): the budget term decides gx


# ---------------------------------------------------------------------------------------------------------------------
# rings
# ---------------------------------------------------------------------------------------------------------------------
def ring_counts(N, half, cap, rcap):
    """(segments, hub rows) of ring_pairs(N, half) in a capacity class, by the segment model"""
    deg = bg.degrees(ring_pairs(N, half), N)
    bounds, hubs = bg.segment_model(deg, cap, rcap)
    return len(bounds) - 1, len(hubs)


def ring_size(cap, rcap, half, segments):
    """the smallest N (a multiple of 4) at which ring_pairs(N, half) has `segments` segments in the class (cap, rcap)"""
    count = lambda n: ring_counts(n, half, cap, rcap)[0]
    # a segment holds at most cap edges and a row has 2 half + 1/2 on average: start a tenth below segments cap / (2 half + 1/2)
    N = max(8 * half + 8, 4 * int(0.9 * segments * cap / (2 * half + 0.5) / 4))
    assert count(N) < segments
    while count(N) < segments:
        N += 4 * 16
    N -= 4 * 16
    while count(N) < segments:
        N += 4
    return N


# (cap, rcap, half, segments) -> N, as ring_size finds it (asserted by tests/test_batch_scale_cpu.py)
RING_N = {
    (128, 64, 1, 256): 13008, (128, 64, 1, 257): 13060, (128, 64, 1, 513): 26116,
    (512, 256, 4, 256): 15304, (512, 256, 4, 257): 15364,
    # the fold rings, in the class of Q = 12 and in that of Q = 5 (twice the capacities: twice the rows)
    (128, 64, 1, 64): 3216, (128, 64, 1, 65): 3268, (128, 64, 1, 128): 6480, (128, 64, 1, 129): 6532,
    (256, 128, 1, 64): 6428, (256, 128, 1, 65): 6532, (256, 128, 1, 128): 12956, (256, 128, 1, 129): 13060,
}
DENSE = dict(N=16384, half=8, segments=2341, E2=270336)  # at (128, 64)
FOLD_ROWS = (64, 65, 128, 129)

_GRAPHS = {}


def graph(N, half, cap, rcap):
    """ring_pairs(N, half) once per process, with its degrees and its segment plan in the class; the arrays are read-only"""
    key = (N, half, cap, rcap)
    if key not in _GRAPHS:
        pairs = ring_pairs(N, half)
        deg = bg.degrees(pairs, N)
        for x in (pairs, deg):
            x.setflags(write=False)
        bounds, hubs = bg.segment_model(deg, cap, rcap)
        _GRAPHS[key] = dict(pairs=pairs, N=N, half=half, deg=deg, E2=2 * len(pairs), n_blocks=len(bounds) - 1, hubs=hubs,
                            hub_edges=int(deg[hubs].sum()) if hubs else 0)
    return _GRAPHS[key]


# With boundary_graph.params the ring of degree 2 contracts by about a factor 3 per sweep. The lattices of 8 and 16 neighbours
# do not: at Q = 3 and 4 the oracle wanders for 400 sweeps (differences of 0.01 .. 0.2 at the end). There the contrast of cab
# about its mean is scaled by 0.15, at which the oracle converges in 15 .. 17 sweeps (0.5: not at all; 0.35: 85 .. 235; 0.25:
# 32 .. 41). The ring of 16 neighbours carries EM steps after three sweeps only and need not converge; at full contrast almost
# every vertex takes one label there (expected group sizes of 0.1 .. 16 000), at 0.15 the replicas are within 1e-3 of each
# other after the three sweeps; at 0.5 the group sizes spread over 30 .. 10 000 and the replicas are 0.07 .. 0.19 apart.
CONTRAST = {1: 1.0, 4: 0.15, 8: 0.5}  # by `half`


def params(Q, N, dc, pairs, half):
    cab, na, tc = bg.params(Q, N, dc, pairs)
    if CONTRAST[half] != 1.0:
        cab = cab.mean() + (cab - cab.mean()) * CONTRAST[half]
    return cab, na, tc


def instance(Q, dc, N, half):
    """a case on ring_pairs(N, half) in the capacity class of Q, parameters and true labels as params()"""
    cap, rcap = bg.caps_for(Q)
    gr = graph(N, half, cap, rcap)
    cab, na, tc = params(Q, N, dc, gr["pairs"], half)
    t = dict(gr, Q=Q, dc=dc, cap=cap, rcap=rcap, cab=cab, na=na, tc=tc, flag=0, conf=None, seed=Q)
    t["launch"] = launch_model(N, gr["E2"], gr["n_blocks"], len(gr["hubs"]), Q)
    return t


def segments_instance(Q, dc, segments):
    """the ring of `segments` segments in the class of Q (half = cap / 128, as the shard rings: 64 rows fill a segment)"""
    cap, rcap = bg.caps_for(Q)
    half = max(1, cap // 128)
    return instance(Q, dc, RING_N[(cap, rcap, half, segments)], half)


def fold_instance(Q, dc, rows):
    """the ring of degree 2 (half 1) on which the frame pass of the class of Q writes `rows` rows"""
    cap, rcap = bg.caps_for(Q)
    return instance(Q, dc, RING_N[(cap, rcap, 1, rows)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_batch_scale.py; tests/test_batch_scale_cpu.py checks each of them on the CPU
# ---------------------------------------------------------------------------------------------------------------------
R = 3
SWEEP = [(Q, dc, s) for Q, dc in ((9, 0), (9, 1), (16, 0)) for s in (256, 257, 513)] + [(Q, dc, s) for Q, dc in ((3, 0), (4, 2)) for s in (256, 257)]
SINGLE_ENGINE = (9, 1, 257, 1)  # (Q, dc, segments, replica): the case and replica that is also compared with a single engine
CALLS = ((2, 0.7), (2, 1.0))    # boundary_graph.BATCH_DAMPS as two calls of two sweeps
assert tuple(d for n, d in CALLS for _ in range(n)) == bg.BATCH_DAMPS
CONVERGE_SWEEPS = 400
COLOURED = [(9, dc, n) for dc in (0, 1) for n in (256, 257)]  # on coloured_step_graph.ring(n), R = 2
SERIES_K = 3  # the forced order of the dc 0 fold cases: the highest every label count up to 16 has

# (c) one EM step: (name, Q, dc, non-edge mode, forced order); mode 0 automatic, 1 exact, 2 series
EM_FOLD = [(Q, dc, rows) for Q in (5, 12) for dc in (0, 1) for rows in FOLD_ROWS]
EM_FIELD = [(3, 1, 4096), (3, 1, 4100)]
EM_EXACT = [(3, 0, 2048), (3, 0, 2052)]
EM_SERIES = [(4, 0, 32772)]
EM_DENSE = [(9, 1), (16, 1), (12, 2)]


# The mask of the reductions: sbmbp_batch_em_step takes none, the learning loop passes one (the replicas that still learn). On
# the two-chunk ring at Q = 3, dc 1 the oracle's synchronous learning (criterion 1e-6, rate 0.2, every BP run converged) takes
# 54 / 55 / 56 EM steps from cab scaled by 1 / 0.6 / 0.3 and 50 from 1.5: the replica started at 1.5 leaves the mask first.
LEARN_CASE = (3, 1, 4100)
LEARN_ARGS = (1e-6, 100, 0.2, 1.0)  # criterion, limit, learning rate, damping
LEARN_SCALES = (1.0, 0.6, 0.3)
LEARN_EARLY = 1.5
LEARN_FIRST_OUT = (0, 1)  # the replica that takes LEARN_EARLY in place of its scale


def em_instance(kind, Q, dc, size):
    """(instance, non-edge mode, forced series order) of an EM case"""
    if kind == "fold":
        return fold_instance(Q, dc, size), (2 if dc == 0 else 0), (SERIES_K if dc == 0 else 0)
    if kind == "exact":
        return instance(Q, dc, size, 1), 1, 0
    if kind == "dense":
        return instance(Q, dc, DENSE["N"], DENSE["half"]), 0, 0
    return instance(Q, dc, size, 1), 0, 0  # "field", "series": automatic


def perturbed(state, seed, rel=1e-13):
    """a state (marginals, messages) with every entry moved by a relative `rel` at most"""
    rng = np.random.default_rng(seed)
    return tuple(x * (1.0 + rel * rng.uniform(-1.0, 1.0, x.shape)) for x in state)
