"""TEST INFRASTRUCTURE - one deterministic graph recipe that puts rows and segments ON the thresholds of the sweep and
reduction kernels (segments). Never imported by the product.

The kernels work on segments: consecutive rows packed greedily by segment_plan (csrc/host_graph.cpp) until an edge capacity
CAP or a row capacity RCAP is reached; a row above CAP is a hub row, updated in fragments of 256 edges. caps_for and
segment_model RESTATE those rules (they import nothing from the engine), so a change of CAP, RCAP or the packing shows as a
disagreement between the model and stats() instead of a silent loss of coverage."""
import numpy as np

FRAG = 256  # edges per hub fragment


def caps_for(Q):
    """(CAP, RCAP) of label count Q"""
    if Q <= 4:
        return 512, 256
    if Q <= 8:
        return 256, 128
    if Q <= 16:
        return 128, 64
    return 64, 16


CLASSES = [(512, 256), (256, 128), (128, 64), (64, 16)]


def segment_model(deg, cap, rcap):
    """segment_plan without chunks: (row boundaries of the segments, hub rows). A hub row closes the open segment and is a
    segment of its own; otherwise a row opens a new segment when it would be row rcap + 1 or bring the edges above cap."""
    bounds, hubs = [0], []
    rows = edges = 0
    for i, d in enumerate(int(x) for x in deg):
        if d > cap:
            if rows:
                bounds.append(i)
            hubs.append(i)
            bounds.append(i + 1)
            rows = edges = 0
            continue
        if rows + 1 > rcap or edges + d > cap:
            bounds.append(i)
            rows = edges = 0
        rows += 1
        edges += d
    if bounds[-1] != len(deg):
        bounds.append(len(deg))
    return bounds, hubs


def step_segment_model(deg, rows, cap, rcap):
    """the segments of one step of the coloured order (csrc/host_graph.cpp coloured_step_tables) over `rows` (ascending): hub
    rows are set aside WITHOUT closing the open segment. Returns (list of row lists, hub rows)."""
    segs, hubs, cur, edges = [], [], [], 0
    for i in rows:
        d = int(deg[i])
        if d > cap:
            hubs.append(int(i))
            continue
        if len(cur) + 1 > rcap or edges + d > cap:
            segs.append(cur)
            cur, edges = [], 0
        cur.append(int(i))
        edges += d
    if cur:
        segs.append(cur)
    return segs, hubs


def step_plan_model(deg, step, cap, rcap, frag=FRAG):
    """the tables of the whole coloured order (csrc/host_graph.cpp coloured_step_tables) from the step of every row:
    step_segment_model step by step. Segments and hubs are numbered over all steps; loff holds per segment the edge offset of
    each row inside it and then its edge total (so segment b's block starts at loff[seg_row0[b] + b]); a hub's record is the
    number of segments of its step plus its index among the step's hubs; seg0 / hub0 / frag0 are the first segment, hub and
    fragment of every step (n_steps + 1 entries); max_rec = the most records (segments + hubs) of a step, at least 1."""
    step = np.asarray(step, dtype=np.int64)
    n_steps = int(step.max()) + 1 if len(step) else 0
    t = dict(rows=[], loff=[], seg_row0=[0], hub_row=[], hub_rec=[], frag_hub=[], hub_frag0=[0], seg0=[0], hub0=[0], frag0=[0], max_rec=1)
    order = np.argsort(step, kind="stable")
    first = np.searchsorted(step[order], np.arange(n_steps + 1))
    for s in range(n_steps):
        segs, hubs = step_segment_model(deg, order[first[s]:first[s + 1]], cap, rcap)
        for seg in segs:
            e = 0
            for i in seg:
                t["rows"].append(i)
                t["loff"].append(e)
                e += int(deg[i])
            t["loff"].append(e)
            t["seg_row0"].append(len(t["rows"]))
        for k, h in enumerate(hubs):
            t["hub_rec"].append(len(segs) + k)
            t["frag_hub"] += [len(t["hub_row"])] * (-(-int(deg[h]) // frag))
            t["hub_row"].append(h)
            t["hub_frag0"].append(len(t["frag_hub"]))
        t["max_rec"] = max(t["max_rec"], len(segs) + len(hubs))
        t["seg0"].append(len(t["seg_row0"]) - 1)
        t["hub0"].append(len(t["hub_row"]))
        t["frag0"].append(len(t["frag_hub"]))
    return t


STEP_TABLES = ("rows", "loff", "seg_row0", "hub_row", "hub_rec", "frag_hub", "hub_frag0", "seg0", "hub0", "frag0")


def hub_whole(cap):
    """a hub of whole fragments: two if that is a hub at this capacity, else three"""
    return 2 * FRAG if 2 * FRAG > cap + 1 else 3 * FRAG


BLOCKS = ("smallest_hub", "full_row", "two_rows_fill", "both_caps", "no_edges", "row_limit_first", "row_lengths", "hub_fragments")


def boundary_blocks(cap, rcap):
    """the structured rows block by block: [(name, degrees)]. Every block but the second begins with a separator row of
    cap + 1 edges - a hub, and a hub closes the open segment - so every block starts on a segment boundary."""
    sep = [cap + 1]
    return [
        ("smallest_hub", [cap + 1]),                                  # row 0: fragments of 256 edges plus one short one
        ("full_row", [cap]),                                          # one row fills a segment
        ("two_rows_fill", sep + [cap - 1, 1, 2]),                     # two rows fill a segment exactly; the third opens a new one
        ("both_caps", sep + [cap // rcap] * rcap + [1]),              # both capacities are reached by the same row
        ("no_edges", sep + [0] * (rcap + 1)),                         # rcap rows without a single edge, and one more row
        ("row_limit_first", sep + [1] * rcap + [cap - rcap + 1]),     # the row limit far below the edge limit; the next row would overflow the edges
        ("row_lengths", sep + [32, 33, 31, 8, 9, 7]),                 # BIG_ROW / FT_D and the renormalisation period
        ("hub_fragments", sep + [hub_whole(cap), 3 * FRAG + 1, 3 * FRAG - 1]),  # whole fragments, one edge more, one less
    ]


def boundary_degrees(cap, rcap, drop=None):
    """degree sequence of the structured rows in row order; drop = name of a block to leave out (the CPU test shows that every
    block is needed)"""
    out = []
    for name, d in boundary_blocks(cap, rcap):
        if name != drop:
            out += d
    return out


def build(cap, rcap, pool=900, whole_trips=False, drop=None, seed=77):
    """(pairs, N, number of structured rows). Structured row i takes its d_i neighbours round-robin from `pool` vertices placed
    after the structured rows: distinct neighbours, and no two structured rows adjacent. After the pool: three isolated rows,
    then one more hub row of cap + 1 edges as the last row. About 2 pool random pool-pool pairs (no self-loops, no repeats)
    make the graph non-bipartite. whole_trips: the number of directed edges is a multiple of 64 (the default one is not:
    k_wem takes 64 edges per trip), by leaving out trailing random pairs."""
    deg = boundary_degrees(cap, rcap, drop)
    ns = len(deg)
    N = ns + pool + 4
    assert max(deg) <= pool
    src, dst, cursor = [], [], 0
    for i, d in list(enumerate(deg)) + [(N - 1, cap + 1)]:
        src.append(np.full(d, i, dtype=np.int64))
        dst.append(ns + (cursor + np.arange(d, dtype=np.int64)) % pool)
        cursor = (cursor + d) % pool
    fixed = np.stack([np.concatenate(src), np.concatenate(dst)], 1)
    rng = np.random.default_rng(seed)
    ab = rng.integers(0, pool, size=(2 * pool, 2))
    ab = ab[ab[:, 0] != ab[:, 1]]
    ab = np.sort(ab, 1)
    _, first = np.unique(ab[:, 0] * pool + ab[:, 1], return_index=True)
    ab = ab[np.sort(first)] + ns  # no repeats, in the order drawn
    n = len(ab)
    if whole_trips:
        while (len(fixed) + n) % 32:
            n -= 1
    elif (len(fixed) + n) % 32 == 0:
        n -= 1
    pairs = np.concatenate([fixed, ab[:n]]).astype(np.uint32)
    return pairs, N, ns


def degrees(pairs, N):
    return np.bincount(np.asarray(pairs, dtype=np.int64).ravel(), minlength=N)


def params(Q, N, dc, pairs):
    """(cab, na, true_conf): true_conf = i % Q; cab symmetric, uniform(0.4, 1.6) plus 1.5 on the diagonal, divided by the
    squared mean degree under degree correction (as tests/test_gpu_fuzz.py); na from true_conf. (The seed is one at which no
    run of the reference ends within 1e-3 of the criterion: at 500 + Q the Q = 64, dc 1 run stopped on 0.9998e-10.)"""
    rng = np.random.default_rng(600 + Q)
    cab = rng.uniform(0.4, 1.6, size=(Q, Q))
    cab = (cab + cab.T) / 2 + np.eye(Q) * 1.5
    if dc:
        cab = cab / (2.0 * len(pairs) / N) ** 2
    tc = (np.arange(N) % Q).astype(np.uint32)
    na = np.bincount(tc, minlength=Q).astype(np.uint32)
    return cab, na, tc


def named_rows(cap, rcap):
    """row indices of the structured rows the clamped variants pin: {name: row}"""
    out, at = {}, 0
    for name, d in boundary_blocks(cap, rcap):
        if name == "full_row":
            out["cap_row"] = at
        elif name == "both_caps":
            out["rcap_first"], out["rcap_last"] = at + 1, at + rcap
        elif name == "no_edges":
            out["zero_first"], out["zero_last"] = at + 1, at + rcap
        elif name == "row_limit_first":
            out["ones_first"], out["ones_last"] = at + 1, at + rcap
        elif name == "row_lengths":
            out["d32"], out["d33"] = at + 1, at + 2
        elif name == "hub_fragments":
            out["hub_whole"] = at + 1
        at += len(d)
    return out


def conditions(deg, cap, rcap, ns=None):
    """what the segment model finds on a degree sequence: {name: bool}, one entry per threshold case. ns: count the row
    lengths among the first ns rows only (the structured ones; a pool vertex may have 7, 8 or 9 edges by chance)"""
    deg = np.asarray(deg, dtype=np.int64)
    bounds, hubs = segment_model(deg, cap, rcap)
    hubset = set(hubs)
    shapes, inside, pairs_of_rows = set(), set(), set()
    for a, b in zip(bounds[:-1], bounds[1:]):
        if a in hubset:
            continue
        shapes.add((b - a, int(deg[a:b].sum())))
        if b - a == 2:
            pairs_of_rows.add((int(deg[a]), int(deg[a + 1])))
        inside.update(int(d) for d in deg[a:min(b, len(deg) if ns is None else ns)])
    hd = sorted(int(deg[h]) for h in hubs)
    out = {
        "segment (1, cap)": (1, cap) in shapes,
        "segment (2, cap)": (cap - 1, 1) in pairs_of_rows,  # (at cap = 64 the rows of 33 and 31 edges fill a segment as well)
        "segment (rcap, cap)": (rcap, cap) in shapes,
        "segment (rcap, 0)": (rcap, 0) in shapes,
        "segment (rcap, rcap)": (rcap, rcap) in shapes,
        "row 0 is a hub of cap + 1": bool(len(deg)) and int(deg[0]) == cap + 1 and 0 in hubset,
        "last row is a hub of cap + 1": bool(len(deg)) and int(deg[-1]) == cap + 1 and (len(deg) - 1) in hubset,
        "hub of whole fragments": hub_whole(cap) in hd,
        "hub of whole fragments + 1": 3 * FRAG + 1 in hd,
        "hub of whole fragments - 1": 3 * FRAG - 1 in hd,
        "adjacent hubs": any(h + 1 in hubset for h in hubs),
    }
    for d in (31, 32, 33, 7, 8, 9):
        out["degree %d in a segment" % d] = d in inside
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_boundary.py; tests/test_boundary_cpu.py checks on the CPU that the oracle stays finite and
# converges on every one of them
# ---------------------------------------------------------------------------------------------------------------------
SINGLE = [(Q, dc) for Q in (2, 3, 4, 5, 8, 9, 16) for dc in (0, 1)] + [(Q, 2) for Q in (2, 5, 9)]
COLOURED = [(Q, dc) for Q in (2, 7, 13) for dc in (0, 1)]
BATCH = [(Q, 2 if Q in (4, 8) else (1 if Q % 3 == 0 else 0)) for Q in range(2, 17)]
WIDE = [(Q, dc, whole) for Q in (17, 33, 64) for dc in (0, 1) for whole in (False, True)]
WIDE_CLAMPED_Q = 33
BATCH_SEEDS = (3, 4, 5)
BATCH_SCALES = (1.0, 1.1, 0.85)  # as tests/test_gpu_batch_learn.py: three different (cab, na)
SINGLE_DAMPS = (0.7, 0.7, 1.0, 1.0, 1.0)  # as tests/test_gpu_label_counts.py
BATCH_DAMPS = (0.7, 0.7, 1.0, 1.0)        # as tests/test_gpu_batch.py
WIDE_DAMPS = (0.7, 0.7, 1.0, 1.0)         # as tests/test_gpu_wide.py
# Cases whose reference run does not converge within 600 sweeps at 1e-10 (the GPU test may then only require that both sides
# report -1): none. tests/test_boundary_cpu.py fails if a case belongs here and is not listed, or is listed and converges.
NOT_CONVERGING = {}

_GRAPHS = {}


def graph(cap, rcap, whole_trips=False):
    """build(cap, rcap) once per process; the arrays are read-only"""
    key = (cap, rcap, bool(whole_trips))
    if key not in _GRAPHS:
        pairs, N, ns = build(cap, rcap, whole_trips=whole_trips)
        pairs.setflags(write=False)
        deg = degrees(pairs, N)
        deg.setflags(write=False)
        bounds, hubs = segment_model(deg, cap, rcap)
        _GRAPHS[key] = dict(pairs=pairs, N=N, ns=ns, deg=deg, n_blocks=len(bounds) - 1, hubs=hubs, hub_edges=int(deg[hubs].sum()))
    return _GRAPHS[key]


def clamp_rows(cap, rcap):
    """the rows the clamped variants pin: the row of cap edges, one hub row, the first and the last row of the three blocks
    of rcap rows, the rows of 32 and 33 edges"""
    r = named_rows(cap, rcap)
    return sorted(r[k] for k in ("cap_row", "hub_whole", "rcap_first", "rcap_last", "zero_first", "zero_last", "ones_first", "ones_last", "d32", "d33"))


def instance(Q, dc, whole_trips=False, clamp=False):
    cap, rcap = caps_for(Q)
    gr = graph(cap, rcap, whole_trips)
    cab, na, tc = params(Q, gr["N"], dc, gr["pairs"])
    conf = None
    if clamp:
        conf = np.full(gr["N"], -1, dtype=np.int32)
        rows = clamp_rows(cap, rcap)
        conf[rows] = tc[rows]
    return dict(gr, Q=Q, dc=dc, cap=cap, rcap=rcap, cab=cab, na=na, tc=tc, flag=1 if clamp else 0, conf=conf, seed=Q)


def three_params(t):
    """tests/test_gpu_batch_learn.py _three_params: cab scaled, r vertices moved from the first group to the last"""
    out = []
    for r, s in enumerate(BATCH_SCALES):
        na = t["na"].astype(np.int64).copy()
        na[0] -= r
        na[-1] += r
        out.append((t["cab"] * s, na.astype(np.uint32)))
    return out


def oracle_of(orc, t, msg_form=False, seed=None, cab=None, na=None):
    og = orc.Graph.from_edges(t["pairs"], t["N"])
    ob = orc.OracleBP(og, t["Q"], t["dc"])
    ob.init_messages(t["flag"], t["conf"], t["tc"], orc.Rng(t["seed"] if seed is None else seed))
    ob.set_params(t["cab"] if cab is None else cab, t["na"] if na is None else na, 1.0)
    if msg_form:
        ob.set_msg_form(True)
    return og, ob


def structured_colouring(t, row_ptr, nbr):
    """a caller's colouring for the coloured order: every structured row (and the isolated rows and the last hub row) in class
    0 - an independent set by construction -, the pool coloured greedily from 1 in row order"""
    N, ns = t["N"], t["ns"]
    colour = np.zeros(N, dtype=np.int64)
    colour[ns:N - 4] = -1
    for i in range(ns, N - 4):
        taken = {int(colour[l]) for l in nbr[int(row_ptr[i]):int(row_ptr[i + 1])]}
        colour[i] = next(c for c in range(1, N + 1) if c not in taken)
    return colour
