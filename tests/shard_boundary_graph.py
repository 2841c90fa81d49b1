"""TEST INFRASTRUCTURE - deterministic graph recipes that put the rows of a SHARDED run on the edges of the shard kernels: full
and empty send-slot lists, hub rows on shard and chunk boundaries, empty chunks, ranks without edges, and a per-rank fold of 64,
65 and 129 segments. Never imported by the product.

The partition (plan_model.partition_rows) and the chunk cuts (plan_model.chunk_rows) balance sum(deg + 2). A recipe is a list
of sections, one per rank, padded to the same weight, so every section IS a rank; where the chunk cuts fall inside a rank is
never assumed: chunked_segment_model restates segment_plan (csrc/host_graph.cpp) WITH chunk boundaries, importing nothing from
the engine, and conditions() reads every named case off that model and the plan model of each rank.

Layouts (chosen by `world`; the capacity class (CAP, RCAP) sizes the structured rows):
  world 2  "mid"   rank 0 = 128 leaves | hub M | hub M2 | 128 leaves, rank 1 = the rows M and M2 read. M weighs more than a
                   quarter of its rank, so two chunk cuts fall behind it: an empty chunk between two others.
  world 3  "edge"  pool A | structured rows | pool B. A structured row takes its neighbours from the pools on both sides.
  world 4  "edge"  pool A | structured rows | pool B | isolated rows (a rank without an edge).
  world 5  "star"  leaves | leaves | ONE hub row | leaves | leaves: a rank that is one hub row (a row as heavy as a whole
                   rank needs three ranks' worth of neighbours, hence five ranks).
and ring(): a ring lattice with chords over two ranks, sized so that rank 0 has a given number of segments."""
import numpy as np

import plan_model as pm
from boundary_graph import BATCH, FRAG, caps_for, params, segment_model

CLASSES = sorted({caps_for(Q) for Q in range(2, 17)}, reverse=True)  # the capacity classes below Q = 17: (512, 256), (256, 128), (128, 64)
POOL = 800                                     # rows per pool
BIG_HUB = 2 * FRAG + 64                        # 576 edges: a hub row at every label count up to 16


def chunked_segment_model(deg, cap, rcap, chunk_row):
    """segment_plan with chunks: (blk_row, hub_row, chunk_blk, chunk_hub). As boundary_graph.segment_model, and a chunk
    boundary closes the open segment; chunk_blk / chunk_hub count the segments / hub rows before every chunk boundary."""
    chunk_row = [int(x) for x in chunk_row]
    n, n_chunks = len(deg), len(chunk_row) - 1
    blk, hubs, cblk, chub = [0], [], [0], [0]
    rows = edges = 0
    nxt = 1
    for i, d in enumerate(int(x) for x in deg):
        while nxt < n_chunks and i == chunk_row[nxt]:
            if rows:
                blk.append(i)
                rows = edges = 0
            cblk.append(len(blk) - 1)
            chub.append(len(hubs))
            nxt += 1
        if d > cap:
            if rows:
                blk.append(i)
            hubs.append(i)
            blk.append(i + 1)
            rows = edges = 0
            continue
        if rows + 1 > rcap or edges + d > cap:
            blk.append(i)
            rows = edges = 0
        rows += 1
        edges += d
    if blk[-1] != n:
        blk.append(n)
    while len(cblk) < n_chunks + 1:
        cblk.append(len(blk) - 1)
        chub.append(len(hubs))
    return blk, hubs, cblk, chub


# ---------------------------------------------------------------------------------------------------------------------
# assembling a graph from sections of equal weight
# ---------------------------------------------------------------------------------------------------------------------
class _Row:
    __slots__ = ("deg", "id", "name")

    def __init__(self, name=None):
        self.deg, self.id, self.name = 0, -1, name


class _Asm:
    def __init__(self):
        self.edges, self.cursor = [], {}

    def rows(self, n, name=None):
        return [_Row(name) for _ in range(n)]

    def link(self, r, pool, key, cnt):
        """cnt neighbours of row r, round-robin from `pool` (distinct while cnt <= len(pool))"""
        assert cnt <= len(pool)
        c = self.cursor.get(key, 0)
        for k in range(cnt):
            self.join(r, pool[(c + k) % len(pool)])
        self.cursor[key] = (c + cnt) % len(pool)

    def join(self, a, b):
        self.edges.append((a, b))
        a.deg += 1
        b.deg += 1

    def random_pairs(self, pool, n, seed, limit=None):
        """about n random pairs inside a pool: no self-loops, no repeats, in the order drawn (as boundary_graph.build); limit:
        exactly that many, the first drawn"""
        P = len(pool)
        ab = np.random.default_rng(seed).integers(0, P, size=(n, 2))
        ab = np.sort(ab[ab[:, 0] != ab[:, 1]], 1)
        _, first = np.unique(ab[:, 0] * P + ab[:, 1], return_index=True)
        ab = ab[np.sort(first)]
        assert limit is None or len(ab) >= limit
        for a, b in ab[:limit]:
            self.join(pool[int(a)], pool[int(b)])

    def finish(self, sections, fills):
        """sections: row lists; fills[s] = (position, "isolated" | "pairs" | None). Pads every section so that its cumulated
        weight ends within [T, T + 5] of T = (s + 1) W, the last one exactly on world * W: with the total exactly world * W,
        partition_rows cuts behind the last row of every section. Returns (pairs, N, row0 of every section)."""
        weight = lambda rows: sum(r.deg + 2 for r in rows)
        fixed = [weight(rows) for rows, (_, kind) in zip(sections, fills) if kind is None]
        if fixed:  # sections that cannot be padded set the weight, and hit it exactly
            W = fixed[0]
        else:
            W = max(weight(s) for s in sections) + 6
            W += W % 2
        c = 0
        for s, (rows, (pos, kind)) in enumerate(zip(sections, fills)):
            T, last = (s + 1) * W, s == len(sections) - 1
            need = T - c - weight(rows)
            assert need >= 0
            if kind == "isolated":
                extra = self.rows((need + 1) // 2, "fill")
            elif kind == "pairs":  # rows joined two by two: weight 6 a pair, own edges only
                extra = self.rows(2 * ((need + 5) // 6), "fill")
                for a, b in zip(extra[0::2], extra[1::2]):
                    self.join(a, b)
            else:
                extra = []
            rows[pos:pos] = extra
            c += weight(rows)
            assert T <= c <= T + 5 and (not last or c == T), (s, c, T)
            assert c - (rows[-1].deg + 2) < T  # the cut falls behind the last row, not before it
        row0, at = [], 0
        for rows in sections:
            row0.append(at)
            for r in rows:
                r.id = at
                at += 1
        pairs = np.array([(a.id, b.id) for a, b in self.edges], dtype=np.uint32).reshape(-1, 2)
        assert len(np.unique(np.sort(pairs.astype(np.int64), 1) @ [at, 1])) == len(pairs) and (pairs[:, 0] != pairs[:, 1]).all()
        return pairs, at, row0


# the blocks build(drop=...) can leave out, per layout
BLOCKS = {2: ("mid_hub", "next_hub"),
          3: ("head_sep", "tail_sep", "full_slots", "almost_full_slots", "no_slots", "all_peers", "pool_gap"),
          4: ("head_sep", "tail_sep", "full_slots", "almost_full_slots", "no_slots", "all_peers", "pool_gap", "empty_rank"),
          5: ("lone_hub",)}


def _edge(cap, rcap, world, drop):
    """worlds 3 and 4. The structured rank: a separator hub of cap + 1 edges (all in pool A) first and last, and
      full_slots         rcap rows of one edge into pool A and one into pool B: cap edges, all cut, 2 rcap send slots;
      almost_full_slots  the same, but the first row has both edges in pool A: 2 rcap - 1 send slots;
      no_slots           separator, rcap rows without an edge, one row of cap edges;
      all_peers          separator, a hub of BIG_HUB edges in pool A and one in pool B: a hub row every other rank reads.
    Droppable as well: head_sep / tail_sep (the first / last separator), pool_gap (no pair between the pools: without it one
    row of pool A is joined to one of pool B), empty_rank (world 4: without it two rows of the fourth rank are joined)."""
    a = _Asm()
    A, B = a.rows(POOL, "pool_a"), a.rows(POOL, "pool_b")
    S = []

    def row(name, na, nb):
        r = _Row(name)
        S.append(r)
        a.link(r, A, "A", na)
        a.link(r, B, "B", nb)

    if "head_sep" not in drop:
        row("sep", cap + 1, 0)
    if "full_slots" not in drop:
        for _ in range(rcap):
            row("full", 1, 1)
    if "almost_full_slots" not in drop:
        row("almost", 2, 0)
        for _ in range(rcap - 1):
            row("almost", 1, 1)
    if "no_slots" not in drop:
        row("sep", cap + 1, 0)
        for _ in range(rcap):
            row("zero", 0, 0)
        row("cap_row", cap, 0)
    if "all_peers" not in drop:
        row("sep", cap + 1, 0)
        row("big_hub", BIG_HUB - 1, 1)
    fill_at = len(S)
    if "tail_sep" not in drop:
        row("sep", cap + 1, 0)
    a.random_pairs(A, 2 * POOL, 78)
    a.random_pairs(B, 2 * POOL, 79)
    if "pool_gap" in drop:
        a.join(A[0], B[0])
    sections, fills = [A, S, B], [(0, "isolated"), (fill_at, "pairs"), (POOL, "isolated")]
    if world == 4:
        Z = []
        if "empty_rank" in drop:
            Z = a.rows(2, "fill")
            a.join(Z[0], Z[1])
        sections.append(Z)
        fills.append((0, "isolated"))
    return a, sections, fills


def _mid(cap, rcap, drop):
    """world 2. M: 256 own neighbours (128 leaves on either side of it) and 512 in rank 1, so its fragment boundary at 256
    edges lies between own and halo neighbours; M2 behind it: 513 edges, all in rank 1."""
    a = _Asm()
    lo, hi, L = a.rows(128, "leaf"), a.rows(128, "leaf"), a.rows(513, "read")
    mid = []
    if "mid_hub" not in drop:
        M = _Row("mid_hub")
        for r in lo + hi:
            a.join(M, r)
        a.link(M, L, "L", 512)
        mid.append(M)
    else:  # the leaves keep an edge each
        for x, y in zip(lo, hi):
            a.join(x, y)
    if "next_hub" not in drop:
        M2 = _Row("next_hub")
        a.cursor["L"] = 0
        a.link(M2, L, "L", 513)
        mid.append(M2)
    return a, [lo + mid + hi, L], [(len(lo + mid + hi), "isolated"), (len(L), "isolated")]


def _star(cap, rcap, drop):
    """world 5. Four groups of 400 leaves of one hub row of 1600 edges; 201 pairs inside every group bring a group to the
    hub's weight of 1602. Without lone_hub the leaves keep their pairs and the middle rank is isolated rows."""
    a = _Asm()
    H = _Row("lone_hub")
    groups = [a.rows(400, "leaf") for _ in range(4)]
    for k, g in enumerate(groups):
        if "lone_hub" not in drop:
            for r in g:
                a.join(H, r)
        a.random_pairs(g, 230, 80 + k, limit=201)
    if "lone_hub" in drop:
        return a, [groups[0], groups[1], [], groups[2], groups[3]], [(0, None), (0, None), (0, "isolated"), (0, None), (0, None)]
    return a, [groups[0], groups[1], [H], groups[2], groups[3]], [(0, None)] * 5


def build(cap, rcap, world, drop=()):
    """(pairs, N, names): names[i] = what row i is in the recipe. drop: block names left out (the CPU test shows that every
    block is needed)"""
    drop = (drop,) if isinstance(drop, str) else tuple(drop)
    if world not in BLOCKS or not set(drop) <= set(BLOCKS[world]):
        raise ValueError("world %r has no block %r" % (world, drop))
    if world == 2:
        a, sections, fills = _mid(cap, rcap, drop)
    elif world in (3, 4):
        a, sections, fills = _edge(cap, rcap, world, drop)
    elif world == 5:
        a, sections, fills = _star(cap, rcap, drop)
    pairs, N, row0 = a.finish(sections, fills)
    names = np.array([r.name for s in sections for r in s], dtype=object)
    return pairs, N, names, row0


def csr(pairs, N):
    """(row_ptr, nbr) with ascending neighbours in every row, as the engine's and the oracle's graph builders give it"""
    p = np.asarray(pairs, dtype=np.int64)
    src, dst = np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]])
    order = np.lexsort((dst, src))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int64)
    return row_ptr, dst[order]


# ---------------------------------------------------------------------------------------------------------------------
# what the plan model and the chunked segment model find on a case
# ---------------------------------------------------------------------------------------------------------------------
def rank_models(row_ptr, nbr, world, n_chunks, cap, rcap):
    """per rank: the plan model's shard and the chunked segment plan of its rows"""
    bounds = pm.partition_rows(row_ptr, world)
    out = []
    for r in range(world):
        sp = pm.ShardPlan(row_ptr, nbr, bounds, r, n_chunks)
        blk, hubs, cblk, chub = chunked_segment_model(sp.deg, cap, rcap, sp.chunk_row)
        flat, _ = segment_model(sp.deg, cap, rcap)
        out.append(dict(plan=sp, blk=blk, hubs=hubs, chunk_blk=cblk, chunk_hub=chub, n_blocks=len(blk) - 1, n_blocks_unchunked=len(flat) - 1,
                        n_hub_rows=len(hubs), hub_edges=int(sp.deg[hubs].sum()) if hubs else 0))
    return bounds, out


CONDITIONS = (
    "segment with 2 rcap send slots", "segment with 2 rcap - 1 send slots", "segment (rcap, 0) without a send slot in a rank > 0",
    "segment (1, cap) in a rank > 0", "plain row read by every other rank", "hub row read by every other rank",
    "hub first row of a rank > 0", "hub last row of a rank", "hub first row of a chunk > 0", "hub last row of an inner chunk",
    "hub with halo neighbours only", "hub fragment boundary between own and halo neighbours", "rank of one hub row, three empty chunks",
    "chunk boundary closes an open segment", "chunk with more than 8 segments, no multiple of 8", "chunk with 1 to 7 segments",
    "empty chunk between two others", "rank without an edge", "two ranks with edges exchange nothing",
)


def conditions(row_ptr, nbr, world, n_chunks, cap, rcap):
    """{name: [(rank, chunk or -1), ...]}: where each named case shows, by the models alone"""
    bounds, ranks = rank_models(row_ptr, nbr, world, n_chunks, cap, rcap)
    found = {k: [] for k in CONDITIONS}
    e2 = int(row_ptr[-1])
    for r, m in enumerate(ranks):
        sp, blk, hubset = m["plan"], m["blk"], set(m["hubs"])
        rp, deg, n = sp.row_ptr.astype(np.int64), sp.deg, sp.n_own
        slots = np.diff(sp.snd_ptr.astype(np.int64))
        halo = sp.nbr_local.astype(np.int64) >= n
        owner = np.full(len(halo), r)
        if sp.n_halo:
            owner[halo] = np.searchsorted(bounds, sp.halo_global[sp.nbr_local[halo].astype(np.int64) - n], side="right") - 1
        chunk_of = lambda row: int(np.searchsorted(sp.chunk_row.astype(np.int64), row, side="right")) - 1
        cr = sp.chunk_row.astype(np.int64)
        for a, b in zip(blk[:-1], blk[1:]):
            where = (r, chunk_of(a))
            if a in hubset:
                h = halo[rp[a]:rp[b]]
                if slots[a] == world - 1 and world >= 3:
                    found["hub row read by every other rank"].append(where)
                if a == 0 and r > 0:
                    found["hub first row of a rank > 0"].append(where)
                if a == n - 1:
                    found["hub last row of a rank"].append(where)
                if a > 0 and a in cr[1:-1] and a == cr[chunk_of(a)]:
                    found["hub first row of a chunk > 0"].append(where)
                if b < n and b in cr[1:-1]:
                    found["hub last row of an inner chunk"].append(where)
                if h.all():
                    found["hub with halo neighbours only"].append(where)
                if any(h[k - 1] != h[k] for k in range(FRAG, len(h), FRAG)):
                    found["hub fragment boundary between own and halo neighbours"].append(where)
                if n == 1 and n_chunks == 4 and list(cr) == [0, 1, 1, 1, 1]:
                    found["rank of one hub row, three empty chunks"].append(where)
                continue
            rows, edges, ns = b - a, int(rp[b] - rp[a]), int(slots[a:b].sum())
            if rows == rcap and edges == cap and halo[rp[a]:rp[b]].all():
                two = all(deg[i] == 2 and owner[rp[i]] != owner[rp[i] + 1] for i in range(a, b))
                if ns == 2 * rcap and two:
                    found["segment with 2 rcap send slots"].append(where)
                if ns == 2 * rcap - 1:
                    found["segment with 2 rcap - 1 send slots"].append(where)
            if r > 0 and rows == rcap and edges == 0 and ns == 0 and int(slots.sum()) > 0:
                found["segment (rcap, 0) without a send slot in a rank > 0"].append(where)
            if r > 0 and rows == 1 and edges == cap:
                found["segment (1, cap) in a rank > 0"].append(where)
            if world >= 3:
                for i in range(a, b):
                    if slots[i] == world - 1:
                        found["plain row read by every other rank"].append((r, chunk_of(i)))
                        break
        if m["n_blocks"] > m["n_blocks_unchunked"]:
            found["chunk boundary closes an open segment"].append((r, -1))
        counts = np.diff(m["chunk_blk"])
        for c, k in enumerate(counts):
            if k > 8 and k % 8:
                found["chunk with more than 8 segments, no multiple of 8"].append((r, c))
            if 0 < k < 8:
                found["chunk with 1 to 7 segments"].append((r, c))
            if k == 0 and counts[:c].any() and counts[c + 1:].any():
                found["empty chunk between two others"].append((r, c))
        if sp.n_edges == 0 and sp.n_halo == 0 and sp.send_counts.sum() == 0 and e2 > 0:
            found["rank without an edge"].append((r, -1))
        for q in range(r + 1, world):
            if sp.n_edges and ranks[q]["plan"].n_edges and sp.send_counts[q] == 0 and sp.recv_counts[q] == 0 \
                    and ranks[q]["plan"].send_counts[r] == 0 and ranks[q]["plan"].recv_counts[r] == 0:
                found["two ranks with edges exchange nothing"].append((r, q))
    return found


# ---------------------------------------------------------------------------------------------------------------------
# the per-rank fold: a ring lattice with chords over two ranks
# ---------------------------------------------------------------------------------------------------------------------
FOLD_ROWS = 64  # rows of the per-rank fold (SBMBP_FOLD_ROWS): the fold's stride grows at 65 and at 129 segments
# Rows of the ring on which rank 0 has exactly 64 / 65 / 129 segments, the smallest such (tests/test_shard_boundary_cpu.py
# asserts both). A ring of degree 2 fills segments of rcap rows and cap edges; at (512, 256) 129 of them would take 33 000
# rows a rank, so the lattice joins every row to its cap / 128 nearest rows on either side: 64 rows fill a segment in every class.
RING_N = {}


def ring_pairs(N, half):
    """row i joined to i +- 1 .. i +- half (a ring lattice), and every fourth row to the row N // 2 + 1 further on (a chord
    between the two ranks; N // 2 + 1 is odd where N // 2 is even, so the graph has odd cycles)"""
    i = np.arange(N, dtype=np.int64)
    e = [np.stack([i, (i + k) % N], 1) for k in range(1, half + 1)]
    c = i[::4]
    e.append(np.stack([c, (c + N // 2 + 1) % N], 1))
    p = np.sort(np.concatenate(e), 1)
    _, first = np.unique(p @ [N, 1], return_index=True)
    return p[np.sort(first)].astype(np.uint32)


def ring_segments(N, cap, rcap, world=2):
    """segments of every rank of ring_pairs(N, cap // 128), by the models (one chunk)"""
    pairs = ring_pairs(N, cap // 128)
    row_ptr, nbr = csr(pairs, N)
    bounds = pm.partition_rows(row_ptr, world)
    deg = np.diff(row_ptr)
    return [len(segment_model(deg[bounds[r]:bounds[r + 1]], cap, rcap)[0]) - 1 for r in range(world)]


def ring_size(cap, rcap, segments):
    """the smallest N (a multiple of 4) at which rank 0 of two has exactly `segments` segments"""
    key = (cap, rcap, segments)
    if key not in RING_N:
        N = 4 * (segments * 12)  # well below: a segment holds at most rcap >= 64 rows
        while ring_segments(N, cap, rcap)[0] < segments:
            N += 4 * 64
        N -= 4 * 64
        while ring_segments(N, cap, rcap)[0] < segments:
            N += 4
        RING_N[key] = N
    return RING_N[key]


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_shard_boundary.py; tests/test_shard_boundary_cpu.py checks each of them on the CPU
# ---------------------------------------------------------------------------------------------------------------------
THRESHOLD = [(Q, dc) for Q in (2, 4, 5, 8, 9, 16) for dc in (0, 1)] + [(Q, 2) for Q in (2, 5, 9)]
LAYOUTS = [(2, 1), (2, 4), (3, 1), (3, 4), (4, 1), (4, 4), (5, 4)]  # (world, n_chunks): every one shows a condition of its own
CLAMPED_Q = (3, 8, 13)
LABELS = list(BATCH)  # every compiled label count on the (128, 64) recipe, dc rotating as in boundary_graph.BATCH
FOLD = [(Q, segs, clamp) for Q in (3, 7, 13) for segs in (64, 65, 129) for clamp in (False, True) if not clamp or segs == 65]
KNOB_Q = (5, 12)
DAMPS = (0.7, 0.7, 1.0, 1.0, 1.0)  # boundary_graph.SINGLE_DAMPS
# Cases whose reference run does not converge within 600 sweeps at 1e-10 (the GPU test then only requires that both sides
# report -1): degree-corrected runs on the star-like layouts (worlds 2 and 5: one row holds most of the edges, and the
# synchronous sweep swings with period 2 at differences of order 1), some on the four-rank layout, and two star runs without
# degree correction. tests/test_shard_boundary_cpu.py fails if a case belongs here and is not listed, or is listed and converges.
NOT_CONVERGING = {
    ("threshold", 2, 1, 2), ("threshold", 2, 2, 2), ("threshold", 4, 1, 2), ("threshold", 5, 1, 2), ("threshold", 5, 2, 2),
    ("threshold", 8, 1, 2), ("threshold", 9, 1, 2), ("threshold", 9, 2, 2), ("threshold", 16, 1, 2), ("threshold", 4, 1, 4),
    ("threshold", 5, 2, 4), ("threshold", 8, 1, 4), ("threshold", 9, 1, 4), ("threshold", 9, 2, 4), ("threshold", 2, 1, 5),
    ("threshold", 2, 2, 5), ("threshold", 4, 0, 5), ("threshold", 4, 1, 5), ("threshold", 5, 0, 5), ("threshold", 5, 1, 5),
    ("threshold", 5, 2, 5), ("threshold", 8, 1, 5), ("threshold", 9, 1, 5), ("threshold", 9, 2, 5), ("threshold", 16, 1, 5),
}

_GRAPHS = {}


def graph(cap, rcap, world):
    """build(cap, rcap, world) once per process; the arrays are read-only"""
    key = (cap, rcap, world)
    if key not in _GRAPHS:
        pairs, N, names, row0 = build(cap, rcap, world)
        row_ptr, nbr = csr(pairs, N)
        for x in (pairs, row_ptr, nbr):
            x.setflags(write=False)
        _GRAPHS[key] = dict(pairs=pairs, N=N, names=names, row0=row0, row_ptr=row_ptr, nbr=nbr, deg=np.diff(row_ptr))
    return _GRAPHS[key]


def ring_graph(cap, rcap, segments):
    key = (cap, rcap, "ring", segments)
    if key not in _GRAPHS:
        N = ring_size(cap, rcap, segments)
        pairs = ring_pairs(N, cap // 128)
        row_ptr, nbr = csr(pairs, N)
        for x in (pairs, row_ptr, nbr):
            x.setflags(write=False)
        _GRAPHS[key] = dict(pairs=pairs, N=N, row_ptr=row_ptr, nbr=nbr, deg=np.diff(row_ptr))
    return _GRAPHS[key]


def clamp_rows(gr):
    """ten rows of the edge layout the clamped variants pin: first and last row of the two slot segments and of the rows
    without an edge, the row of cap edges, the big hub, the first separator, a pool row"""
    nm = gr["names"]
    at = lambda name: np.flatnonzero(nm == name)
    rows = [at("full")[0], at("full")[-1], at("almost")[0], at("almost")[-1], at("zero")[0], at("zero")[-1], at("cap_row")[0],
            at("big_hub")[0], at("sep")[0], at("pool_b")[0]]
    return sorted(int(x) for x in rows)


def instance(Q, dc, world, clamp=False, cls=None, ring=None):
    """a case on the recipe of Q's capacity class (cls: of another class; ring: the ring of that many segments)"""
    cap, rcap = caps_for(Q)
    gr = ring_graph(cap, rcap, ring) if ring else graph(*(cls or (cap, rcap)), world)
    cab, na, tc = params(Q, gr["N"], dc, gr["pairs"])
    conf = None
    if clamp:
        conf = np.full(gr["N"], -1, dtype=np.int32)
        rows = np.arange(0, gr["N"], 9) if ring else clamp_rows(gr)
        conf[rows] = tc[rows]
    return dict(gr, Q=Q, dc=dc, cap=cap, rcap=rcap, world=world, cab=cab, na=na, tc=tc, flag=1 if clamp else 0, conf=conf, seed=Q)


CALLS = ((2, DAMPS[0]), (3, DAMPS[2]))  # the five sweeps as two calls: equal dampings queued together
assert tuple(d for n, d in CALLS for _ in range(n)) == DAMPS


def run_case(S, t, n_chunks):
    """one sharded run of a case on the engine S (the package, passed in: this module imports nothing of the product), the
    sweeps queued as CALLS: (differences, marginals after either call, messages after the last, halo components)"""
    from sbm_bp_amd.distributed import LocalShards
    sb = LocalShards(S.Graph.from_edges(t["pairs"], t["N"]), t["Q"], t["dc"], t["world"], n_chunks=n_chunks)
    try:
        sb.init_messages(t["flag"], t["conf"], t["tc"], t["seed"], True)
        sb.expand_bp_params(t["cab"], t["na"], 1.0)
        d, psi = [], []
        for n, damp in CALLS:
            d.append(sb.sweep(n, damp))
            p, msg = sb.global_state()
            psi.append(p)
        return np.array(d), np.array(psi), msg, sb.ranks[0].info.halo_components
    finally:
        sb.close()
