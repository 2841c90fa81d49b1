"""Agreement of the replicas of a batch (include/sbmbp.h sbmbp_batch_agreement; csrc/kernels_batch.h k_agree / k_agree_fold):
the pairwise confusion matrices of all three kinds against tests/agreement_model.py, the exact overlap and alignment, the
groups, and the command line. The kernel reads marginals only, so most cases set the marginal tables directly. Every graph
has at most 20 011 vertices."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import agreement_model as M
import batch_scale_graph as sc
from conftest import ROOT, args_of, golden, gpath
from test_gpu_batch import batch_from

pytestmark = pytest.mark.gpu

TRIP = 32  # vertices a workgroup stages per trip: AG_V of csrc/kernels_batch.h
KINDS = ("soft", "hard_soft", "hard")


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def test_the_trip_is_the_kernels():
    src = open(os.path.join(ROOT, "sbm-bp_amd", "csrc", "kernels_batch.h")).read()
    assert "constexpr int AG_V = %d," % TRIP in src


def ring_batch(S, N, Q, R):
    """a batch of R replicas on a ring of N vertices (a single edge for N = 2, no edge for N = 1), every replica with a state"""
    if N >= 3:
        pairs = np.stack([np.arange(N), (np.arange(N) + 1) % N], 1).astype(np.uint32)
    else:
        pairs = np.array([[0, 1]] if N == 2 else [], dtype=np.uint32).reshape(-1, 2)
    g = S.Graph.from_edges(pairs, N)
    b = S.ReplicaBatch(g, Q, 0, R)
    b.init_messages(0, None, (np.arange(N) % Q).astype(np.uint32), list(range(R)))
    return g, b


def random_tables(rng, n, N, Q):
    out = []
    for _ in range(n):
        p = rng.random((N, Q)) ** 3  # peaked rows: the labels are spread over all of 0 .. Q-1
        out.append(p / p.sum(1, keepdims=True))
    return out


def set_tables(b, psis, replicas=None):
    for x, p in enumerate(psis):
        b.set_state(x if replicas is None else replicas[x], p, None)


def check_against_model(b, psis, replicas=None, kinds=KINDS):
    """all kinds against the model on the tables psis (those of the listed replicas). SOFT and HARD_SOFT entrywise to
    4 N 2^-53 C + 1e-300: both sides add N non-negative terms in some order, each within N 2^-53 C of the exact sum. HARD with ==:
    integer sums below 2^53. The overlap is the brute-force maximum for Q <= 8 (its Q terms are added in one order on both sides
    only up to rounding: Q 2^-53 relative), and always the trace along the returned permutation. Above 64 pairs the brute force
    takes the first 8 x 8 pairs and 64 drawn ones; the trace and the permutation are checked on every pair."""
    N, Q = psis[0].shape
    n = len(psis)
    brute = None
    if n * n > 64:
        drawn = np.random.default_rng(n * 1000 + Q).integers(0, n, size=(64, 2))
        brute = {(x, y) for x in range(8) for y in range(8)} | {(int(x), int(y)) for x, y in drawn}
    out = {}
    for kind in kinds:
        ov, C, perm = b.agreement(kind, replicas)
        Cm = M.confusion(psis, kind)
        if kind == "hard":
            assert np.array_equal(C, Cm), kind
            assert np.array_equal(C, np.swapaxes(np.swapaxes(C, 0, 1), 2, 3))  # C_yx = C_xy^T
            assert (np.diagonal(ov) == 1.0).all()
        else:
            err = np.abs(C - Cm)
            print(kind, "max error / bound", np.nanmax(err / (4 * N * 2.0 ** -53 * np.abs(Cm) + 1e-300)))
            assert (err <= 4 * N * 2.0 ** -53 * np.abs(Cm) + 1e-300).all(), kind
        for x in range(n):
            for y in range(n):
                p = perm[x, y]
                assert sorted(p) == list(range(Q))
                tr = sum(C[x, y, a, p[a]] for a in range(Q)) / N
                assert ov[x, y] == tr
                if Q <= 8 and (brute is None or (x, y) in brute):
                    best, _ = M.overlap_brute(C[x, y], N)
                    assert abs(ov[x, y] - best) <= 2 * Q * 2.0 ** -53 * max(best, 1e-300), (kind, x, y, ov[x, y], best)
        out[kind] = (ov, C, perm)
    return out


# (n, Q): one column pair in a 16-wide tile; n Q = 15, 16, 18; two tiles; n Q = 65; the limit 256 with the tile rows split
@pytest.mark.parametrize("n,Q", [(1, 2), (3, 5), (4, 4), (3, 6), (8, 4), (5, 13), (16, 16)])
def test_all_kinds_against_the_model(S, n, Q):
    N = 777  # 24 trips and a last one of 9 vertices
    g, b = ring_batch(S, N, Q, n)
    psis = random_tables(np.random.default_rng(100 * n + Q), n, N, Q)
    set_tables(b, psis)
    for x in range(n):  # what the call must read is what get_state returns
        assert np.array_equal(b.get_state(x, msg=False)[0], psis[x])
    check_against_model(b, psis)
    b.close()


@pytest.mark.parametrize("n,Q", sc.AGREE)
def test_every_tile_shape_against_the_model(S, n, Q):
    """with the cases above, every tile count CT = ceil(n Q / 16) from 1 to 16 (tests/batch_scale_graph.py agree_plan;
    tests/test_batch_scale_cpu.py asserts the coverage): the three k_agree<KIND, 4> instantiations (CT 3 and 4), every ragged
    last workgroup row - (7, 2), (6, 4), (5, 5, 1), (5, 5, 2), (4, 4, 4, 1 .. 3) -, both parities of the image's row stride,
    exact multiples of 16 columns and one column under and over, and more than 16 replicas: label rows of (n + 7) & ~7 bytes
    and a slot table filled by more than one wave, up to AG_MAXN = 128 replicas"""
    N = 777
    p = sc.agree_plan(n, Q)
    print("agreement n %d Q %d: CT %d, TPW %d, workgroup rows %s, S %d, LN %d, %d padding columns"
          % (n, Q, p["CT"], p["TPW"], p["split"], p["S"], p["LN"], p["pad"]))
    g, b = ring_batch(S, N, Q, n)
    psis = random_tables(np.random.default_rng(100 * n + Q), n, N, Q)
    set_tables(b, psis)
    check_against_model(b, psis)
    b.close()


def test_the_partial_table_budget_decides_the_grid(S):
    """N = 20 011 with 256 columns: the budget of the partial tables (128 tables of 512 KB) decides the number of workgroups
    along the vertices, not the trips (157); every workgroup walks four or five trips, and the fold adds 128 tables"""
    N, n, Q = sc.AGREE_BUDGET
    p = sc.agree_plan(n, Q)
    terms = sc.agree_gx_terms(N, p["CP"], p["gy"])
    assert terms == (157, 256, 128) and sc.agree_gx(N, p["CP"], p["gy"]) == 128
    g, b = ring_batch(S, N, Q, n)
    psis = random_tables(np.random.default_rng(20011), n, N, Q)
    set_tables(b, psis)
    first = check_against_model(b, psis)
    for kind in KINDS:
        again = b.agreement(kind)
        for u, v in zip(first[kind], again):
            assert u.tobytes() == v.tobytes(), kind
    b.close()


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, TRIP - 1, TRIP, TRIP + 1])
def test_rows_on_the_trip_and_step_edges(S, N):
    n, Q = 3, 5  # 15 columns: one padding column next to the data
    g, b = ring_batch(S, N, Q, n)
    psis = random_tables(np.random.default_rng(N), n, N, Q)
    set_tables(b, psis)
    check_against_model(b, psis)
    b.close()


def test_many_workgroups_many_trips_and_the_same_bits_twice(S):
    N, n, Q = 20011, 5, 4  # 626 trips: more than a hundred workgroups of several trips each, as many partial tables in the fold
    g, b = ring_batch(S, N, Q, n)
    psis = random_tables(np.random.default_rng(7), n, N, Q)
    set_tables(b, psis)
    first = check_against_model(b, psis)
    for kind in KINDS:
        again = b.agreement(kind)
        for u, v in zip(first[kind], again):
            assert u.tobytes() == v.tobytes(), kind
    b.close()


@pytest.mark.parametrize("Q", [4, 12])
def test_a_relabelled_copy_has_overlap_one(S, Q):
    """replica 1 = replica 0 with label a moved to pi(a). At Q = 12 the identity rule of the overlap with the true configuration
    would report the trace of a permuted matrix."""
    N = 500
    rng = np.random.default_rng(Q)
    g, b = ring_batch(S, N, Q, 2)
    p0 = random_tables(rng, 1, N, Q)[0]
    p0[:, Q - 1] = 0.0  # the last label owns no vertex: it may map anywhere
    p0 /= p0.sum(1, keepdims=True)
    pi = rng.permutation(Q)
    while (pi == np.arange(Q)).all():
        pi = rng.permutation(Q)
    p1 = np.zeros_like(p0)
    p1[:, pi] = p0
    set_tables(b, [p0, p1])
    ov, C, perm = b.agreement("hard")
    assert ov[0, 1] == 1.0 and ov[1, 0] == 1.0 and ov[0, 0] == 1.0
    owned = np.flatnonzero(np.bincount(M.labels(p0), minlength=Q))
    assert len(owned) == Q - 1
    assert (perm[0, 1][owned] == pi[owned]).all(), (perm[0, 1], pi)
    inv = np.argsort(pi)
    assert (perm[1, 0][pi[owned]] == inv[pi[owned]]).all()
    assert np.trace(C[0, 1]) < N  # the identity would not have found it
    check_against_model(b, [p0, p1])
    b.close()


def test_ties_go_to_the_lowest_label_and_nan_rows_to_label_0(S):
    N, Q = 70, 4
    g, b = ring_batch(S, N, Q, 3)
    tie = np.tile([0.1, 0.4, 0.1, 0.4], (N, 1))         # two equal maxima: label 1
    tie[::2] = [0.25, 0.25, 0.25, 0.25]                 # four: label 0
    nan = np.full((N, Q), np.nan)
    plain = random_tables(np.random.default_rng(3), 1, N, Q)[0]
    plain[5] = [np.nan, 0.2, 0.7, 0.1]                  # a NaN never wins: label 2
    plain[6] = [0.3, np.nan, 0.3, np.nan]               # label 0
    set_tables(b, [tie, nan, plain])
    ov, C, perm = b.agreement("hard")
    assert C[0, 0, 0, 0] == N // 2 and C[0, 0, 1, 1] == N // 2 and C[0, 0].sum() == N
    assert C[1, 1, 0, 0] == N and C[1, 1].sum() == N
    lab = M.labels(np.nan_to_num(plain, nan=-np.inf))
    assert lab[5] == 2 and lab[6] == 0
    assert np.array_equal(C[2, 2], np.diag(np.bincount(lab, minlength=Q)).astype(float))
    assert np.array_equal(C[0, 2], M.confusion([tie, np.nan_to_num(plain, nan=-np.inf)], "hard")[0, 1])
    # HARD_SOFT with the NaN rows on the hard side only
    C1 = b.agreement("hard_soft", [1, 0])[1]
    Cm = M.confusion([np.nan_to_num(nan, nan=0.0), tie], "hard_soft")  # all rows label 0
    assert np.abs(C1[0, 1] - Cm[0, 1]).max() <= 4 * N * 2.0 ** -53 * Cm[0, 1].max()
    b.close()


@functools.lru_cache(maxsize=None)
def _q4():
    return args_of(golden("q4_tight_seed0"))


PARITY_SEEDS = [0, 1, 2, 3, 4, 5]


def _converged_states_equal_the_model(b, R):
    psis = [b.get_state(r, msg=False)[0] for r in range(R)]
    check_against_model(b, psis)
    return psis


def test_replicas_on_different_parities(S):
    """replicas of one batch stop on different sweeps, so their current tables lie in different halves of the double buffer:
    the call must read the table get_state returns for each. The same under a per-vertex prior of one replica."""
    a = _q4()
    g, b, st = batch_from(S, a, PARITY_SEEDS)
    niter, last = b.converge(a["crit"], a["tmax"], 1.0)
    print("niter", list(niter))
    assert (niter >= 0).all()
    assert len({(int(k) + 1) & 1 for k in niter}) == 2, niter  # sweeps executed: odd for some replicas, even for others
    _converged_states_equal_the_model(b, len(PARITY_SEEDS))
    # one replica under a prior table of its own, the others advanced beside it
    prior = np.ones((a["N"], a["Q"]))
    prior[::3, 0] = 4.0
    b.set_vertex_prior(prior, 1)
    b.sweep(3, 1.0)
    _converged_states_equal_the_model(b, len(PARITY_SEEDS))
    b.close()


def test_after_a_coloured_converge(S):
    a = _q4()
    g, b, st = batch_from(S, a, PARITY_SEEDS[:4])
    b.sweep(1, 1.0)  # odd parity for all, then in place
    b.set_sweep_order("coloured")
    b.converge(a["crit"], a["tmax"], 1.0)
    _converged_states_equal_the_model(b, 4)
    b.close()


def test_hard_soft_is_the_confusion_of_the_single_engine(S):
    """row (x, .): a single engine whose true configuration is l^x and whose state is replica y's reports C_xy as confusion()"""
    a = _q4()
    seeds = [0, 1, 2]
    g, b, st = batch_from(S, a, seeds)
    b.sweep(7, 1.0)
    states = [b.get_state(r) for r in range(3)]
    ov, C, perm = b.agreement("hard_soft")
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    for x in range(3):
        lx = M.labels(states[x][0]).astype(np.uint32)
        for y in range(3):
            bp = S.bp_conditional()
            bp.init_messages(bm, 0, None, lx, 0)
            bp.set_state(*states[y])
            Cs = bp.confusion()
            assert (np.abs(Cs - C[x, y]) <= 4 * a["N"] * 2.0 ** -53 * np.abs(Cs) + 1e-300).all(), (x, y)
    b.close()


def test_subsets_and_refusals(S):
    N, Q, R = 300, 4, 4
    g, b = ring_batch(S, N, Q, R)
    psis = random_tables(np.random.default_rng(11), R, N, Q)
    set_tables(b, psis)
    for kind in KINDS:
        ov, C, perm = b.agreement(kind)
        ov2, C2, perm2 = b.agreement(kind, [2, 0])
        idx = [2, 0]
        for i, x in enumerate(idx):
            for j, y in enumerate(idx):
                assert np.array_equal(C2[i, j], C[x, y]) and ov2[i, j] == ov[x, y] and np.array_equal(perm2[i, j], perm[x, y])
    check_against_model(b, [psis[3]], [3])
    for bad, what in (([0, 0], "twice"), ([1, 4], "outside"), ([], "n >= 1")):
        with pytest.raises(S.SbmbpError) as ei:
            b.agreement("hard", bad)
        assert ei.value.code == -1 and what in str(ei.value), bad
    with pytest.raises(S.SbmbpError) as ei:
        b.agreement(3)
    assert ei.value.code == -1
    b.close()
    # 17 replicas of 16 labels are 272 columns
    g = S.Graph.from_edges(np.array([[0, 1], [1, 2]], dtype=np.uint32), 3)
    b = S.ReplicaBatch(g, 16, 0, 17)
    with pytest.raises(S.SbmbpError) as ei:
        b.agreement("hard")
    assert ei.value.code == -6 and "subset" in str(ei.value)
    with pytest.raises(S.SbmbpError) as ei:  # a subset fits, but nobody has a state yet
        b.agreement("hard", [0, 1])
    assert ei.value.code == -4
    b.init_messages(0, None, np.zeros(3, dtype=np.uint32), list(range(17)))
    ov = b.agreement("hard", list(range(16)))[0]
    assert ov.shape == (16, 16) and (np.diagonal(ov) == 1.0).all()
    b.close()


def _stats_bytes(b):
    import ctypes as C
    s = b.stats()
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


def test_nothing_moves(S):
    """states, sweep counts, statistics and the next sweep are bit for bit the same with and without agreement calls in between"""
    a = _q4()
    seeds = [0, 1, 2]
    runs = []
    for with_call in (False, True):
        g, b, st = batch_from(S, a, seeds)
        b.sweep(3, 1.0)
        if with_call:
            before = ([b.get_state(r) for r in range(3)], _stats_bytes(b))
            for kind in KINDS:
                b.agreement(kind)
            b.agreement("hard", [1])
            after = ([b.get_state(r) for r in range(3)], _stats_bytes(b))
            assert before[1] == after[1]
            for (p0, m0), (p1, m1) in zip(before[0], after[0]):
                assert p0.tobytes() == p1.tobytes() and m0.tobytes() == m1.tobytes()
        d = b.sweep(1, 1.0)
        niter, last = b.converge(a["crit"], a["tmax"], 1.0)
        f = b.compute_free_energy()
        runs.append((d.tobytes(), niter.tobytes(), last.tobytes(), f.tobytes(), [tuple(x.tobytes() for x in b.get_state(r)) for r in range(3)],
                     _stats_bytes(b), b.stats().sweeps))
        b.close()
    assert runs[0] == runs[1]


def test_three_fixed_points_of_the_hub_graph_are_three_groups(S):
    """hub_n600 under dc 0 has three BP fixed points: the reference's runs from seeds 0, 1 and 23. Their
    HARD overlaps, computed here with the model from the goldens' marginals: 0.588333 (0, 1), 0.523333 (0, 23), 0.785 (1, 23).
    The largest is 0.215 away from 1; the threshold 0.999 leaves 0.001, a margin of 215."""
    names = ["hub_dc0_tight_seed0", "hub_dc0_tight_seed1", "hub_dc0_tight_seed23"]
    gs = [golden(n) for n in names]
    a = args_of(gs[0])
    N, Q = a["N"], a["Q"]
    psis = [np.array(x["result"]["psi"]).reshape(N, Q) for x in gs]
    Cm = M.confusion(psis, "hard")
    cross = [M.overlap_brute(Cm[x, y], N)[0] for x, y in ((0, 1), (0, 2), (1, 2))]
    threshold = 0.999
    assert max(cross) < threshold and (1.0 - max(cross)) >= 10 * (1.0 - threshold), cross
    pi = np.array([2, 0, 1])
    copy = np.zeros_like(psis[0])
    copy[:, pi] = psis[0]
    g, b, st = batch_from(S, a, [0, 1, 23, 5])
    set_tables(b, psis + [copy])
    group, n_groups, ov = b.agreement_groups(threshold)
    assert n_groups == 3 and list(group) == [0, 1, 2, 0], (group, ov)
    assert ov[0, 3] == 1.0 and list(b.agreement("hard")[2][0, 3]) == list(pi)
    mg, mn = M.groups(ov, threshold)
    assert mn == 3 and np.array_equal(mg, group)
    for (x, y), c in zip(((0, 1), (0, 2), (1, 2)), cross):
        assert ov[x, y] == c
    b.close()


def test_command_line_reports_the_agreement(S, tmp_path):
    BP = os.path.join(ROOT, "bin", "bp")
    a = args_of(golden("q10_tight_seed1"))
    base = [str(x) for x in [BP, "-l", a["path"], "-n"] + a["n"] + ["--pa"] + a["pa"] + ["--cab"] + a["cab_upper"] +
            ["-m", "infer", "-d", 1, "-e", 1e-10, "-t", 2000, "--restarts", 3]]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    mj = tmp_path / "m.json"
    pr = subprocess.run(base + ["--agreement", "0.99", "--metrics_json", str(mj)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and pr.returncode == 0, (plain.stderr[-2000:], pr.stderr[-2000:])
    assert pr.stdout == plain.stdout and plain.stdout != ""
    lines = [x for x in pr.stderr.splitlines() if x.startswith("agreement:")]
    assert len(lines) == 1 and "agreement:" not in plain.stderr
    ag = json.load(open(mj))["agreement"]
    assert ag["kind"] == "hard" and ag["threshold"] == 0.99
    ov = np.array(ag["overlap"])
    assert ov.shape == (3, 3)
    mg, mn = M.groups(ov, 0.99)
    assert ag["n_groups"] == mn and ag["group"] == list(mg)
    assert ("%d group" % mn) in lines[0]
    # the same seeds through ReplicaBatch
    g, b, st = batch_from(S, a, [1, 2, 3])
    b.set_schedule(1.0, 8)
    res, best = b.inference(1e-10, 2000, 1.0)
    ov2 = b.agreement("hard")[0]
    assert np.abs(ov - ov2).max() <= 1e-12, (ov, ov2)
    b.close()
