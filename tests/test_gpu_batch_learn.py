"""Multi-start EM on replica batches (include/sbmbp.h: sbmbp_batch_em_step, sbmbp_batch_learning; csrc/kernels_batch.h:
k_em_frame_batch and the other reduction kernels with the replica as a grid dimension), against the per-replica reductions of
the batch, single engines in message-gather form, the oracle's synchronous learning and the reference's goldens.
Every instance has N <= 1000."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, args_of, golden, gpath
from test_gpu_coloured import _hub_instance
from test_gpu_parity import oracle_from

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


# ------------------------------------------------------------------------------------------------------------------
# (1) the batched reductions against the per-replica path and the oracle, on the same states
# ------------------------------------------------------------------------------------------------------------------
def _fixture_instance(name, dc=None, beta=None):
    a = args_of(golden(name))
    import oracle as orc
    if "eps" in a:
        cab, na = orc.param_from_epsilon_c(a["N"], a["Q"], a["eps"], a["c"])
    else:
        cab, na = orc.param_from_direct(a["N"], a["Q"], a["pa"], a["cab_upper"])
    pairs = np.loadtxt(a["path"], dtype=np.int64).reshape(-1, 2)[:, :2].astype(np.uint32)
    return dict(pairs=pairs, N=a["N"], Q=a["Q"], dc=a["dc"] if dc is None else dc, beta=a["beta"] if beta is None else beta, cab=cab, na=na,
                tc=a["true_conf"], conf=None, flag=0)


def _random_instance(zeros, clamp):
    rng = np.random.default_rng(21)
    Q, N = 3, 240
    pairs = rng.integers(0, N, size=(700, 2)).astype(np.uint32)
    cab = np.array([[8.0, 0.0, 1.0], [0.0, 7.0, 1.5], [1.0, 1.5, 6.0]]) if zeros else np.array([[8.0, 0.5, 1.0], [0.5, 7.0, 1.5], [1.0, 1.5, 6.0]])
    tc = rng.integers(0, Q, size=N).astype(np.uint32)
    na = np.bincount(tc, minlength=Q).astype(np.uint32)
    conf = None
    if clamp:
        conf = np.full(N, -1, dtype=np.int32)
        fixed = rng.choice(N, 40, replace=False)
        conf[fixed] = tc[fixed]
    return dict(pairs=pairs, N=N, Q=Q, dc=0, beta=1.0, cab=cab, na=na, tc=tc, conf=conf, flag=1 if clamp else 0)


def _hub(Q, N, long_row, dc):
    pairs, cab, na, tc = _hub_instance(Q, N, long_row)
    return dict(pairs=pairs, N=N, Q=Q, dc=dc, beta=1.0, cab=cab / 36.0 if dc else cab, na=na, tc=tc, conf=None, flag=0)


INSTANCES = {
    "c1_dc0_beta08": lambda: _fixture_instance("c1_matched_beta08_seed0", 0, 0.8),
    "c1_dc1_beta08": lambda: _fixture_instance("c1_dc1_tight_seed0", 1, 0.8),
    "c1_dc2_beta08": lambda: _fixture_instance("c1_dc2_tight_seed0", 2, 0.8),
    "q4_n400": lambda: _fixture_instance("q4_tight_seed0"),
    "q10_n1000": lambda: _fixture_instance("q10_tight_seed1"),  # above EM_FRAME_QMAX labels: the numerators take k_em_edges_batch
    "zeros_in_cab": lambda: _random_instance(True, False),
    "clamped_rows": lambda: _random_instance(False, True),
    "hub_q9_dc0": lambda: _hub(9, 300, 140, 0),   # Q = 9: a segment holds 128 edges
    "hub_q9_dc1": lambda: _hub(9, 300, 140, 1),
    "hub_q5_dc0": lambda: _hub(5, 400, 300, 0),   # Q = 5: a segment holds 256 edges; the numerators of the hub row come from the frame pass
    "hub_q5_dc2": lambda: _hub(5, 400, 300, 2),
}
SERIES_K = 3  # the highest order every label count up to 16 has (engine.hip: max_series_order)
SCALES = (1.0, 1.1, 0.85)  # three different (cab, na)


def _three_params(inst):
    out = []
    for r, s in enumerate(SCALES):
        na = inst["na"].astype(np.int64).copy()
        if r:  # move r vertices from the first group to the last
            na[0] -= r
            na[-1] += r
        out.append((inst["cab"] * s, na.astype(np.uint32)))
    return out


@pytest.mark.parametrize("mode", [1, 2], ids=["exact", "series"])
@pytest.mark.parametrize("name", list(INSTANCES))
def test_em_step_equals_the_per_replica_reductions(S, orc, name, mode):
    inst = INSTANCES[name]()
    Q, N, dc = inst["Q"], inst["N"], inst["dc"]
    g = S.Graph.from_edges(inst["pairs"], N)
    og = orc.Graph.from_edges(inst["pairs"], N)
    seeds = [3, 4, 5]
    params = _three_params(inst)

    def make():
        b = S.ReplicaBatch(g, Q, dc, 3)
        b.init_messages(inst["flag"], inst["conf"], inst["tc"], seeds, conditional=True)
        for r, (cab, na) in enumerate(params):
            b.set_params(S.bp_blockmodel_state(cab, na), inst["beta"], r)
        # forced series: order 3 on both sides. At N <= 1000 the truncated series is 1e-7 away from the exact sum, so the oracle
        # evaluates the series of the same order (tests/test_gpu_series.py pins the two to each other order by order;
        # test_series_order_is_per_replica compares the automatic orders with the exact sum)
        b.set_nonedge_mode(mode, SERIES_K if mode == 2 else 0)
        b.set_schedule(field_mix=0.5)  # a relaxed field is stale after the sweeps: the field refresh runs first
        last = b.sweep(3, 1.0)
        assert (last > 1e-6).all()  # not converged
        return b

    # two batches in the same states (the sweeps are reproducible bit for bit): the per-replica reference runs on the second,
    # so its field refresh is the single engine's and not the one k_field_refresh_batch left behind
    b, b2 = make(), make()
    if name.startswith("hub"):
        assert b.stats().n_hub_rows == 1
    assert all(np.array_equal(x, y) for r in range(3) for x, y in zip(b.get_state(r), b2.get_state(r)))
    na_b, nna_b, cab_b, f_b, parts_b = b.em_step()
    f_r, parts_r = b2.compute_free_energy(parts=True)

    def close(x, y, tol):
        x, y = np.asarray(x), np.asarray(y)
        d = np.abs(x - y) / np.maximum(1.0, np.abs(y))
        print("%s mode %d: max rel diff %.3g (tol %g)" % (name, mode, d.max(), tol))
        return bool((d <= tol).all())

    for r in range(3):
        na_r, nna_r, cab_r = b2.em_expectations(r)
        assert close(na_b[r], na_r, 1e-11) and close(nna_b[r], nna_r, 1e-11) and close(cab_b[r], cab_r, 1e-11), r
    assert close(parts_b, parts_r, 1e-11) and close(f_b, f_r, 1e-11)
    # a second call on the same states gives the same bits (fixed summation order)
    again = b.em_step()
    assert all(np.array_equal(x, y) for x, y in zip((na_b, nna_b, cab_b, f_b, parts_b), again))
    # the oracle on the same states
    for r, (cab, na) in enumerate(params):
        psi, msg = b.get_state(r)
        ob = orc.OracleBP(og, Q, dc)
        ob.init_messages(inst["flag"], inst["conf"], inst["tc"], orc.Rng(seeds[r]))
        ob.set_params(cab, na, inst["beta"])
        ob.set_state(psi, msg)
        ob.compute_h()
        ona, onna, ocab = ob.em_expect()
        fo, oparts = ob.free_energy(SERIES_K if mode == 2 else 0)
        assert close(na_b[r], ona, 1e-9) and close(nna_b[r], onna, 1e-9) and close(cab_b[r], ocab, 1e-9), r
        assert close(parts_b[r], oparts, 1e-9) and close(f_b[r], fo, 1e-9), r
    b.close()
    b2.close()


def test_series_order_is_per_replica(S, orc):
    """automatic series order (SURVEY A.4 bound below 1e-12): three replicas on the c1 dataset whose cab are far enough apart
    that the orders are 4, 3 and 2. The moment kernel runs at the largest, every replica contracts the orders it asked for:
    per-replica path at 1e-11, the oracle's EXACT non-edge sum at 1e-9."""
    inst = _fixture_instance("c1_matched_tight_seed0")
    Q, N = inst["Q"], inst["N"]
    scales = (1.0, 0.01, 0.001)

    def order(cab):  # host_reduce.h: series_order
        wmax = max((N * (1.0 - (1.0 - cab / N))).max(), cab.max())
        return next((K for K in range(1, 5) if N * (wmax / N) ** (K + 1) / (2.0 * (K + 1)) < 1e-12), 4)

    assert [order(inst["cab"] * s) for s in scales] == [4, 3, 2]
    g = S.Graph.from_edges(inst["pairs"], N)
    og = orc.Graph.from_edges(inst["pairs"], N)
    seeds = [3, 4, 5]

    def make():
        b = S.ReplicaBatch(g, Q, 0, 3)
        b.init_messages(0, None, inst["tc"], seeds)
        for r, s in enumerate(scales):
            b.set_params(S.bp_blockmodel_state(inst["cab"] * s, inst["na"]), 1.0, r)
        b.set_nonedge_mode(2, 0)
        b.sweep(3, 1.0)
        return b

    b, b2 = make(), make()
    _, _, _, f_b, parts_b = b.em_step()
    f_r, parts_r = b2.compute_free_energy(parts=True)
    print("f_nonedge batch / per replica:", parts_b[:, 2], parts_r[:, 2])
    assert np.abs(parts_b - parts_r).max() <= 1e-11 and np.abs(f_b - f_r).max() <= 1e-11
    for r, s in enumerate(scales):
        psi, msg = b.get_state(r)
        ob = orc.OracleBP(og, Q, 0)
        ob.init_messages(0, None, inst["tc"], orc.Rng(seeds[r]))
        ob.set_params(inst["cab"] * s, inst["na"], 1.0)
        ob.set_state(psi, msg)
        ob.compute_h()
        fo, oparts = ob.free_energy(0)
        print("replica %d: f_nonedge %.15g oracle (exact) %.15g" % (r, parts_b[r, 2], oparts[2]))
        assert np.abs(parts_b[r] - oparts).max() <= 1e-9 * max(1.0, np.abs(oparts).max()) and abs(f_b[r] - fo) <= 1e-9 * max(1.0, abs(fo))
    b.close()
    b2.close()


def test_em_step_needs_parameters_and_state(S):
    rng = np.random.default_rng(0)
    g = S.Graph.from_edges(rng.integers(0, 200, size=(600, 2)).astype(np.uint32), 200)
    b = S.ReplicaBatch(g, 3, 0, 2)
    for call in (b.em_step, lambda: b.learning(1e-6, 10, 0.2, 1.0)):
        with pytest.raises(S.SbmbpError) as ei:
            call()
        assert ei.value.code == -4
    b.close()


# ------------------------------------------------------------------------------------------------------------------
# (2) - (4) sbmbp_batch_learning
# ------------------------------------------------------------------------------------------------------------------
# Seeds of the contract test. The oracle's synchronous learning (message form) was run on the CPU from every listed seed and
# the distance of lr * na_expect + (1 - lr) * na + snap to the nearest integer recorded at every truncation of every EM step;
# _oracle_learning repeats that and the tests assert it. Smallest distance per run:
#   c1_learn_515   seed 0: 0.222 (33 steps)   seed 3: 0.222 (33 steps)
#   q4_learn_seed2 seed 2: 3.4e-2 (39 steps)  seed 3: 3.3e-4 (74 steps)  seed 4: 2.3e-4 (71 steps)
# All are more than 1e-6 away from an integer boundary: no seed is left out.
CONTRACT = [("c1_learn_515_seed0", (0, 3)), ("q4_learn_seed2", (2, 3, 4))]
# different initial cab on the c1 dataset: the runs end in different rounds (oracle: 33, 1 and 1 EM steps)
C1_STARTS = (np.array([[5.0, 1.0], [1.0, 5.0]]), np.array([[4.0, 2.0], [2.0, 4.0]]), np.array([[3.63, 2.36], [2.36, 3.63]]))


@functools.lru_cache(maxsize=None)
def _oracle_learning(name, seed, start=-1):
    """the oracle's synchronous learning in message form, restated round by round with its own primitives so that the margin of
    every group-size truncation is seen; computed once, shared, read-only. Checked against OracleBP.learning itself."""
    import oracle as orc
    a = args_of(golden(name))
    runs = []
    for _ in range(2):
        _, ob, _ = oracle_from(orc, dict(a, seed=seed))
        if start >= 0:
            ob.set_params(C1_STARTS[start], ob.get_params()[1], a["beta"])
        ob.set_msg_form(True)
        runs.append(ob)
    ob, twin = runs
    N = a["N"]
    crit, lr, damp = np.float32(a["lcrit"]), float(np.float32(a["lr"])), float(np.float32(a["damp"]))
    ob.set_field_mix(0.3)
    fold, fdiff, steps, status, margin = 0.0, 1.0, 0, 0, 1.0
    for _ in range(a["tmax"]):
        if fdiff < crit:
            crit = np.float32(float(crit) * 0.1)
        ob.converge_sync(float(crit), a["tmax"], damp)
        na_e, _, cab_e = ob.em_expect()
        fnew, _ = ob.free_energy(0)
        fdiff, fold = abs(fnew - fold), fnew
        if not np.isfinite(fold):
            status = 2
            break
        if fdiff < crit:
            status = 1
            break
        cab, na = ob.get_params()
        x = lr * na_e[:-1] + (1.0 - lr) * na[:-1] + min(1.0 * N * float(crit), 0.01)
        margin = min(margin, float(np.min(np.minimum(x - np.floor(x), np.ceil(x) - x))))
        nn = na.copy()
        nn[:-1] = x.astype(np.int64)
        nn[-1] = N - nn[:-1].sum()
        ob.set_params(lr * cab_e + (1.0 - lr) * cab, nn, a["beta"])
        steps += 1
    cab, na = ob.get_params()
    tsteps, tf = twin.learning(a["lcrit"], a["tmax"], a["lr"], a["damp"], None, sync=True, series_K=0)
    tcab, tna = twin.get_params()
    assert tsteps == steps and tf == fold and np.array_equal(tcab, cab) and np.array_equal(tna, na)  # the restatement IS the oracle's loop
    psi, msg = ob.get_state()
    for v in (cab, na, psi, msg):
        v.setflags(write=False)
    return dict(steps=steps, status=status, f=fold, margin=margin, cab=cab, na=na, overlap=ob.overlap(), psi=psi, msg=msg)


def _learn_batch(S, a, seeds, starts=None):
    g = S.load_edge_list(a["path"], a["N"])
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    st = S.bp_param_from_direct(bm, a["pa"], a["cab_upper"])
    b = S.ReplicaBatch(g, a["Q"], a["dc"], len(seeds))
    b.init_messages(a["init_flag"], None, a["true_conf"], list(seeds), conditional=False)
    b.set_params(st, a["beta"])
    for r, k in enumerate(starts or ()):
        b.set_params(S.bp_blockmodel_state(C1_STARTS[k], st.na), a["beta"], r)
    return g, bm, st, b


def _learn_single(S, a, seed, start=None):
    g = S.load_edge_list(a["path"], a["N"])
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    st = S.bp_param_from_direct(bm, a["pa"], a["cab_upper"])
    if start is not None:
        st = S.bp_blockmodel_state(C1_STARTS[start], st.na)
    bp = S.bp_basic()
    bp.init_messages(bm, a["init_flag"], None, a["true_conf"], seed)
    bp.set_beta(a["beta"])
    bp.set_gather_mode(1)
    res = bp.learning(bm, st, a["lcrit"], a["tmax"], a["lr"], a["damp"])
    return bp, res


def test_an_early_finisher_stays_frozen(S, orc):
    """three starts on the c1 dataset that end in different rounds: the state of a replica that stopped learning early is the
    state of the same single-engine run, although the batch went on for dozens of rounds"""
    a = args_of(golden("c1_learn_515_seed0"))
    ref = [_oracle_learning("c1_learn_515_seed0", 0, k) for k in range(3)]
    print("oracle em_steps:", [x["steps"] for x in ref])
    assert len({x["steps"] for x in ref}) >= 2
    g, bm, st, b = _learn_batch(S, a, [0, 0, 0], starts=(0, 1, 2))
    res, eta, cab, best = b.learning(a["lcrit"], a["tmax"], a["lr"], a["damp"])
    steps = [x.em_steps for x in res]
    print("batch em_steps:", steps, "status:", [x.status for x in res], "sweeps:", [x.total_sweeps for x in res])
    assert len(set(steps)) >= 2 and steps == [x["steps"] for x in ref]
    early = int(np.argmin(steps))
    assert steps[early] < max(steps)
    for r in range(3):
        bp, sres = _learn_single(S, a, 0, r)
        (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
        if r == early or steps[r] == steps[early]:
            assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12, r
        assert (sres.em_steps, sres.status, sres.total_sweeps) == (res[r].em_steps, res[r].status, res[r].total_sweeps), r
        scab, sna = bp.get_params()
        bcab, bna, _ = b.get_params(r)
        assert list(sna) == list(bna) and np.abs(scab - bcab).max() <= 1e-9 * np.abs(scab).max()
    assert b.stats().sweeps == sum(x.total_sweeps for x in res)
    b.close()


@pytest.mark.parametrize("name,seeds", CONTRACT)
def test_every_replica_learns_as_a_single_engine_does(S, orc, name, seeds):
    gd = golden(name)
    a = args_of(gd)
    ref = [_oracle_learning(name, s) for s in seeds]
    print("oracle (steps, status, f, margin):", [(x["steps"], x["status"], x["f"], x["margin"]) for x in ref])
    assert all(x["margin"] > 1e-6 for x in ref)  # no truncation of the oracle's run sits at an integer boundary
    g, bm, st, b = _learn_batch(S, a, seeds)
    res, eta, cab, best = b.learning(a["lcrit"], a["tmax"], a["lr"], a["damp"])
    fs = [x.free_energy for x in res]
    print("batch (steps, status, sweeps, f, overlap):", [(x.em_steps, x.status, x.total_sweeps, x.free_energy, x.overlap) for x in res], "best", best)
    for r, s in enumerate(seeds):
        # (3) the contract: a single engine in message-gather form from the same start
        bp, sres = _learn_single(S, a, s)
        scab, sna = bp.get_params()
        bcab, bna, _ = b.get_params(r)
        assert (res[r].em_steps, res[r].status, res[r].total_sweeps) == (sres.em_steps, sres.status, sres.total_sweeps), r
        assert list(bna) == list(sna)
        assert np.array_equal(cab[r], bcab) and np.array_equal(eta[r], bna / float(a["N"]))
        assert np.abs(bcab - scab).max() <= 1e-9 * np.abs(scab).max()
        assert np.abs(eta[r] - sna / float(a["N"])).max() <= 1e-9
        assert abs(res[r].free_energy - sres.free_energy) <= 1e-9 and abs(res[r].overlap - sres.overlap) <= 1e-9
        # (4) the oracle's synchronous learning
        x = ref[r]
        assert res[r].em_steps == x["steps"] and res[r].status == x["status"] and list(bna) == list(x["na"])
        assert np.abs(bcab - x["cab"]).max() < 1e-6 * np.abs(x["cab"]).max() and abs(res[r].free_energy - x["f"]) < 1e-6
        assert abs(res[r].overlap - x["overlap"]) < 1e-6
    # best = the argmin among status 1, else among status 0; NaN never
    cand = [r for r in range(len(seeds)) if res[r].status == 1 and not np.isnan(fs[r])] or \
           [r for r in range(len(seeds)) if res[r].status == 0 and not np.isnan(fs[r])]
    assert best == (min(cand, key=lambda r: (fs[r], r)) if cand else 0)
    if name == "c1_learn_515_seed0":  # the reference's own (asynchronous) runs of the two commands: tests/test_gpu_parity.py's tolerances
        for r, s in enumerate(seeds):
            rr = golden("c1_learn_515_seed%d" % s)["result"]
            bcab, bna, _ = b.get_params(r)
            ref_cab = np.array(rr["cab_final"]).reshape(bcab.shape)
            assert list(bna) == list(rr["na_final"])
            assert np.abs(bcab - ref_cab).max() < 1e-7 * np.abs(ref_cab).max()
            assert abs(res[r].overlap - rr["overlap"]) < 1e-7
    b.close()


# ------------------------------------------------------------------------------------------------------------------
# (5) command line
# ------------------------------------------------------------------------------------------------------------------
BP = os.path.join(ROOT, "bin", "bp")


def _run(*args):
    p = subprocess.run([BP] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_learn_restarts(S, tmp_path):
    a = args_of(golden("c1_learn_515_seed0"))
    base = ["-l", gpath("c1_dataset.edgelist"), "-n"] + a["n"] + ["--pa"] + a["pa"] + ["--cab"] + a["cab_upper"] + ["-t", a["tmax"], "-m", "learn"]
    mj = tmp_path / "m.json"
    rc, out, err = _run(*base, "--seed", 0, "--learn_restarts", 3, "--precision", 12, "--metrics_json", mj)
    assert rc == 0, err
    g, bm, st, b = _learn_batch(S, a, [0, 1, 2])
    res, eta, cab, best = b.learning(a["lcrit"], a["tmax"], a["lr"], a["damp"])
    lines = out.strip("\n").split("\n")
    assert len(lines) == 1 + a["Q"]
    got_eta = np.array([float(v) for v in lines[0].split()])
    got_cab = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    assert np.abs(got_eta - eta[best]).max() < 1e-8 and np.abs(got_cab - cab[best]).max() < 1e-8
    m = json.load(open(mj))
    assert m["learn_restarts"] == 3 and m["best"] == best and m["seed"] == [0, 1, 2]
    assert m["em_steps"] == [x.em_steps for x in res] and m["status"] == [x.status for x in res]
    assert m["total_sweeps"] == [x.total_sweeps for x in res] and m["sweeps"] == sum(x.total_sweeps for x in res)
    assert np.abs(np.array(m["free_energy"]) - [x.free_energy for x in res]).max() < 1e-9
    per = [ln for ln in err.split("\n") if ln.startswith("restart ")]
    assert len(per) == 3 and all("seed %d " % s in ln and "em_steps" in ln and "status" in ln and "free_energy" in ln and "overlap" in ln
                                 for s, ln in enumerate(per))
    tail = [ln for ln in err.split("\n") if ln]
    assert tail[-1].startswith("overlap:") and abs(float(tail[-1].split(":")[1]) - res[best].overlap) < 1e-8
    b.close()
    # --learn_restarts 1 is the single-engine path, byte for byte
    rc0, plain, _ = _run(*base, "--seed", 0)
    rc1, one, _ = _run(*base, "--seed", 0, "--learn_restarts", 1)
    assert rc0 == 0 and rc1 == 0 and plain == one and len(plain.split("\n")) == 2 + a["Q"]
