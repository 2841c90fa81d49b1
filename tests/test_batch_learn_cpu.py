"""CPU tier of multi-start EM (include/sbmbp.h: sbmbp_batch_learning and the host functions it shares with sbmbp_learning):
the learning step and the best-replica rule are host code and are checked here without a device; so are the argument checks of
the batch calls and the command line's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, args_of, golden, gpath
from test_gpu_parity import oracle_from


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def _dp(x):
    return x.ctypes.data_as(C.POINTER(C.c_double))


def step_host(lib, N, lr, snap, crit, na_e, cab_e, na, cab):
    Q = len(na)
    na = np.array(na, dtype=np.uint32)
    cab = np.array(cab, dtype=np.float64).reshape(Q, Q).copy()
    na_e = np.ascontiguousarray(na_e, dtype=np.float64)
    cab_e = np.ascontiguousarray(cab_e, dtype=np.float64)
    rc = lib.sbmbp_learning_step_host(Q, N, lr, snap, crit, _dp(na_e), _dp(cab_e), na.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(cab))
    assert rc == 0
    return na, cab


def step_numpy(N, lr, snap, crit, na_e, cab_e, na, cab):
    """belief_propagation.cpp:53-75 with the snap rule of sbmbp_set_learning_schedule"""
    Q = len(na)
    s = min(snap * N * crit, 0.01)
    out = np.zeros(Q, dtype=np.int64)
    for i in range(Q - 1):
        out[i] = int(lr * na_e[i] + (1.0 - lr) * na[i] + s)  # truncation towards zero (:58-63)
    out[Q - 1] = N - out[:Q - 1].sum()  # the last group takes the rest (:64)
    return out, lr * np.asarray(cab_e, dtype=np.float64).reshape(Q, Q) + (1.0 - lr) * np.asarray(cab, dtype=np.float64).reshape(Q, Q)


@pytest.mark.parametrize("Q", [2, 5])
@pytest.mark.parametrize("lr", [1.0, 0.3])
@pytest.mark.parametrize("snap", [1.0, 0.0])
def test_learning_step_host_equals_the_restatement(S, Q, lr, snap):
    lib = S.load_library()
    rng = np.random.default_rng(100 * Q + int(10 * lr) + int(snap))
    N, crit = 1000, 1e-6
    na = rng.multinomial(N, np.ones(Q) / Q)
    na_e = rng.dirichlet(np.ones(Q) * 50) * N
    cab = rng.uniform(0.5, 8.0, (Q, Q))
    cab = (cab + cab.T) / 2
    cab_e = rng.uniform(0.5, 8.0, (Q, Q))
    # group 0 lands 1e-7 below an integer: with the snap rule (min(1 * 1000 * 1e-6, 0.01) = 1e-3 above it) it IS that integer,
    # without it the reference's truncation takes the integer below
    target = 237
    na_e[0] = (target - 1e-7 - (1.0 - lr) * na[0]) / lr
    got_na, got_cab = step_host(lib, N, lr, snap, crit, na_e, cab_e, na, cab)
    want_na, want_cab = step_numpy(N, lr, snap, crit, na_e, cab_e, na, cab)
    assert list(got_na) == list(want_na) and got_na.sum() == N
    assert got_na[0] == (target if snap else target - 1)
    assert got_na[Q - 1] == N - got_na[:Q - 1].sum()
    assert np.array_equal(got_cab, want_cab)
    if lr == 1.0:
        assert np.array_equal(got_cab, cab_e)


def test_learning_step_host_snap_is_capped_and_scaled(S):
    lib = S.load_library()
    cab = np.eye(2)
    # snap * N * crit = 1e-3 * 1e5 = 100 -> capped at 0.01: 499.98 stays 499, 499.995 becomes 500
    assert step_host(lib, 100000, 1.0, 1.0, 1e-3, [499.98, 0.0], cab, [0, 0], cab)[0][0] == 499
    assert step_host(lib, 100000, 1.0, 1.0, 1e-3, [499.995, 0.0], cab, [0, 0], cab)[0][0] == 500
    # a tighter criterion narrows the window: N * crit = 1e-5
    assert step_host(lib, 1000, 1.0, 1.0, 1e-8, [499.9999, 0.0], cab, [0, 0], cab)[0][0] == 499
    assert step_host(lib, 1000, 1.0, 1.0, 1e-8, [499.999995, 0.0], cab, [0, 0], cab)[0][0] == 500


def test_learning_step_host_follows_the_oracles_first_em_step(S, orc):
    """c1_learn_515: two oracles from the same converged state. One runs its synchronous learning for ONE round (one BP sweep,
    expectations, learning_step); the other runs the same sweep and hands its em_expect to sbmbp_learning_step_host."""
    lib = S.load_library()
    a = args_of(golden("c1_learn_515_seed0"))
    pair = []
    for _ in range(2):
        _, ob, _ = oracle_from(orc, a)
        ob.converge_sync(1e-3, 200, 1.0)  # not a fixed point yet: the expectations move the parameters visibly
        pair.append(ob)
    cab0, na0 = pair[0].get_params()
    steps, _ = pair[0].learning(a["lcrit"], 1, a["lr"], a["damp"], None, sync=True, series_K=0)
    assert steps == 1
    want_cab, want_na = pair[0].get_params()
    pair[1].set_field_mix(0.3)
    pair[1].converge_sync(float(np.float32(a["lcrit"])), 1, a["damp"])
    na_e, _, cab_e = pair[1].em_expect()
    lr = float(np.float32(a["lr"]))  # the learning rate arrives as a float in sbmbp_learning and in the oracle
    got_na, got_cab = step_host(lib, a["N"], lr, 1.0, float(np.float32(a["lcrit"])), na_e, cab_e, na0, cab0)
    assert list(got_na) == list(want_na)
    assert np.abs(got_cab - want_cab).max() <= 4e-16 * np.abs(want_cab).max()  # the same two products and one sum per entry
    assert np.abs(got_cab - cab0).max() > 1e-3  # the step did move the parameters


def best(lib, f, rank, n_ranks=2):
    f = np.array(f, dtype=np.float64)
    rank = np.array(rank, dtype=np.int32)
    out = C.c_uint32(99)
    assert lib.sbmbp_best_replica(len(f), _dp(f), rank.ctypes.data_as(C.POINTER(C.c_int)), n_ranks, C.byref(out)) == 0
    return out.value


def learn_rank(status):
    """sbmbp_batch_learning: status 1 (stopped on fdiff < crit) before status 0 (out of steps); status 2 (NaN/Inf) never"""
    return [0 if s == 1 else (1 if s == 0 else -1) for s in status]


def test_best_replica_rule(S):
    lib = S.load_library()
    nan = float("nan")
    # status preference: a converged run wins over a lower free energy that ran out of steps
    assert best(lib, [-3.0, -2.0, -2.5], learn_rank([0, 1, 1])) == 2
    # no status 1: the best among status 0
    assert best(lib, [-3.0, -2.0, -3.5], learn_rank([0, 0, 0])) == 2
    # NaN never, whatever its status; status 2 never
    assert best(lib, [nan, -1.0, -0.5], learn_rank([1, 1, 1])) == 1
    assert best(lib, [nan, -1.0, -7.0], learn_rank([1, 0, 2])) == 1
    assert best(lib, [nan, nan], learn_rank([1, 0])) == 0 and best(lib, [-1.0, -2.0], learn_rank([2, 2])) == 0
    # ties to the lowest index
    assert best(lib, [-2.0, -2.0, -2.0], learn_rank([1, 1, 1])) == 0
    assert best(lib, [-1.0, -2.0, -2.0], learn_rank([1, 1, 1])) == 1
    # the inference ranking of sbmbp_batch_inference: converged runs first, all the others next
    assert best(lib, [-5.0, -1.0], [1, 0]) == 1 and best(lib, [-5.0, -1.0], [1, 1]) == 0
    assert lib.sbmbp_best_replica(0, None, None, 2, None) == -1


def test_argument_errors_of_the_batch_calls_need_no_device(S):
    lib = S.load_library()
    from sbm_bp_amd.capi import SYMBOLS, LearnResult
    res = (LearnResult * 2)()
    assert lib.sbmbp_batch_set_learning_schedule(None, 0.3, 1.0) == -1
    assert lib.sbmbp_batch_em_step(None, None, None, None, None, None) == -1
    assert lib.sbmbp_batch_learning(None, 1e-6, 10, 0.2, 1.0, res, None, None, None) == -1
    x = np.zeros(4)
    n = np.zeros(2, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.sbmbp_learning_step_host(2, 10, 0.2, 1.0, 1e-6, None, _dp(x), n.ctypes.data_as(u32p), _dp(x)) == -1
    assert lib.sbmbp_learning_step_host(2, 10, 0.2, 1.0, 1e-6, _dp(x), _dp(x), None, _dp(x)) == -1
    assert lib.sbmbp_learning_step_host(0, 10, 0.2, 1.0, 1e-6, _dp(x), _dp(x), n.ctypes.data_as(u32p), _dp(x)) == -1
    for name in ("sbmbp_batch_set_learning_schedule", "sbmbp_batch_em_step", "sbmbp_batch_learning", "sbmbp_learning_step_host",
                 "sbmbp_best_replica"):
        assert name in SYMBOLS
    for name in ("em_step", "learning", "set_learning_schedule"):
        assert callable(getattr(S.ReplicaBatch, name))


def test_cli_help_lists_learn_restarts_and_conflicts_need_no_gpu(S):
    bp = os.path.join(ROOT, "bin", "bp")
    p = subprocess.run([bp, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--learn_restarts" in p.stderr
    base = [bp, "-l", gpath("c1_dataset.edgelist"), "-n", "500", "500", "--epsilon_c", "0.1", "3.0"]
    for extra, word in ((["-m", "infer", "--learn_restarts", "2"], "infer"), (["-m", "learn", "--learn_restarts", "2", "--gpus", "2"], "--gpus"),
                        (["-m", "learn", "--learn_restarts", "2", "--schedule", "coloured"], "coloured"),
                        (["-m", "learn", "--learn_restarts", "0"], "at least 1"), (["-m", "learn", "--learn_restarts", "-3"], "at least 1")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout == "" and "--learn_restarts" in p.stderr and word in p.stderr, (extra, p.stderr)
    many = [bp, "-l", gpath("q10_n1000.edgelist"), "-n"] + ["50"] * 20 + ["--epsilon_c", "0.1", "5.0", "-m", "learn", "--learn_restarts", "2"]
    p = subprocess.run(many, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout == "" and "--learn_restarts" in p.stderr and "16" in p.stderr
    # --restarts with -m learn keeps its own refusal
    p = subprocess.run(base + ["-m", "learn", "--restarts", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout == "" and "--restarts" in p.stderr and "learn" in p.stderr


def test_cli_learn_restarts_conflict_is_named_before_a_restarts_batch_runs(S):
    """--restarts and --learn_restarts together: -m infer is a conflict of --learn_restarts, named before any device work"""
    bp = os.path.join(ROOT, "bin", "bp")
    p = subprocess.run([bp, "-l", gpath("c1_dataset.edgelist"), "-n", "500", "500", "--epsilon_c", "0.1", "3.0", "-m", "infer", "--restarts", "3",
                        "--learn_restarts", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout == "" and "--learn_restarts" in p.stderr and "infer" in p.stderr
