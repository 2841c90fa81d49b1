"""CPU tier of the per-vertex prior (include/sbmbp.h sbmbp_set_vertex_prior): the test model against the oracle, the prior
file reader, the argument errors of the entry points that need no device, and the command line's --prior_path handling
(every conflict and file error ends with rc 1 and nothing on stdout, before any device work)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import prior_model as pm
from conftest import ROOT, gpath

BP = os.path.join(ROOT, "bin", "bp")
DS = gpath("c1_dataset.edgelist")


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    assert os.path.exists(BP)
    return S


def _oracle(orc, Q, dc, N=300, seed=5):
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, N, size=(3 * N, 2)).astype(np.uint32)
    pairs = np.concatenate([pairs, np.array([[7, i] for i in range(8, 108)], dtype=np.uint32)])  # one row above 32 edges
    og = orc.Graph.from_edges(pairs, N)
    ob = orc.OracleBP(og, Q, dc)
    tc = (np.arange(N) % Q).astype(np.uint32)
    na = np.bincount(tc, minlength=Q).astype(np.uint32)
    cab = rng.uniform(0.4, 1.6, size=(Q, Q))
    cab = (cab + cab.T) / 2 + np.eye(Q) * 1.5
    if dc:
        cab = cab / (og.E2 / N) ** 2
    ob.init_messages(0, None, tc, orc.Rng(seed))
    ob.set_params(cab, na, 1.0)
    return og, ob, cab, na


@pytest.mark.parametrize("Q,dc", [(2, 0), (3, 1), (5, 2), (16, 0)])
def test_model_with_one_class_of_weight_one_is_sweep_sync_bit_for_bit(orc, Q, dc):
    og, ob, cab, na = _oracle(orc, Q, dc)
    _, twin, _, _ = _oracle(orc, Q, dc)
    for damp in (0.7, 1.0, 1.0):
        d1 = pm.sweep(ob, cab, na, np.ones((1, Q), dtype=np.int64), np.zeros(og.N, dtype=np.int64), damp)
        psi0, msg0 = twin.get_state()
        d2 = twin.sweep_sync(damp)
        assert all(np.array_equal(x, y) for x, y in zip(ob.get_state(), twin.get_state()))
        md = np.abs(twin.get_state()[1] - msg0).max() / damp
        assert d1 == md and abs(d1 - d2) <= 1e-15  # (the oracle reports the undamped difference itself: no division by damp)


def test_model_stitches_classes_and_equals_the_numpy_restatement(orc):
    """three classes: every row of class c is the row of the oracle run with eta * w_c; and the sweep written out in numpy
    (used where the integer route cannot express the weights) agrees with both the oracle at weight 1 and the model"""
    Q = 3
    for dc in (0, 1):
        og, ob, cab, na = _oracle(orc, Q, dc)
        psi0, msg0 = ob.get_state()
        weights = np.array([[1, 1, 1], [3, 1, 2], [1, 5, 1]], dtype=np.int64)
        cls = np.arange(og.N) % 3
        p1, m1, d1 = pm.numpy_sweep(og.row_ptr, og.nbr, og.rev, psi0, msg0, cab, na, np.ones((og.N, Q)), dc, 1.0)
        _, twin, _, _ = _oracle(orc, Q, dc)
        d2 = twin.sweep_sync(1.0)
        assert np.abs(p1 - twin.get_state()[0]).max() < 1e-13 and np.abs(m1 - twin.get_state()[1]).max() < 1e-13 and abs(d1 - d2) < 1e-13
        d = pm.sweep(ob, cab, na, weights, cls, 0.7)
        p2, m2, d3 = pm.numpy_sweep(og.row_ptr, og.nbr, og.rev, psi0, msg0, cab, na, pm.classes_of(weights, cls), dc, 0.7)
        assert np.abs(p2 - ob.get_state()[0]).max() < 1e-13 and np.abs(m2 - ob.get_state()[1]).max() < 1e-13 and abs(d - d3) < 1e-13
        assert np.abs(ob.get_state()[0][cls == 1] - twin.get_state()[0][cls == 1]).max() > 1e-3  # the prior moves the rows it names
        assert list(ob.get_params()[1]) == list(na)


def _load(S, path, N, Q):
    lib = S.load_library()
    pr = np.full((N, Q), -7.0)
    given = C.c_uint64(99)
    rc = lib.sbmbp_prior_load(os.fsencode(str(path)), N, Q, pr.ctypes.data_as(C.POINTER(C.c_double)), C.byref(given))
    return rc, pr, given.value, lib.sbmbp_last_error().decode()


BAD_FILES = {
    "vertex id >= N": ("5 1 2 3\n", "5 >= N"),
    "vertex named twice": ("0 3 3 3\n", "named twice"),
    "too few columns": ("1 1 2\n", "2 weights"),
    "too many columns": ("1 1 2 3 4\n", "4 weights"),
    "not a number": ("1 1 x 3\n", "bad value"),
    "negative": ("1 1 -2 3\n", "bad value"),
    "nan": ("1 1 nan 3\n", "bad value"),
    "inf": ("1 inf 2 3\n", "bad value"),
    "no positive weight": ("1 0 0 0\n", "bad value"),
    "bad vertex id": ("-1 1 2 3\n", "vertex id"),
}


def test_prior_load_good_and_bad_files(S, tmp_path):
    p = tmp_path / "prior.txt"
    p.write_text("3 0.5 0 2\n\n0 1e-3 1 1\n 2\t7 8 9 \r\n")
    rc, pr, given, _ = _load(S, p, 5, 3)
    assert rc == 0 and given == 3
    assert np.array_equal(pr, [[1e-3, 1, 1], [1, 1, 1], [7, 8, 9], [0.5, 0, 2], [1, 1, 1]])
    assert np.array_equal(S.load_priors(str(p), 5, 3), pr)
    p.write_text("")
    rc, pr, given, _ = _load(S, p, 4, 2)
    assert rc == 0 and given == 0 and (pr == 1.0).all()
    for what, (text, needle) in BAD_FILES.items():
        p.write_text("0 1 1 1\n" + text)
        rc, _, _, msg = _load(S, p, 5, 3)
        assert rc == -1 and needle in msg and "line 2" in msg, (what, rc, msg)
    rc, _, _, msg = _load(S, tmp_path / "missing.txt", 5, 3)
    assert rc == -5 and "missing.txt" in msg
    with pytest.raises(S.SbmbpError) as ei:
        S.load_priors(str(tmp_path / "missing.txt"), 5, 3)
    assert ei.value.code == -5
    lib = S.load_library()
    assert lib.sbmbp_prior_load(None, 5, 3, None, None) == -1


def test_entry_points_without_an_engine_or_a_device(S):
    lib = S.load_library()
    pr = np.ones((4, 2))
    present = C.c_int(5)
    assert lib.sbmbp_set_vertex_prior(None, pr.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert b"sbmbp_set_vertex_prior" in lib.sbmbp_last_error()
    assert lib.sbmbp_set_vertex_prior(None, None) == -1
    assert lib.sbmbp_get_vertex_prior(None, None, C.byref(present)) == -1
    bp = S.bp_basic()
    with pytest.raises(S.SbmbpError) as ei:  # no engine yet
        bp.set_vertex_prior(np.ones((4, 2)))
    assert ei.value.code == -1
    import torch
    if not torch.cuda.is_available():
        g = S.load_edge_list(DS, 1000)
        with pytest.raises(S.SbmbpError) as ei:  # the engine is what holds a prior, and there is none without a GPU
            bp.init_messages(S.blockmodel_t(g, 2, 0), 0, None, np.repeat([0, 1], 500), 0)
        assert ei.value.code == -3


def run(*args):
    p = subprocess.run([BP] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


BASE = ["-l", DS, "-n", 500, 500, "--epsilon_c", 0.1, 3, "-d", 0]


def test_cli_help_lists_the_option(S):
    rc, out, err = run("-h")
    assert rc == 0 and out == "" and "--prior_path" in err


def test_cli_conflicts(S, tmp_path):
    p = tmp_path / "prior.txt"
    p.write_text("0 2 1\n")
    cases = [
        (["-m", "infer", "--gpus", 2], "--gpus"),
        (["-m", "infer", "--restarts", 2], "--restarts"),
        (["-m", "learn", "--learn_restarts", 2], "--learn_restarts"),
        (["-m", "infer", "--schedule", "coloured"], "--schedule coloured"),
    ]
    for extra, other in cases:
        rc, out, err = run(*BASE, *extra, "--prior_path", p)
        assert rc == 1 and out == "" and "--prior_path" in err and other in err, (extra, rc, out, err)
    n20 = ["-l", DS, "-n"] + [50] * 20 + ["--epsilon_c", 0.1, 3, "-d", 0, "-m", "infer"]
    rc, out, err = run(*n20, "--prior_path", p)
    assert rc == 1 and out == "" and "--prior_path" in err and "Q > 16" in err


def test_cli_file_errors(S, tmp_path):
    p = tmp_path / "prior.txt"
    for mode in ("infer", "learn"):
        rc, out, err = run(*BASE, "-m", mode, "--prior_path", tmp_path / "missing.txt")
        assert rc == 1 and out == "" and "--prior_path" in err and "missing.txt" in err
    bad = {"1000 1 2\n": "1000 >= N", "3 1 2\n3 1 2\n": "named twice", "3 1 2 3\n": "3 weights", "3 1\n": "1 weights",
           "3 1 x\n": "bad value", "3 -1 2\n": "bad value", "3 0 0\n": "bad value"}
    for text, needle in bad.items():
        p.write_text(text)
        rc, out, err = run(*BASE, "-m", "infer", "--prior_path", p)
        assert rc == 1 and out == "" and "--prior_path" in err and needle in err, (text, rc, out, err)
