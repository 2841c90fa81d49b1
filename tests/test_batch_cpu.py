"""CPU tier of the replica batches (include/sbmbp.h sbmbp_batch_*): the symbols are there, the argument checks come before
any device work, and without a GPU the batch fails as loudly as the single engine does."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, gpath


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def test_every_batch_symbol_of_the_header_is_exported(S):
    from sbm_bp_amd.capi import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sbmbp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sbmbp_batch_[a-z0-9_]+)\s*\(", hdr))
    for name in ("create", "destroy", "init_messages", "init_messages_device", "set_state", "get_state", "get_field", "get_relaxation",
                 "set_params", "get_params", "set_schedule", "set_auto_relax", "sweep", "converge", "free_energy", "entropy", "overlap",
                 "em_expectations", "inference", "get_stats"):
        assert "sbmbp_batch_" + name in declared, name
    raw = C.CDLL(S.lib_path())
    for name in declared:
        assert getattr(raw, name) is not None and name in SYMBOLS, name
    assert S.ReplicaBatch is not None


def test_argument_errors_come_before_any_device_work(S):
    lib = S.load_library()
    g = S.load_edge_list(gpath("c1_dataset.edgelist"), 1000)
    h = C.c_void_p()
    # (a machine with a GPU answers the same: none of these reaches the device)
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 2, 0, 0, 0) == -1 and b"n_replicas" in lib.sbmbp_last_error()
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 1, 0, 2, 0) == -1 and b"Q" in lib.sbmbp_last_error()
    assert lib.sbmbp_batch_create(C.byref(h), None, 2, 0, 2, 0) == -1
    assert lib.sbmbp_batch_create(None, g._h, 2, 0, 2, 0) == -1
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 2, 3, 2, 0) == -1 and b"deg_corr_flag" in lib.sbmbp_last_error()
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 2, 0, 70000, 0) == -1 and b"65535" in lib.sbmbp_last_error()
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 20, 0, 2, 0) == -6 and b"Q = 16" in lib.sbmbp_last_error()
    assert h.value is None
    # a null batch is an argument error everywhere, and destroying it is a no-op
    assert lib.sbmbp_batch_sweep(None, 1.0, 1, None) == -1 and lib.sbmbp_batch_get_stats(None, None) == -1
    assert lib.sbmbp_batch_num_replicas(None) == 0
    lib.sbmbp_batch_destroy(None)


def test_without_a_gpu_the_batch_fails_as_the_engine_does(S):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = S.load_library()
    g = S.load_edge_list(gpath("c1_dataset.edgelist"), 1000)
    h = C.c_void_p()
    assert lib.sbmbp_batch_create(C.byref(h), g._h, 2, 0, 3, 0) == -3 and b"no CPU fallback" in lib.sbmbp_last_error()
    assert h.value is None
    with pytest.raises(S.SbmbpError) as ei:
        S.ReplicaBatch(g, 2, 0, 3)
    assert ei.value.code == -3


def test_cli_help_lists_restarts_and_conflicts_need_no_gpu(S):
    bp = os.path.join(ROOT, "bin", "bp")
    p = subprocess.run([bp, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--restarts" in p.stderr
    base = [bp, "-l", gpath("c1_dataset.edgelist"), "-n", "500", "500", "--epsilon_c", "0.1", "3.0"]
    for extra, word in ((["-m", "learn", "--restarts", "2"], "learn"), (["-m", "infer", "--restarts", "2", "--gpus", "2"], "--gpus"),
                        (["-m", "infer", "--restarts", "2", "--schedule", "coloured"], "coloured"), (["-m", "infer", "--restarts", "0"], "at least 1"),
                        (["-m", "infer", "--restarts", "-3"], "at least 1")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout == "" and "--restarts" in p.stderr and word in p.stderr, (extra, p.stderr)
    many = [bp, "-l", gpath("q10_n1000.edgelist"), "-n"] + ["50"] * 20 + ["--epsilon_c", "0.1", "5.0", "-m", "infer", "--restarts", "2"]
    p = subprocess.run(many, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout == "" and "--restarts" in p.stderr and "16" in p.stderr
