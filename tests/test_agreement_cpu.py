"""CPU tier of replica agreement (include/sbmbp.h sbmbp_batch_agreement / sbmbp_agreement_groups): the symbols exist at every
layer, the group rule through ctypes against tests/agreement_model.py, the assignment under the host sanitizers, and the
command line's refusals. No compute entry point is called here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import agreement_model as M
from conftest import ROOT, gpath

BP = os.path.join(ROOT, "bin", "bp")
Q10 = gpath("q10_n1000.edgelist")


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def test_the_symbols_exist_at_every_layer(S):
    from sbm_bp_amd.capi import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sbmbp.h")).read()
    lib = S.load_library()
    for name in ("sbmbp_batch_agreement", "sbmbp_agreement_groups"):
        assert "int %s(" % name in hdr and name in SYMBOLS and getattr(lib, name)
    for name, val in (("SBMBP_AGREE_SOFT", 0), ("SBMBP_AGREE_HARD_SOFT", 1), ("SBMBP_AGREE_HARD", 2)):
        assert "#define %s %d" % (name, val) in hdr
    assert callable(S.ReplicaBatch.agreement) and callable(S.ReplicaBatch.agreement_groups) and callable(S.agreement_groups)
    # a null batch is an argument error, with a reason, before any device work
    assert lib.sbmbp_batch_agreement(None, 2, None, 0, None, None, None) == -1
    assert b"null batch" in lib.sbmbp_last_error()


def _groups(S, ov, t):
    g, n = S.agreement_groups(np.asarray(ov, dtype=np.float64), t)
    mg, mn = M.groups(ov, t)
    assert n == mn and g.dtype == np.uint32 and np.array_equal(g, mg), (ov, t, g, mg)
    return list(g), n


def test_groups_follow_the_leader_rule(S):
    assert _groups(S, np.eye(4), 0.5) == ([0, 1, 2, 3], 4)
    assert _groups(S, np.ones((5, 5)), 1.0) == ([0] * 5, 1)
    # 0-1 and 1-2 pass, 0-2 does not: 2 is compared with the LEADER 0 alone and leads a group of its own
    chain = np.array([[1.0, 0.95, 0.2], [0.95, 1.0, 0.95], [0.2, 0.95, 1.0]])
    assert _groups(S, chain, 0.9) == ([0, 0, 1], 2)
    # a fourth run close to 2 but not to 0 joins 2; the comparison is >=
    ov4 = np.array([[1.0, 0.95, 0.2, 0.1], [0.95, 1.0, 0.95, 0.3], [0.2, 0.95, 1.0, 0.9], [0.1, 0.3, 0.9, 1.0]])
    assert _groups(S, ov4, 0.9) == ([0, 0, 1, 1], 2)
    assert _groups(S, np.zeros((0, 0)), 0.5) == ([], 0)
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 16, 33):
        for t in (0.2, 0.5, 0.8):
            a = rng.random((n, n))
            ov = (a + a.T) / 2
            np.fill_diagonal(ov, 1.0)
            _groups(S, ov, t)
    # straight through ctypes, with the matrix only read
    lib = S.load_library()
    ov = np.ascontiguousarray(chain)
    g = np.full(3, 99, dtype=np.uint32)
    n = C.c_uint32(99)
    assert lib.sbmbp_agreement_groups(3, ov.ctypes.data_as(C.POINTER(C.c_double)), 0.9, g.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)) == 0
    assert list(g) == [0, 0, 1] and n.value == 2 and np.array_equal(ov, chain)
    assert lib.sbmbp_agreement_groups(3, None, 0.9, g.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)) == -1
    with pytest.raises(ValueError):
        S.agreement_groups(np.ones((2, 3)), 0.5)


def test_assignment_and_groups_under_asan_ubsan(tmp_path):
    """best_assignment and agreement_groups of csrc/host_reduce.h (plain C++, no device types) compiled on their own with
    -fsanitize=address,undefined by tests/sanitize/agreement_sanitize.cpp: the brute-force maximum for Q = 2 .. 9, a planted
    permutation for Q = 10 .. 16, matrices on which every assignment ties"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "agreement_sanitize"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-mavx2", "-pthread",
                    "-o", str(exe), os.path.join(ROOT, "tests", "sanitize", "agreement_sanitize.cpp")], check=True, timeout=600)
    pr = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, TMPDIR=str(tmp_path), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert pr.returncode == 0 and "agreement_sanitize ok" in pr.stdout, (pr.stdout[-500:], pr.stderr[-3000:])
    assert "runtime error" not in pr.stderr and "AddressSanitizer" not in pr.stderr and "LeakSanitizer" not in pr.stderr


def _bp(*args):
    p = subprocess.run([BP] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_command_line_lists_and_refuses(S):
    rc, out, err = _bp("-h")
    assert rc == 0 and "--agreement" in err
    base = ["-l", Q10, "-n"] + [100] * 10 + ["--epsilon_c", 0.1, 8, "-m", "infer", "-d", 1]
    cases = [
        base + ["--agreement", 0.9],                                      # no restarts at all
        base + ["--restarts", 1, "--agreement", 0.9],                     # not above 1
        base + ["--restarts", 3, "--agreement", 0],                       # T outside (0, 1]
        base + ["--restarts", 3, "--agreement", 1.5],
        base + ["--restarts", 3, "--agreement", -0.5],
        base + ["--restarts", 26, "--agreement", 0.9],                    # R Q = 260 > 256
        base[:-4] + ["-m", "learn", "-d", 1, "--learn_restarts", 26, "--agreement", 0.9],
        base[:-4] + ["-m", "learn", "-d", 1, "--agreement", 0.9],
    ]
    for args in cases:
        rc, out, err = _bp(*args)
        assert rc == 1 and out == "" and "--agreement" in err, (args, rc, out, err)
