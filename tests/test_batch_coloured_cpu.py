"""CPU tier of the coloured sweep order of replica batches (include/sbmbp.h sbmbp_batch_set_sweep_order /
sbmbp_batch_get_sweep_order): the symbols are there from the header to ReplicaBatch, a null batch is an argument error before
any device work, and the command line keeps refusing --restarts with --schedule coloured."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, gpath

NAMES = ("sbmbp_batch_set_sweep_order", "sbmbp_batch_get_sweep_order")


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def test_both_symbols_from_the_header_to_the_bindings(S):
    from sbm_bp_amd.capi import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sbmbp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sbmbp_batch_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(S.lib_path())
    for name in NAMES:
        assert name in declared and name in SYMBOLS and getattr(raw, name) is not None, name
    # the argument lists are the single engine's, with the batch in place of the engine
    assert SYMBOLS["sbmbp_batch_set_sweep_order"] == SYMBOLS["sbmbp_set_sweep_order"]
    assert SYMBOLS["sbmbp_batch_get_sweep_order"] == SYMBOLS["sbmbp_get_sweep_order"]


def test_replica_batch_has_the_method_and_the_property(S):
    import inspect
    assert callable(S.ReplicaBatch.set_sweep_order) and isinstance(S.ReplicaBatch.sweep_order, property)
    mine = inspect.signature(S.ReplicaBatch.set_sweep_order)
    single = inspect.signature(S.BeliefPropagation.set_sweep_order)
    assert [(p.name, p.default) for p in mine.parameters.values()] == [(p.name, p.default) for p in single.parameters.values()]


def test_a_null_batch_is_an_argument_error_before_any_device_work(S):
    lib = S.load_library()
    o, nc, ns = C.c_int(7), C.c_uint32(7), C.c_uint32(7)
    for order in (0, 1, 2, -1):
        assert lib.sbmbp_batch_set_sweep_order(None, order, None, 0.0) == -1
    assert lib.sbmbp_batch_get_sweep_order(None, C.byref(o), C.byref(nc), C.byref(ns)) == -1
    assert (o.value, nc.value, ns.value) == (7, 7, 7)  # nothing is written
    assert lib.sbmbp_batch_get_sweep_order(None, None, None, None) == -1


def test_cli_keeps_refusing_restarts_in_the_coloured_order(S):
    bp = os.path.join(ROOT, "bin", "bp")
    p = subprocess.run([bp, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--restarts" in p.stderr and "--learn_restarts" in p.stderr
    base = [bp, "-l", gpath("c1_dataset.edgelist"), "-n", "500", "500", "--epsilon_c", "0.1", "3.0"]
    for extra, flag in ((["-m", "infer", "--restarts", "2", "--schedule", "coloured"], "--restarts"),
                        (["-m", "learn", "--learn_restarts", "2", "--schedule", "coloured"], "--learn_restarts")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout == "" and flag in p.stderr and "coloured" in p.stderr, (extra, p.stderr)
        # the refusal says where the combination does exist
        assert "sbmbp_batch_set_sweep_order" in p.stderr and "ReplicaBatch.set_sweep_order" in p.stderr, p.stderr
