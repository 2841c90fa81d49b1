"""CPU tier of the per-vertex priors of replica batches (include/sbmbp.h sbmbp_batch_set_vertex_prior /
sbmbp_batch_get_vertex_prior): the symbols are declared, exported and listed, a null batch is an argument error before any
device work, and ReplicaBatch carries the two methods."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NAMES = ("sbmbp_batch_set_vertex_prior", "sbmbp_batch_get_vertex_prior")


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.build_all()
    S.load_library()
    return S


def test_header_library_and_symbol_table_agree(S):
    from sbm_bp_amd.capi import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sbmbp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = C.CDLL(S.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(raw, name) is not None and name in SYMBOLS, name
    res, args = SYMBOLS["sbmbp_batch_set_vertex_prior"]
    assert res is C.c_int and args[1] is C.c_int and len(args) == 3  # the replica is signed: -1 = all
    res, args = SYMBOLS["sbmbp_batch_get_vertex_prior"]
    assert res is C.c_int and args[1] is C.c_uint32 and len(args) == 4
    # the header no longer says that batches take no prior, and documents the three states and the two consequences
    assert "Replica batches and sbmbp_dist_* take no prior" not in hdr
    doc = hdr[hdr.index("Per-vertex label priors of a batch"):hdr.index("int sbmbp_batch_set_vertex_prior")]
    for word in ("NONE", "SHARED", "OWN", "ones that the batch keeps", "-log(c)/N", "same table", "SBMBP_ERR_NOMEM"):
        assert word in doc, word


def test_a_null_batch_is_an_argument_error(S):
    lib = S.load_library()
    table = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    present = C.c_int(7)
    assert lib.sbmbp_batch_set_vertex_prior(None, -1, table) == -1
    assert lib.sbmbp_batch_set_vertex_prior(None, 0, None) == -1
    assert lib.sbmbp_batch_get_vertex_prior(None, 0, None, C.byref(present)) == -1 and present.value == 7
    assert lib.sbmbp_batch_get_vertex_prior(None, 0, table, None) == -1


def test_replica_batch_has_both_methods(S):
    import inspect
    sig = inspect.signature(S.ReplicaBatch.set_vertex_prior)
    assert list(sig.parameters) == ["self", "prior", "replica"] and sig.parameters["replica"].default == -1
    assert list(inspect.signature(S.ReplicaBatch.vertex_prior).parameters) == ["self", "replica"]
