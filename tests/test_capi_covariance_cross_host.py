"""CPU-side checks of the general covariance queries of the C ABI (rsba_solver_covariance_blocks, rsba_solver_time_covariances):
exported, declared, bound, and a NULL solver refused before any device is touched; the older single-pair call keeps its contract."""
import ctypes as C
import os
import re

import pytest

from realsensecalibration_amd import capi

NAMES = ("rsba_solver_covariance_blocks", "rsba_solver_time_covariances")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsba.h")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def test_exports_and_header_agree():
    lib = capi.load()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi._SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert "int rsba_solver_covariance_blocks(rsba_solver* s, int64_t num_pairs, const int64_t* offsets_a, const int64_t* offsets_b, double* out);" in text
    assert "int rsba_solver_time_covariances(rsba_solver* s, double* out);" in text


def test_null_solver_is_an_argument_error():
    lib = capi.load()
    a = (C.c_int64 * 1)(0)
    out = (C.c_double * 36)()
    assert lib.rsba_solver_covariance_blocks(None, 1, a, a, out) == capi.ERR_ARG
    assert lib.rsba_solver_covariance_blocks(None, 0, None, None, None) == capi.ERR_ARG
    assert lib.rsba_solver_time_covariances(None, out) == capi.ERR_ARG
    assert lib.rsba_solver_time_covariances(None, None) == capi.ERR_ARG


def test_the_single_pair_call_keeps_its_contract():
    """The comment above rsba_solver_covariance_block still names RSBA_ERR_UNSUPPORTED and points to the general call."""
    text = open(HEADER).read()
    at = text.index("int rsba_solver_covariance_block(const rsba_solver* s")
    comment = text[text.rindex("/*", 0, at):at]
    assert "RSBA_ERR_UNSUPPORTED" in comment and "rsba_solver_covariance_blocks" in comment


def test_python_binding_has_the_queries():
    for name in ("covariance_blocks", "time_covariances", "time_offset", "marker_offset", "camera_offset", "point_offset"):
        assert callable(getattr(capi.Solver, name)), name
