"""CPU-side checks of the two entry points of the extended layout (rsba_solver_set_extended_layout,
rsba_solver_num_extended_parameters): exports, EXPORTS and the header agree, and the argument checks that need no device — a NULL
solver.  (With a device, tests/test_gpu_marker_intrinsics_queries.py covers what they do.)"""
import os
import re

import pytest

from realsensecalibration_amd import capi

NAMES = ("rsba_solver_set_extended_layout", "rsba_solver_num_extended_parameters")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsba.h")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def test_exports_and_header_agree():
    lib = capi.load()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert "int rsba_solver_set_extended_layout(rsba_solver* s, int32_t on);" in text
    assert "int64_t rsba_solver_num_extended_parameters(const rsba_solver* s);" in text
    for name in ("set_extended_layout", "num_extended_parameters", "intrinsics_offset"):
        assert hasattr(capi.Solver, name), name


def test_null_solver():
    lib = capi.load()
    assert lib.rsba_solver_set_extended_layout(None, 1) == capi.ERR_ARG
    assert lib.rsba_solver_set_extended_layout(None, 0) == capi.ERR_ARG
    assert lib.rsba_solver_num_extended_parameters(None) == -capi.ERR_ARG
