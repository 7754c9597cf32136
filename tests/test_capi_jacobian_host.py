"""CPU-side checks of the Jacobian entry points of the C ABI: the symbols exist, and a NULL solver is refused before any device is
touched, with every output left as it was."""
import ctypes as C

import numpy as np
import pytest

from realsensecalibration_amd import capi

NAMES = ("rsba_solver_jacobian_structure", "rsba_solver_evaluate_jacobian")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def test_symbols_exist():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert hasattr(capi.Solver, "jacobian_structure") and hasattr(capi.Solver, "evaluate_jacobian")


def test_null_solver_is_an_argument_error():
    lib = capi.load()
    counts = [C.c_int64(-7), C.c_int64(-8), C.c_int64(-9)]
    row_ptr, cols, values = np.full(4, -5, np.int64), np.full(4, -6, np.int32), np.full(4, -1.5)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rsba_solver_jacobian_structure(None, C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2]), vp(row_ptr), vp(cols)) == capi.ERR_ARG
    assert lib.rsba_solver_jacobian_structure(None, None, None, None, None, None) == capi.ERR_ARG
    assert lib.rsba_solver_evaluate_jacobian(None, None, vp(values)) == capi.ERR_ARG
    assert lib.rsba_solver_evaluate_jacobian(None, None, None) == capi.ERR_ARG
    assert [c.value for c in counts] == [-7, -8, -9]
    assert np.all(row_ptr == -5) and np.all(cols == -6) and np.all(values == -1.5)
