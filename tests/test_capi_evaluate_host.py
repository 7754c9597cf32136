"""CPU-side checks of the evaluate / set-parameters entry points of the C ABI: the symbols exist, the options default to Ceres'
EvaluateOptions, and a NULL solver is refused before any device is touched."""
import ctypes as C

import pytest

from realsensecalibration_amd import capi

NAMES = ("rsba_evaluate_options_default", "rsba_solver_num_residuals", "rsba_solver_evaluate", "rsba_solver_set_parameters")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def test_symbols_exist():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name), name


def test_options_default_to_apply_loss_function():
    o = capi.EvaluateOptions(apply_loss_function=7, reserved=7)
    capi.load().rsba_evaluate_options_default(C.byref(o))
    assert (o.apply_loss_function, o.reserved) == (1, 0)
    capi.load().rsba_evaluate_options_default(None)   # NULL is ignored


def test_null_solver_is_an_argument_error():
    lib = capi.load()
    cost = C.c_double(123.0)
    x = (C.c_double * 6)()
    assert lib.rsba_solver_evaluate(None, None, C.byref(cost), None, None) == capi.ERR_ARG
    assert cost.value == 123.0
    assert lib.rsba_solver_evaluate(None, None, None, None, None) == capi.ERR_ARG
    assert lib.rsba_solver_set_parameters(None, x) == capi.ERR_ARG
    # a count cannot be an error code: the NULL solver's answer is the NEGATIVE code, which no count is
    assert lib.rsba_solver_num_residuals(None) == -capi.ERR_ARG
