"""CPU-side checks of the observation-weight entry points of the C ABI (ceres::ScaledLoss on the marker-chain models): exports and
header agree, the problem-level setter validates and round-trips, the point model refuses, and a NULL solver is refused before any
device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import marker_loss_ref as ref
from realsensecalibration_amd import capi, synthetic

NAMES = ("rsba_problem_set_observation_weights", "rsba_problem_observation_weights", "rsba_solver_set_observation_weights")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsba.h")


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
    assert "int rsba_problem_set_observation_weights(rsba_problem* p, const double* weights" in text
    assert "const double* rsba_problem_observation_weights(const rsba_problem* p);" in text
    assert "int rsba_solver_set_observation_weights(rsba_solver* s, const double* weights" in text


def test_problem_setter_validates_and_round_trips():
    lib = capi.load()
    pr = capi.Problem.marker_chain(ref.hongo())
    try:
        N = pr.num_observations
        assert pr.observation_weights is None and not lib.rsba_problem_observation_weights(pr.h)
        w = np.random.default_rng(1).choice([0.0, 0.25, 1.0, 4.0], N)
        pr.set_observation_weights(w)
        w[:] = -1.0   # the array was copied
        want = np.random.default_rng(1).choice([0.0, 0.25, 1.0, 4.0], N)
        np.testing.assert_array_equal(pr.observation_weights, want)
        for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
            b = want.copy()
            b[N // 2] = bad
            assert lib.rsba_problem_set_observation_weights(pr.h, b.ctypes.data_as(C.c_void_p)) == capi.ERR_ARG, bad
            np.testing.assert_array_equal(pr.observation_weights, want)   # the previous weights stay
        with pytest.raises(ValueError):
            pr.set_observation_weights(np.ones(N + 1))
        pr.set_observation_weights(np.ones(N))   # all ones is a set of weights like any other
        np.testing.assert_array_equal(pr.observation_weights, np.ones(N))
        pr.set_observation_weights(None)
        assert pr.observation_weights is None
        pr.set_observation_weights(None)   # clearing twice is fine
    finally:
        pr.close()
    assert lib.rsba_problem_set_observation_weights(None, None) == capi.ERR_ARG
    assert not lib.rsba_problem_observation_weights(None)


def test_point_model_is_unsupported():
    lib = capi.load()
    pr = capi.Problem.points(synthetic.make_problem(2, 10, 2, seed=1))
    try:
        w = np.ones(pr.num_observations)
        assert lib.rsba_problem_set_observation_weights(pr.h, w.ctypes.data_as(C.c_void_p)) == capi.ERR_UNSUPPORTED
        assert lib.rsba_problem_set_observation_weights(pr.h, None) == capi.ERR_UNSUPPORTED
        assert pr.observation_weights is None
    finally:
        pr.close()


def test_null_solver_is_an_argument_error():
    w = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    assert capi.load().rsba_solver_set_observation_weights(None, w) == capi.ERR_ARG
    assert capi.load().rsba_solver_set_observation_weights(None, None) == capi.ERR_ARG
