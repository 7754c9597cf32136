"""CPU-side checks of the constant-components entry points of the C ABI (ceres::SubsetParameterization on a pose block of the
marker-chain models): exports, EXPORTS and the header agree, the setter validates and round-trips, a mask of 0 clears, the point model
refuses, the whole-block call is as it was and both settings coexist, and the Python binding takes a mask or an index list."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import marker_loss_ref as ref
from realsensecalibration_amd import capi, synthetic

NAMES = ("rsba_problem_set_parameter_subset_constant", "rsba_problem_parameter_subset_constant")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsba.h")
MIRROR = os.path.join(ROOT, "include", "rsba", "bundle_adjustment.h")


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
    assert "int rsba_problem_set_parameter_subset_constant(rsba_problem* p, int64_t parameter_offset, int32_t constant_mask);" in text
    assert "int32_t rsba_problem_parameter_subset_constant(const rsba_problem* p, int64_t parameter_offset);" in text
    assert "THIS DEPARTS FROM CERES, whose CRS matrix has the block's local size" in text   # the Jacobian's zero columns are stated
    for name in ("set_parameter_subset_constant", "parameter_subset_constant"):
        assert hasattr(capi.Problem, name), name
    assert "bool SetSubsetConstant(double* block, const std::vector<int>& constant_parameters)" in open(MIRROR).read()


def test_setter_validates_and_round_trips():
    lib = capi.load()
    pr = capi.Problem.marker_chain(ref.hongo())
    try:
        nb = pr.num_parameters // 6
        assert nb == 21
        assert all(lib.rsba_problem_parameter_subset_constant(pr.h, 6 * b) == 0 for b in range(nb))
        masks = {1: 0b000111, 7: 0b100100, nb - 1: 0b011111, 0: 0b000001}
        for b, m in masks.items():
            assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6 * b, m) == capi.OK
        for b in range(nb):
            assert lib.rsba_problem_parameter_subset_constant(pr.h, 6 * b) == masks.get(b, 0), b
        # argument errors change nothing
        for off, m in ((6 * 1 + 1, 1), (6 * 1 + 5, 1), (-6, 1), (6 * nb, 1), (6 * nb + 6, 1), (6, 63), (6, 64), (6, 127), (6, 1 << 8), (6, -1), (6, -64),
                       (6, 1 << 31 - 1)):
            assert lib.rsba_problem_set_parameter_subset_constant(pr.h, off, m) == capi.ERR_ARG, (off, m)
        for b in range(nb):
            assert lib.rsba_problem_parameter_subset_constant(pr.h, 6 * b) == masks.get(b, 0), b
        assert lib.rsba_problem_parameter_subset_constant(pr.h, 7) == 0 and lib.rsba_problem_parameter_subset_constant(pr.h, -6) == 0
        assert lib.rsba_problem_parameter_subset_constant(pr.h, 6 * nb) == 0
        # every mask of one to five bits is legal; a mask of 0 clears
        for m in range(63):
            assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6 * 2, m) == capi.OK
            assert lib.rsba_problem_parameter_subset_constant(pr.h, 6 * 2) == m
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6 * 2, 0) == capi.OK
        assert lib.rsba_problem_parameter_subset_constant(pr.h, 6 * 2) == 0
        # the parameters are not touched by any of this
        np.testing.assert_array_equal(pr.params, ref.hongo()["params"])
    finally:
        pr.close()
    assert lib.rsba_problem_set_parameter_subset_constant(None, 6, 1) == capi.ERR_ARG
    assert lib.rsba_problem_parameter_subset_constant(None, 6) == 0


def test_point_model_is_unsupported():
    lib = capi.load()
    pr = capi.Problem.points(synthetic.make_problem(2, 10, 2, seed=1))
    try:
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6, 0b000111) == capi.ERR_UNSUPPORTED
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6, 0) == capi.ERR_UNSUPPORTED
        assert lib.rsba_problem_parameter_subset_constant(pr.h, 6) == 0
        with pytest.raises(capi.RsbaError) as e:
            pr.set_parameter_subset_constant(6, [0, 1, 2])
        assert e.value.code == capi.ERR_UNSUPPORTED
        pr.set_parameter_block_constant(6)   # the whole-block call is the point model's as before
    finally:
        pr.close()


def test_block_constant_is_as_it_was_and_both_coexist():
    lib = capi.load()
    pr = capi.Problem.marker_chain(ref.hongo())
    try:
        nb = pr.num_parameters // 6
        assert lib.rsba_problem_set_parameter_block_constant(pr.h, 6 * 3, 1) == capi.OK
        assert lib.rsba_problem_set_parameter_block_constant(pr.h, 6 * 3 + 1, 1) == capi.ERR_ARG
        assert lib.rsba_problem_set_parameter_block_constant(pr.h, 6 * nb, 1) == capi.ERR_ARG
        assert lib.rsba_problem_set_parameter_block_constant(pr.h, -6, 1) == capi.ERR_ARG
        assert lib.rsba_problem_set_parameter_block_constant(None, 6, 1) == capi.ERR_ARG
        # a mask on a block that is constant as a whole, and the other way round: each setting keeps its own state
        pr.set_parameter_subset_constant(6 * 3, 0b010101)
        pr.set_parameter_subset_constant(6 * 4, 0b000011)
        pr.set_parameter_block_constant(6 * 4)
        assert pr.parameter_subset_constant(6 * 3) == 0b010101 and pr.parameter_subset_constant(6 * 4) == 0b000011
        pr.set_parameter_block_constant(6 * 3, False)
        pr.set_parameter_block_constant(6 * 4, False)
        assert pr.parameter_subset_constant(6 * 3) == 0b010101 and pr.parameter_subset_constant(6 * 4) == 0b000011
    finally:
        pr.close()


def test_python_binding_takes_a_mask_or_indices():
    pr = capi.Problem.marker_chain(ref.hongo())
    try:
        pr.set_parameter_subset_constant(6, 0b100011)
        assert pr.parameter_subset_constant(6) == 0b100011
        pr.set_parameter_subset_constant(12, [0, 1, 5])
        assert pr.parameter_subset_constant(12) == 0b100011
        pr.set_parameter_subset_constant(18, (q for q in (3, 3, 4)))   # any iterable; a repeated index is the same bit
        assert pr.parameter_subset_constant(18) == 0b011000
        pr.set_parameter_subset_constant(18, np.array([2], np.int64))
        assert pr.parameter_subset_constant(18) == 0b000100
        pr.set_parameter_subset_constant(18, np.int32(5))               # a numpy integer is a mask
        assert pr.parameter_subset_constant(18) == 5
        pr.set_parameter_subset_constant(18, [])
        assert pr.parameter_subset_constant(18) == 0
        pr.set_parameter_subset_constant(12, 0)
        assert pr.parameter_subset_constant(12) == 0
        for bad in ([6], [-1], [0, 7]):
            with pytest.raises(ValueError):
                pr.set_parameter_subset_constant(6, bad)
        for bad in (63, range(6), 64, -1):
            with pytest.raises(capi.RsbaError) as e:
                pr.set_parameter_subset_constant(6, bad)
            assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.RsbaError):
            pr.set_parameter_subset_constant(7, 1)
        assert pr.parameter_subset_constant(6) == 0b100011
    finally:
        pr.close()
