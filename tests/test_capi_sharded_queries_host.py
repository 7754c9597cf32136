"""CPU-side checks of evaluate / set-parameters / covariance on a solver with a communicator: the header states the collective
contract and no longer promises RSBA_ERR_UNSUPPORTED for several ranks, the one export the loopback helper needed is declared,
exported and bound, and the helper itself is there."""
import os
import re

import pytest

from realsensecalibration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def _header():
    return open(os.path.join(ROOT, "include", "rsba.h")).read()


def test_the_helpers_export_is_declared_exported_and_bound():
    declared = set(re.findall(r"\b(rsba_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(capi.EXPORTS), declared ^ set(capi.EXPORTS)
    assert "rsba_solver_comm_abort" in declared
    lib = capi.load()
    assert hasattr(lib, "rsba_solver_comm_abort")
    assert lib.rsba_solver_comm_abort(None) == capi.ERR_ARG   # refused before any device is touched
    assert callable(capi.ShardedLoopbackGroup) and callable(capi.solve_points_sharded_loopback)


def _comment_before(hdr, declaration):
    """The comment block that ends right before `declaration` (back to the previous section rule or declaration)."""
    end = hdr.index(declaration)
    start = max(hdr.rfind("/* ----", 0, end), hdr.rfind(";\n", 0, hdr.rfind("/*", 0, end)))
    return hdr[start:end]


@pytest.mark.parametrize("declaration", ["typedef struct rsba_covariance_options", "typedef struct rsba_evaluate_options",
                                         "int rsba_solver_set_parameters("])
def test_header_no_longer_refuses_several_ranks(declaration):
    text = " ".join(_comment_before(_header(), declaration).split())
    assert "world_size > 1" not in text or "RSBA_ERR_UNSUPPORTED on every rank" not in text, text
    assert not re.search(r"world_size > 1\s*(returns|:)\s*RSBA_ERR_UNSUPPORTED", text), text
    assert "communicator" in text and "COLLECTIVE" in text, text


def test_header_states_the_collective_contract():
    text = " ".join(_header().split())
    for phrase in ("THE COLLECTIVE CONTRACT", "request word", "all ranks then return RSBA_ERR_ARG", "RSBA_ERR_COMM",
                   "residuals alone is local", "rsba_solver_covariance_block and rsba_solver_point_covariances are local"):
        assert phrase in text, phrase
