"""tests/marker_sparse_ref.py (the time blocks eliminated) against tests/marker_loss_ref.py (the dense normal equations): the same
LM trajectory to 1e-12 on small rigs, with constant blocks of every kind and with and without a loss."""
import numpy as np
import pytest

import marker_loss_ref as ref
import marker_sparse_ref as sref
from realsensecalibration_amd import synthetic as syn


def _rig():
    return ref.displace_corners(syn.make_marker_chain(4, 12, 5, seed=61), 0.05, 30.0, 61)


def _consts(prob, kind):
    C, T, M = prob["C"], prob["T"], prob["M"]
    t0 = int(prob["t"][0])
    sel = np.asarray(prob["t"]) == t0
    return {
        "none": (),
        "one_each": (2, C + 4, C + T + 3),
        "markers": tuple(C + T + m for m in range(1, M)),
        "cameras": (1, 3),
        "times": tuple(sorted({C + t0, C + 2, C + 5} | {int(c) for c in np.asarray(prob["c"])[sel] if c != 0}
                              | {C + T + int(m) for m in np.asarray(prob["m"])[sel] if m != 0})),
        "rig": tuple(range(1, C)) + tuple(C + T + m for m in range(1, M)),
    }[kind]


@pytest.mark.parametrize("loss", ["none", "huber", "cauchy"])
@pytest.mark.parametrize("kind", ["none", "one_each", "markers", "cameras", "times", "rig"])
def test_eliminated_reference_matches_dense(kind, loss):
    prob = _rig()
    const = _consts(prob, kind)
    a = 2.0
    smc = sref.SparseMarkerChain(prob, 0, loss, a, const)
    mc = ref.MarkerChain(prob, 0, loss, a, const)
    xs, ss, rs = sref.minimise(smc, max_num_iterations=15)
    xd, sd, rd = ref.minimise(mc, max_num_iterations=15)
    assert (ss["termination"], ss["reason"], len(rs)) == (sd["termination"], sd["reason"], len(rd))
    assert len(rd) > 2
    g0 = rd[0]["gradient_max_norm"]   # (a gradient is a sum that cancels as the solve converges: to 1e-12 of the first one)
    for a_, b_ in zip(rs, rd):
        assert (a_["valid"], a_["successful"]) == (b_["valid"], b_["successful"])
        assert abs(a_["cost"] - b_["cost"]) <= 1e-12 * b_["cost"], (a_["cost"], b_["cost"])
        # (two factorisations of the same system: the steps agree to the solve's rounding, not to the last bits; the radius follows the
        #  ratio of two small cost changes near convergence)
        assert abs(a_["step_norm"] - b_["step_norm"]) <= 1e-9 * b_["step_norm"]
        assert abs(a_["trust_region_radius"] - b_["trust_region_radius"]) <= 1e-9 * b_["trust_region_radius"]
        assert abs(a_["gradient_max_norm"] - b_["gradient_max_norm"]) <= 1e-12 * g0
    assert np.abs(xs - xd).max() <= 1e-12 * max(1.0, np.abs(xd).max())
    if kind == "rig":
        assert smc.nr == 0


def test_test2_variant_with_constant_blocks():
    prob = ref.displace_corners(ref.test2(), 0.05, 25.0, 12)
    C, T = prob["C"], prob["T"]
    const = (1, C + 2, C + T + 3)
    smc = sref.SparseMarkerChain(prob, 1, "huber", 1.5, const)
    mc = ref.MarkerChain(prob, 1, "huber", 1.5, const)
    xs, ss, rs = sref.minimise(smc, max_num_iterations=10)
    xd, sd, rd = ref.minimise(mc, max_num_iterations=10)
    assert [(r["valid"], r["successful"]) for r in rs] == [(r["valid"], r["successful"]) for r in rd]
    assert all(abs(a["cost"] - b["cost"]) <= 1e-12 * b["cost"] for a, b in zip(rs, rd))
    assert np.abs(xs - xd).max() <= 1e-12 * max(1.0, np.abs(xd).max())
