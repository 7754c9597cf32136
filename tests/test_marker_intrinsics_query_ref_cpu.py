"""Pins tests/marker_intrinsics_query_ref.py without a device: the mapping between the extended layout and the reference's own vector,
the gradient against central differences of `cost`, the literal zeros, and the two ways the covariance is taken."""
import numpy as np
import pytest

import marker_intrinsics_query_ref as qref
import marker_intrinsics_ref as iref

CASES = ["3x12x4_3f", "3x70x5_mixed_all"]


@pytest.mark.parametrize("name", CASES)
def test_mapping_round_trips_and_names_every_slot_once(name):
    cs = iref.case(name)
    xe = qref.perturbed(cs)
    q = qref.Queries(cs, xe)
    C, T, M = q.C, q.T, q.M
    assert q.npar == 6 * (C + T + M) == cs["prob"]["params"].size and q.next == q.npar + 6 * C
    assert np.unique(q.ext_of).size == q.mc.n and q.ext_of.max() < q.next
    assert np.array_equal(q.to_chain(xe), q.mc.x0())                       # the chain was built from xe
    assert np.array_equal(q.to_extended(q.to_chain(xe), np.nan)[q.ext_of], xe[q.ext_of])
    # intrinsics blocks: camera k at npar + 6 k, only cameras with a mask
    for k, m in enumerate(cs["masks"]):
        assert (q.position(q.npar + 6 * k) >= q.mc.n_pose) == bool(m)
        if m:
            assert q.held6(q.npar + 6 * k).tolist() == [not (m >> c) & 1 for c in range(6)]
    # the values the formulas read are xe's, for a camera without a block too
    assert np.array_equal(q.mc.six(q.x).ravel(), xe[q.npar:])
    assert np.array_equal(q.mc.full(q.x).ravel(), xe[:q.npar])


@pytest.mark.parametrize("name", CASES)
def test_gradient_agrees_with_central_differences_of_the_cost(name):
    """h = 1e-6 |x_j| + 1e-7.  The bar per entry: the cost's rounding through the difference, 4 u cost / h, and 1e-8 of the largest
    gradient entry for the truncation (h^2 c''' / 6) and Huber's second-derivative jumps (O(h) each)."""
    cs = iref.case(name)
    q = qref.Queries(cs, qref.perturbed(cs))
    g = q.gradient()
    comp = q.computed()
    assert not g[~comp].any() and np.all(np.signbit(g[~comp]) == 0)        # the slots that are zeros by definition
    mc, x = q.mc, q.x
    cost = q.cost()
    assert abs(mc.cost(x)[0] - cost) <= 1e-12 * cost
    gmax = np.abs(g).max()
    rng = np.random.default_rng(3)
    free = np.flatnonzero(~mc.held)
    pick = np.unique(np.concatenate([free[free >= mc.n_pose], rng.choice(free[free < mc.n_pose], 40, replace=False)]))
    worst = 0.0
    for j in pick:
        h = 1e-6 * abs(x[j]) + 1e-7
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd = (mc.cost(xp)[0] - mc.cost(xm)[0]) / (xp[j] - xm[j])
        bar = 4.0 * qref.U * cost / h + 1e-8 * gmax
        worst = max(worst, abs(fd - g[q.ext_of[j]]) / bar)
    print("%s: %d entries, worst error / bar %.2e" % (name, pick.size, worst))
    assert worst <= 1.0


def test_residual_vector_order_and_cost():
    cs = iref.case("3x70x5_mixed_all")
    q = qref.Queries(cs, qref.extended_x0(cs))
    r = q.residuals()
    assert r.size == 8 * q.N + 6 * len(cs["priors"])
    assert not r[8 * q.N:].any()                                           # the prior sits on its block's start value
    # cost = 1/2 sum w rho(s): with Huber and weights not 1/2 |r|^2, but the weight-0 blocks' residuals are zeros
    w = cs["weights"]
    assert not r[:8 * q.N].reshape(-1, 8)[w == 0].any() and r[:8 * q.N].reshape(-1, 8)[w > 0].any()
    assert q.raw_rounding() < 1e-9 and q.rbar() >= 16 * 4 * np.spacing(np.abs(q.mc.obs).max())


@pytest.mark.parametrize("name", CASES)
def test_covariance_two_ways_agree_and_held_rows_are_zero(name):
    cs = iref.case(name)
    q = qref.Queries(cs, qref.extended_x0(cs))
    a, b = q.covariance("inv"), q.covariance("chol")
    held = q.mc.held
    assert not a[held].any() and not a[:, held].any()
    worst = 0.0
    for i in range(0, q.mc.n, 6):
        for j in range(0, q.mc.n, 6):
            ba, bb = a[i:i + 6, j:j + 6], b[i:i + 6, j:j + 6]
            if np.abs(ba).max() > 0:
                worst = max(worst, np.abs(ba - bb).max() / np.abs(ba).max())
    print("%s: inv against Cholesky, worst block difference %.2e of the block's largest entry" % (name, worst))
    assert worst <= 1e-9
    # a camera without a block: no position, zeros
    for k, m in enumerate(cs["masks"]):
        if not m:
            assert q.position(q.npar + 6 * k) == -1 and not q.block(a, q.npar + 6 * k, 6).any()
