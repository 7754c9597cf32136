"""tests/marker_prior_ref.py (Gaussian priors on camera and marker blocks, ceres::NormalPrior) pinned without a device.

  - its gradient and H are those of the stacked residual vector [reprojection; A (x - b)], taken by complex-step columns;
  - THE ACTING CONDITION: every case's priors move its solution by at least 1e-3 in some component against the prior-free solve —
    the device tests compare against solutions the priors really shaped;
  - a prior on a block that is constant as a whole changes the cost only;
  - a zero A reproduces the prior-free reference's iterates exactly.
"""
import numpy as np
import pytest

import marker_prior_ref as pref

CASES = ["P1", "P2", "P3", "P4", "X12", "P1w", "D1"]


def _stacked_jacobian(mc, x):
    """J of stacked_residuals over the kept columns by complex steps, and the residuals."""
    comp = np.tile(np.arange(6), mc.free_blocks.size)[mc.keep]
    full = mc.full(x)
    r = mc.stacked_residuals(full)
    J = np.zeros((r.size, mc.n))
    for j in range(mc.n):
        f = full.astype(complex)
        f[mc.col_block[j], comp[j]] += 1e-30j
        J[:, j] = mc.stacked_residuals(f).imag / 1e-30
    return J, r


@pytest.mark.parametrize("pid", ["P1", "P3", "P4"])
def test_gradient_and_hessian_are_those_of_the_stacked_residuals(pid):
    cs = dict(pref.case(pid), loss="none", a=0.0)   # (raw rows: the corrector is marker_loss_ref's own business)
    mc = pref.chain_of(cs)
    x = mc.x0() + 1e-3 * np.random.default_rng(3).standard_normal(mc.n)   # off the priors' centres: their residuals are not zero
    cost, _, _, H, g, sumsq = mc.linearise(x)
    J, r = _stacked_jacobian(mc, x)
    assert r.size == 8 * mc.N + 6 * len(mc.priors)
    np.testing.assert_allclose(cost, 0.5 * r @ r, rtol=1e-13)
    np.testing.assert_allclose(sumsq, r[:8 * mc.N] @ r[:8 * mc.N], rtol=1e-13)   # the raw metric never sees a prior
    np.testing.assert_allclose(g, J.T @ r, rtol=1e-9, atol=1e-9 * np.abs(g).max())
    np.testing.assert_allclose(H, J.T @ J, rtol=1e-9, atol=1e-9 * np.abs(H).max())
    assert mc.prior_cost(x) > 0.0
    # the model cost change is that of the stacked rows
    delta = 1e-4 * np.random.default_rng(4).standard_normal(mc.n)
    _, rt, Jt, _, _, _ = mc.linearise(x)
    Jd = J @ delta
    np.testing.assert_allclose(mc.model_cost_change(rt, Jt, delta), -float(Jd @ (r + 0.5 * Jd)), rtol=1e-9)


@pytest.mark.parametrize("pid", CASES)
def test_the_priors_act(pid):
    _, mc, summary, rows, with_p = pref.reference_run(pid)
    _, _, summary0, rows0, without = pref.reference_run(pid, with_priors=False)
    moved = float(np.abs(with_p - without).max())
    print("%s: %d iterations with priors (%s), %d without; the solution moves %.3e" % (pid, len(rows) - 1, summary["reason"], len(rows0) - 1, moved))
    assert len(rows) > 3
    assert moved >= 1e-3, moved


def test_a_prior_on_a_constant_block_changes_the_cost_only():
    cs = pref.case("P3")
    consts = [b for b in cs["priors"] if b in cs["constant_blocks"]]
    assert len(consts) == 2                                     # camera 2 and marker 3
    only = {b: (cs["priors"][b][0], cs["priors"][b][1] + 0.01) for b in consts}   # off centre, or the prior's residual is zero
    mc1, mc0 = pref.chain_of(cs, only), pref.chain_of(cs, {})
    assert mc1.n == mc0.n
    x = mc0.x0()
    c1, _, _, H1, g1, s1 = mc1.linearise(x)
    c0, _, _, H0, g0, s0 = mc0.linearise(x)
    np.testing.assert_array_equal(H1, H0)
    np.testing.assert_array_equal(g1, g0)
    assert s1 == s0
    want = 0.5 * sum(float(np.sum((A @ np.full(6, -0.01)) ** 2)) for A, _ in only.values())
    assert want > 0.0 and abs((c1 - c0) - want) <= 1e-12 * want
    assert all(at.size == 0 for _, _, at, _ in mc1.prior_rows(x))


def test_a_zero_matrix_reproduces_the_prior_free_iterates():
    cs = pref.case("P1")
    zero = {b: (np.zeros((6, 6)), v) for b, (_, v) in cs["priors"].items()}
    x1, s1, rows1 = pref.minimise(pref.chain_of(cs, zero))
    x0, s0, rows0 = pref.minimise(pref.chain_of(cs, {}))
    assert rows1 == rows0 and s1 == s0
    np.testing.assert_array_equal(x1, x0)
