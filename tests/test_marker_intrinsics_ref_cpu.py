"""The numpy reference of free intrinsics (tests/marker_intrinsics_ref.py) held to itself, without a device: its rows against central
finite differences of its own residuals, the zero-noise statements of the cases (free intrinsics reach the truth, fixed ones cannot),
a held component keeps its bits, and the first step of the one-step cases is an accepted one."""
import numpy as np
import pytest

import marker_intrinsics_ref as iref


def _away(mc, seed=3):
    """A point away from the start: poses moved by 1e-2, focal lengths and principal points by a pixel, k1 k2 by 1e-2."""
    rng = np.random.default_rng(seed)
    x = mc.x0()
    x[:mc.n_pose] += 1e-2 * rng.standard_normal(mc.n_pose)
    six = x[mc.n_pose:].reshape(-1, 6)
    six[:, :4] += rng.standard_normal((six.shape[0], 4))
    six[:, 4:] += 1e-2 * rng.standard_normal((six.shape[0], 2))
    return x


@pytest.mark.parametrize("name", ["3x12x4_3f", "test2wiring_3x12x4_3f", "3x70x5_mixed_all"])
def test_rows_agree_with_finite_differences(name):
    """d r / d x_j by central differences of residuals_at() against the complex-step rows, column by column of the vector; the
    columns of held components are exact zeros.  Central differences with h = 1e-6 |x_j| + 1e-7: truncation h^2 r''' / 6 and
    rounding u |r| / h, both below 1e-6 of the column's largest entry for residuals of a few hundred pixels at most."""
    cs = iref.case(name)
    mc = iref.chain_of(cs)
    x = _away(mc)
    _, J = mc.rows(x)
    worst = 0.0
    for j in np.random.default_rng(1).choice(mc.n, 60, replace=False).tolist() + list(range(mc.n_pose, mc.n)):
        hit = mc.obs_cols == j                         # (N, 24): the residual blocks and local columns that are vector component j
        col = np.einsum("krq,kq->kr", J, hit.astype(float))
        if mc.held[j]:
            assert not col.any(), j
            continue
        h = 1e-6 * abs(x[j]) + 1e-7
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd = (mc.residuals_at(mc.full(xp), mc.six(xp)) - mc.residuals_at(mc.full(xm), mc.six(xm))) / (xp[j] - xm[j])
        assert not fd[~hit.any(axis=1)].any(), j      # nothing else depends on it
        scale = max(np.abs(col).max(), 1e-300)
        worst = max(worst, np.abs(fd - col).max() / scale)
    print("%s: rows against central differences, worst %.2e of a column's largest entry" % (name, worst))
    assert worst < 1e-6


def test_held_components_have_unit_diagonal_and_zero_gradient():
    cs = iref.case("3x70x5_mixed_all")
    mc = iref.chain_of(cs)
    _, _, _, H, g, _ = mc.linearise(_away(mc))
    at = np.flatnonzero(mc.held)
    assert at.size == 2 + 2 + 2    # two components of camera 2's pose, k1 k2 of camera 0, cx cy of camera 2
    off = H[at].copy()
    off[np.arange(at.size), at] = 0.0
    assert not off.any() and not H[:, at][~mc.held].any() and (H[at, at] == 1.0).all() and not g[at].any()


def test_zero_noise_free_intrinsics_reach_the_truth_and_fixed_ones_cannot():
    for name, k_bar in (("3x12x4_0f", None), ("3x12x4_3f", 1e-6)):
        cs, mc, x, summary, rows = iref.reference_run(name, noise=0.0)
        err = np.abs(mc.six(x) - cs["truth_six"])
        print("%s, zero noise: %d iterations, cost %.2e, intrinsics %.2e px off, k1 k2 %.2e off" % (name, len(rows) - 1, summary["final_cost"], err[:, :4].max(), err[:, 4:].max()))
        assert err[:, :4].max() < 1e-4 and summary["final_cost"] < 1e-9
        if k_bar is not None:
            assert err[:, 4:].max() < k_bar
        _, _, _, fixed, _ = iref.reference_run(name, noise=0.0, fixed=True)
        assert fixed["final_cost"] > 1.0, fixed["final_cost"]


def test_noisy_cases_end_below_fixed_intrinsics():
    costs = {n: iref.reference_run(n)[3]["final_cost"] for n in ("3x12x4_03", "3x12x4_0f", "3x12x4_3f")}
    fixed = iref.reference_run("3x12x4_3f", fixed=True)[3]["final_cost"]
    print("3 x 12 x 4, 0.3 px: fx fy %.2f, + cx cy %.2f, + k1 k2 %.2f, fixed %.2f" % (costs["3x12x4_03"], costs["3x12x4_0f"], costs["3x12x4_3f"], fixed))
    assert costs["3x12x4_3f"] < costs["3x12x4_0f"] < costs["3x12x4_03"] < fixed


def test_mask_03_keeps_the_bits_of_the_held_components():
    cs, mc, x, _, rows = iref.reference_run("3x12x4_03")
    start, end = mc.six(mc.x0()), mc.six(x)
    assert start[:, 2:].tobytes() == end[:, 2:].tobytes()
    assert (start[:, :2] != end[:, :2]).all() and len(rows) > 2


@pytest.mark.parametrize("name", ["3x12x4_3f", "3x70x5_mixed"])
def test_first_step_of_the_one_step_cases_is_accepted(name):
    _, _, _, _, rows = iref.reference_run(name)
    assert rows[1]["valid"] == 1 and rows[1]["successful"] == 1


def test_branch_above_384_columns_and_camera_without_a_block():
    cs, mc, _, _, rows = iref.reference_run("3x70x5_mixed")
    assert mc.n > 384 and list(mc.cams) == [0, 2] and len(rows) > 3
    cs, mc, _, _, _ = iref.reference_run("3x70x5_mixed_all")
    assert mc.n > 384 and mc.held.sum() == 6 and len(mc.priors) == 1 and (mc.w == 0).any()


def test_compact_view_takes_the_same_step():
    """The zero-column / unit-diagonal formulation and the one with the held components removed take the same step."""
    cs = iref.case("3x70x5_mixed")
    mc = iref.chain_of(cs)
    cv = mc.compact_view()
    _, _, _, H, g, _ = mc.linearise(mc.x0())
    _, _, _, Hk, gk, _ = cv.linearise(cv.x0())

    def step(H, g):
        s = 1.0 / (1.0 + np.sqrt(np.diag(H)))
        A = H * np.outer(s, s)
        A += np.diag(np.clip(np.diag(A), 1e-6, 1e32) / 1e4)
        return -s * np.linalg.solve(A, s * g)
    d, dk = step(H, g), step(Hk, gk)
    assert not d[mc.held].any()
    assert np.abs(d[~mc.held] - dk).max() <= 1e-9 * np.abs(dk).max()
