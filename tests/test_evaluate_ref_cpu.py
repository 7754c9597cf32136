"""The reference of tests/evaluate_ref.py checked against central differences of the oracle's cost functions (no GPU).

    D_k(h) = (f(x + h e_k) - f(x - h e_k)) / (2 h),      h = 1e-6 (parameters are radians and metres of order 1)

differs from the true derivative by at most

    rounding     eps f / h             the two costs are rounded values of size f, and their difference is divided by 2 h
    truncation   |D_k(2 h) - D_k(h)|   D(2h) - D(h) = (h^2 / 2) f''' + O(h^4) is three times the leading truncation term h^2 f''' / 6
                                       of D(h); the factor 3 is left in for the higher orders (and for Huber's kink in f'')

Both terms come from the oracle's cost alone; the gradient under test does not enter the bound."""
import numpy as np
import pytest

import evaluate_ref as er
import marker_loss_ref as mlr
from realsensecalibration_amd import synthetic as syn

EPS = np.finfo(float).eps
H = 1e-6


def _check_against_differences(cost_fn, x, gradient, live):
    f0 = cost_fn(x)
    worst = 0.0
    for k in range(len(x)):
        def diff(h):
            xp, xm = x.copy(), x.copy()
            xp[k] += h
            xm[k] -= h
            return (cost_fn(xp) - cost_fn(xm)) / (2.0 * h)
        d1, d2 = diff(H), diff(2.0 * H)
        bound = EPS * f0 / H + abs(d2 - d1)
        if not live[k]:
            # a masked slot: exactly zero in the reference, whatever the cost's own derivative is (constant blocks have one)
            assert gradient[k] == 0.0, k
            continue
        err = abs(gradient[k] - d1)
        worst = max(worst, err / bound)
        assert err <= bound, (k, gradient[k], d1, err, bound)
    print("largest error / bound: %.3f" % worst)


def _point_problem():
    """C = 5, P = 70: camera 4 and point 17 unreferenced, 10 % outliers (so Huber's outer branch is taken)."""
    prob = syn.make_problem(5, 70, 4, seed=31, outlier_frac=0.1)
    keep = (prob["cam_idx"] != 4) & (prob["pt_idx"] != 17)
    return dict(prob, cam_idx=np.ascontiguousarray(prob["cam_idx"][keep]), pt_idx=np.ascontiguousarray(prob["pt_idx"][keep]),
                obs=np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1)), N=int(keep.sum()))


@pytest.mark.parametrize("loss,a", [("none", 0.0), ("huber", 1.5)])
def test_point_gradient_agrees_with_central_differences(oracle, loss, a):
    prob = _point_problem()
    x = prob["params"].copy()
    const_cams, const_pts = (0,), (3, 69)
    ref = er.point_evaluate(oracle, prob, x, const_cams, const_pts, loss, a)
    assert abs(ref.cost - oracle.points_cost(prob, x, a)[0]) <= (prob["N"] + 8) * EPS * ref.cost
    C = prob["C"]
    for off, size in [(0, 6), (6 * 4, 6), (6 * C + 3 * 3, 3), (6 * C + 3 * 17, 3), (6 * C + 3 * 69, 3)]:
        assert not ref.live[off:off + size].any() and np.all(ref.gradient[off:off + size] == 0.0)
    assert ref.live.sum() == len(x) - 2 * 6 - 3 * 3
    if loss == "huber":
        assert (ref.s > a * a).any() and (ref.s <= a * a).any()
    # the differences see the constant blocks' derivatives too: compare those against the reference WITHOUT the constant flags
    free = er.point_evaluate(oracle, prob, x, (), (), loss, a)
    _check_against_differences(lambda v: oracle.points_cost(prob, v, a)[0], x, free.gradient, free.live)
    np.testing.assert_array_equal(ref.gradient[ref.live], free.gradient[ref.live])


def test_marker_chain_gradient_agrees_with_central_differences_on_hongo(oracle):
    prob = mlr.hongo()
    x = prob["params"].copy()
    ref = er.marker_evaluate(oracle, prob, x, 0)
    C, T = prob["C"], prob["T"]
    cost = lambda v: oracle.marker_chain_cost(prob, 0, prob["marker_side"], prob["intr"], v)   # noqa: E731
    assert abs(ref.cost - cost(x)) <= (prob["N"] + 8) * EPS * ref.cost
    for b in (0, C + T):   # the fixed base blocks: camera 0, marker 0
        assert not ref.live[6 * b:6 * b + 6].any() and np.all(ref.gradient[6 * b:6 * b + 6] == 0.0)
    _check_against_differences(cost, x, ref.gradient, ref.live)


def test_unapplied_loss_is_the_raw_problem(oracle):
    prob = _point_problem()
    x = prob["params"]
    raw = er.point_evaluate(oracle, prob, x)
    off = er.point_evaluate(oracle, prob, x, loss="cauchy", a=2.0, apply_loss=False)
    on = er.point_evaluate(oracle, prob, x, loss="cauchy", a=2.0)
    np.testing.assert_array_equal(raw.residuals, off.residuals)
    np.testing.assert_array_equal(raw.gradient, off.gradient)
    assert raw.cost == off.cost and on.cost < raw.cost
    assert abs(on.cost - oracle.points_cost(prob, x, -2.0)[0]) <= (prob["N"] + 8) * EPS * on.cost
    np.testing.assert_array_equal(on.raw, raw.residuals)
