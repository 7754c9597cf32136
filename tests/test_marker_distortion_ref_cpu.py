"""The numpy reference of the marker chain with lens distortion (tests/marker_distortion_ref.py), held on the CPU:

  * zero coefficients reproduce marker_loss_ref.MarkerChain's residuals bit for bit;
  * the complex-step Jacobian (the parent's jacobians(), run on the distorted residuals) agrees with central differences taken in
    np.longdouble;
  * on the zero-noise redetected 4 x 40 x 6 the distorted model's minimum is the truth and the pinhole model's is not;
  * every whole-solve case the GPU test compares against has a robust trajectory: repeated with its normal equations summed in
    np.longdouble the accept / reject sequence is identical and the final parameters agree to 1e-8.
"""
import numpy as np
import pytest

import marker_distortion_ref as dref
import marker_loss_ref as ref
import marker_step_accuracy as msa
import solve_accuracy as sa
from realsensecalibration_amd import synthetic as syn


def test_zero_coefficients_reproduce_the_pinhole_bits():
    for prob, variant in ((syn.make_marker_chain(4, 12, 6, seed=3), 0), (ref.hongo(), 0), (ref.test2(), 1)):
        a = ref.MarkerChain(prob, variant)
        b = dref.MarkerChainDist(prob, np.zeros((prob["C"], 5)), variant)
        full = a.full(a.x0())
        ra, rb = a.residuals(full), b.residuals(full)
        assert ra.tobytes() == rb.tobytes()
        assert np.array_equal(a.jacobians(full), b.jacobians(full))


def test_coefficients_are_in_range_and_structured():
    for C, seed in ((4, 1), (8, 5), (3, 2), (2, 9)):
        d = dref.coefficients(C, seed)
        assert d.shape == (C, 5) and not d[0].any()
        assert -0.30 <= d[:, 0].min() and d[:, 0].max() <= 0.15 and np.abs(d[:, 1]).max() <= 0.10
        assert np.abs(d[:, 2:4]).max() <= 2e-3 and np.abs(d[:, 4]).max() <= 0.05
        assert not d[1, [0, 1, 4]].any() and d[1, 2:4].all()
        if C > 2:
            assert not d[2, :4].any() and d[2, 4] != 0.0
    assert np.array_equal(dref.coefficients(4, 1), dref.coefficients(4, 1))


def test_complex_step_jacobian_against_longdouble_central_differences():
    """h = 1e-6 in np.longdouble (u = 5e-20): truncation h^2 f''' / 6 ~ 1e-12 f''' and rounding u / h ~ 1e-13 of the residuals' size
    (pixels, <= 1e3); third derivatives of a pixel coordinate with respect to a pose parameter stay below 1e4 times the first here
    (depths above 0.3 m, angles O(1)), so the difference quotient is good to 1e-8 of a row's largest entry.  The bar is 1e-7 of it."""
    assert sa.longdouble_ok()
    prob = syn.make_marker_chain(4, 10, 6, seed=11)
    dist = dref.coefficients(4, 3)
    mc = dref.MarkerChainDist(dref.redetect(prob, dist, 0.3, 3), dist)
    full = mc.full(mc.x0())
    J = mc.jacobians(full)
    C, T, M = mc.C, mc.T, mc.M
    ranges = [(0, C), (C, C + T), (C + T, C + T + M)]
    h = np.longdouble(1e-6)
    worst = 0.0
    for q in range(18):
        lo, hi = ranges[q // 6]
        fp, fm = full.astype(np.longdouble), full.astype(np.longdouble)
        fp[lo:hi, q % 6] += h
        fm[lo:hi, q % 6] -= h
        cd = ((mc.residuals(fp) - mc.residuals(fm)) / (2 * h)).astype(float)
        cd[mc.cols[:, q] < 0] = 0.0
        scale = np.abs(J).max(axis=2)
        worst = max(worst, float((np.abs(cd - J[:, :, q]) / scale).max()))
    print("complex step against central differences: %.2e of the row's largest entry (bar 1e-7)" % worst)
    assert worst < 1e-7
    assert np.abs(J - ref.MarkerChain(mc_prob(mc), 0).jacobians(full)).max() > 1e-3   # and distortion is in it


def mc_prob(mc):
    return dict(C=mc.C, T=mc.T, M=mc.M, N=mc.N, c=mc.c, t=mc.t, m=mc.m, obs=mc.obs, intr=mc.intr, marker_side=2 * mc.h, params=mc.full0.ravel())


def test_distorted_model_reaches_the_truth_and_the_pinhole_model_does_not():
    """Zero-noise redetected 4 x 40 x 6 (rig seed 50, coefficients(4, 1)).  Recorded on the reference: the distorted model ends at an
    RMS of 1.8e-09 px with every block within 2.5e-10 of the truth (the wiring fixes the gauge — camera 0 and marker 0 are not in the
    chain, and the marker side fixes the scale.  A deviation from the issue, which asks for tests/gauge.py's alignment: that module
    aligns the point model's cameras and points under a similarity; this wiring (variant 0) has no gauge orbit to align along, so raw
    parameters are compared); the pinhole model on the same detections ends at
    RMS 5.013298e-02 px, 5.4e-03 off the truth."""
    prob, dist, truth = dref.zero_noise_problem()
    mc = dref.MarkerChainDist(prob, dist)
    x, summary, rows = ref.minimise(mc)
    err = np.abs(mc.full(x) - truth).max()
    rms = dref.rms(mc, x)
    pin = ref.MarkerChain(prob, 0)
    xp, _, _ = ref.minimise(pin)
    err_p = np.abs(pin.full(xp) - truth).max()
    rms_p = dref.rms(pin, xp)
    print("distorted: rms %.3e px, %.3e off the truth; pinhole: rms %.6e px, %.3e off the truth" % (rms, err, rms_p, err_p))
    assert summary["termination"] == "CONVERGENCE"
    assert err < 1e-6 and rms < 1e-6
    assert abs(rms_p - PINHOLE_RMS) <= 1e-7, rms_p
    assert err_p > 1e-3 and rms_p > 1e-2


PINHOLE_RMS = 5.013298e-02   # px; the figure test_gpu_marker_distortion.py holds the device's pinhole solve to (1e-4 px)


class _LongdoubleSums:
    """linearise() with H and g summed in np.longdouble (marker_step_accuracy's sums), rounded once to double."""

    def linearise(self, x):
        cost, rt, Jt, _, _, sumsq = super().linearise(x)
        H, g = msa._longdouble_normal_equations(self, rt, Jt)
        return cost, rt, Jt, np.asarray(H, np.float64), np.asarray(g, np.float64), sumsq


@pytest.mark.parametrize("name", dref.SOLVE_CASES)
def test_solve_cases_have_a_robust_trajectory(name):
    assert sa.longdouble_ok()
    cs, mc, summary, rows, final = dref.reference_run(name)
    base = type(mc)
    mc2 = dref.chain_of(cs)
    mc2.__class__ = type("Longdouble" + base.__name__, (_LongdoubleSums, base), {})
    x2, summary2, rows2 = ref.minimise(mc2)
    assert summary["termination"] == "CONVERGENCE" and len(rows) > 3
    assert [(r["valid"], r["successful"]) for r in rows] == [(r["valid"], r["successful"]) for r in rows2]
    assert (summary2["termination"], summary2["reason"]) == (summary["termination"], summary["reason"])
    diff = float(np.abs(mc2.full(x2) - final).max())
    print("%s: %d iterations (%s), final parameters %.2e apart between double and longdouble sums" % (name, len(rows) - 1, summary["reason"], diff))
    assert diff <= 1e-8
    if cs["loss"] != "none":
        r = mc.residuals(final)
        past = int(np.sum(np.sum(r * r, axis=1) > cs["a"] ** 2))
        assert 0 < past < mc.N   # both branches of the loss at the solution
