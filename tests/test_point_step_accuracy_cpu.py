"""The point model's step measure (tests/point_step_accuracy.py) is neither vacuous nor false: without a GPU, on every case shape of
tests/test_gpu_point_step.py,

  * the reference's own fp64 step — a numpy Schur complement and Cholesky, the points back-substituted with explicit 3 x 3 inverses —
    passes through the same x1 = fl(x0 + delta) round trip and stays within the bar on every row, for the first step and for the
    second (the system at x1, iteration 0's scale, the radius Levenberg-Marquardt's rule gives after the first);
  * mutations of that step exceed the bar on v64: one observation left out of a 21-view point's W_j' dc sum, one entry of one point's
    (V_j + D_j)^-1 off by 1e-9 relative, one point given its neighbour's g_p; and, on the second step, one point's kept g_p left
    at iteration 0's, and the system damped with the first step's radius;
  * a second step damped with a scale taken at x1 instead of x0 is NOT above the bar, and cannot be: D / s^2 = diag(H) / radius
    wherever the clip to [min_lm_diagonal, max_lm_diagonal] is inactive (asserted: it is, on every row of v64), so the scale drops
    out of the full system, and the measure is invariant under a diagonal scaling of the unknowns.  What the fixed scale changes is
    the rounding of the solve, not the system solved; the figure is printed;
  * the complex-step rows equal the oracle's point_residual_jacobian rows on v64 to tests/test_gpu_jacobian.py's floor;
  * the view histograms, the camera coverage and the slices > 4 x grid condition of the trip shapes hold, and no row's bar exceeds 1e-9
    but the camera rows of the radius-1e12 case's two steps (no camera is fixed: the gauge directions of the reduced system are held
    by the damping alone there, kappa_s ~ sqrt(radius); its point rows are at 1e-13).

Every shape is checked at its full size (the trip shapes take about ten seconds each)."""
import numpy as np
import pytest

import oracle_lib
import point_step_accuracy as psa
import step_path_ref

BAR_EXCEPTIONS = {("v64_r1e12", 1, "cam"), ("v64_r1e12", 2, "cam")}   # (case, step, row class) whose bar may exceed psa.BAR_CAP: see the module docstring


def _next_radius(radius, rho):
    return min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))


_STEPS = {}


def _two_steps(case):
    """(model, system at x0, x1, system at x1, x2) of the reference's own steps, once per case."""
    if case.name not in _STEPS:
        mdl = psa.model(case)
        sys1 = psa.System(mdl, mdl.x0, case.radius)
        x1 = mdl.x0 + sys1.reference_step()
        mcc, _ = sys1.model_cost_change(x1)
        rho = (sys1.cost - mdl.cost(x1)) / mcc
        sys2 = psa.System(mdl, x1, _next_radius(case.radius, rho), scale=sys1.s)
        x2 = x1 + sys2.reference_step()
        _STEPS[case.name] = (mdl, sys1, x1, sys2, x2)
    return _STEPS[case.name]


@pytest.mark.parametrize("case", psa.CASES, ids=[c.name for c in psa.CASES])
def test_reference_steps_within_the_bar(case):
    mdl, sys1, x1, sys2, x2 = _two_steps(case)
    assert np.linalg.norm(mdl.x0[mdl.free]) > 1.0   # (parameter_tolerance = -1 ends a run only below |x| = 1)
    assert mdl.cam_obs[mdl.cam_free].min() >= 6
    for step, sysm, xn in ((1, sys1, x1), (2, sys2, x2)):
        r = sysm.check(xn)
        print("\n%-14s step %d radius %.3g n %6d m %5d kappa_s %8.3g kappa_p %8.3g | cam eta %.2e bar %.2e | pt eta %.2e bar %.2e | eta/bar %.3f" % (
            case.name, step, sysm.radius, mdl.n_free, mdl.m, sysm.kappa_s, sysm.kappa_pmax, r["cam"]["eta"], r["cam"]["bar"], r["pt"]["eta"],
            r["pt"]["bar"], r["ratio"]))
        for cls in ("cam", "pt"):
            assert r[cls]["eta"] <= r[cls]["bar"], (step, cls, r[cls])
            assert r[cls]["eta_max"] < 1e-13, (step, cls, r[cls])   # (an fp64 step is nowhere near the bar's ceiling either)
            if (case.name, step, cls) not in BAR_EXCEPTIONS:
                assert r[cls]["bar_max"] <= psa.BAR_CAP, (step, cls, r[cls])
        # the reference's own scalars pass the scalar tolerances through the same round trip
        nd, tol = sysm.step_norm_tolerance(xn)
        assert abs(float(np.linalg.norm((xn - sysm.x)[mdl.free])) - nd) <= tol
    if case.huber:
        past = int(np.sum(sys1.sumsq > case.huber ** 2))
        assert 0 < past < mdl.N, past
    if case.const:
        cc, cp = psa.constants(case, mdl.prob)
        assert not mdl.cam_free[list(cc)].any() and not mdl.pt_free[list(cp)].any() and np.all(mdl.views[list(cp)] > 0)
    if case.zero:
        assert np.all(mdl.x0[6 * psa.ZERO_CAM:6 * psa.ZERO_CAM + 3] == 0.0)


def test_mutations_are_above_the_bar():
    case = psa.BY_NAME["v64"]
    mdl, sys1, x1, sys2, x2 = _two_steps(case)
    floor1 = lambda cls: sys1.forming + 4 * psa.U   # noqa: E731
    seen = {}
    for mut in ("drop_view", "inverse_entry", "neighbour_gp"):
        seen[mut] = sys1.check(mdl.x0 + sys1.reference_step(mut))
    seen["stale_point (step 2)"] = sys2.check(x1 + sys2.reference_step("stale_point", stale=sys1))
    assert sys2.radius != sys1.radius
    seen["radius_not_updated (step 2)"] = sys2.check(x1 + psa.System(mdl, x1, sys1.radius, scale=sys1.s).reference_step())
    for k, r in seen.items():
        print("%-30s eta/bar  camera rows %.2e  point rows %.2e   (%s)" % (k, r["cam"]["ratio"], r["pt"]["ratio"], r["pt"]["row"]))
        assert r["ratio"] > 1.0 and max(r["cam"]["eta_max"], r["pt"]["eta_max"]) > floor1(None), (k, r, "the bar does not see this mutation")
    assert len(seen) >= 4
    # the local mutations are found in the rows of the point they touch
    j21 = int(np.flatnonzero(mdl.pt_free & (mdl.views == 21))[0])
    for k in ("drop_view", "neighbour_gp", "stale_point (step 2)"):
        assert seen[k]["pt"]["row"].startswith("point %d " % j21), (k, seen[k]["pt"]["row"])
    # a scale taken at x1: not a different system (see the module docstring)
    own = psa.System(mdl, x1, sys2.radius)
    for sysm in (sys2, own):
        assert np.all((sysm.diagH[mdl.free].astype(float) * sysm.s[mdl.free] ** 2 > psa.MIN_LM) & (sysm.diagH[mdl.free].astype(float) * sysm.s[mdl.free] ** 2 < psa.MAX_LM))
    assert np.abs(own.s[mdl.free] / sys2.s[mdl.free] - 1.0).max() > 1e-6   # (the scales do differ)
    r = sys2.check(x1 + own.reference_step())
    print("%-30s eta/bar  camera rows %.2e  point rows %.2e" % ("scale_at_x1 (step 2)", r["cam"]["ratio"], r["pt"]["ratio"]))
    assert r["ratio"] <= 1.0


def test_complex_step_rows_equal_the_oracles():
    oracle = oracle_lib.load()
    case = psa.BY_NAME["v64_zero"]   # (with the camera of the first-order rotation branch)
    for c in (psa.BY_NAME["v64"], case):
        mdl = psa.model(c)
        prob = mdl.prob
        r, Jc, Jp = mdl.raw(mdl.x0)
        cams, pts, K = mdl.x0[:mdl.nc].reshape(-1, 6), mdl.x0[mdl.nc:].reshape(-1, 3), prob["intr"].reshape(-1, 4)
        uv = prob["obs"].reshape(-1, 2)
        worst = 0.0
        for n in range(mdl.N):
            ro, jc, jp = oracle.point_residual_jacobian(cams[mdl.ci[n]], pts[mdl.pi[n]], K[mdl.ci[n]], uv[n])
            scale = max(np.abs(jc).max(), np.abs(jp).max())
            worst = max(worst, np.abs(Jc[n] - jc).max() / scale, np.abs(Jp[n] - jp).max() / scale)
            assert np.abs(r[n] - ro).max() <= 1e-12 * max(1.0, np.abs(ro).max())
        print("%s: complex-step rows against the oracle's, worst relative difference %.2e (bar %.2e)" % (c.name, worst, 16 * psa.C_JAC * psa.U))
        assert worst <= 16 * psa.C_JAC * psa.U


def test_shapes_reach_what_they_name():
    cus = step_path_ref.CUS
    for name, (C, P, views) in psa.SHAPES.items():
        if name.startswith("trip"):
            grid = 2 * cus - 16 if C <= 128 else cus - 8
            assert psa.backsub_grid(C) == grid and psa.slices(P) > 4 * grid and psa.slices(P - 128) <= 4 * grid and P % 64 == 37
        else:
            assert P == 6 * 64 + 37
    assert psa.SHAPES["trip64"][1] == 64 * (4 * 496 + 1) + 37 == psa.SHAPES["trip128"][1] and psa.SHAPES["trip256"][1] == 64 * (4 * 248 + 1) + 37
    for case in psa.CASES:
        mdl = psa.model(case)
        C, P, views = psa.SHAPES[case.shape]
        views = case.views or views
        assert np.array_equal(psa.view_histogram(mdl.prob), psa.expected_histogram(P, views))
        assert (0 in views) == bool(np.any(mdl.views == 0)) and mdl.cam_obs[mdl.cam_free].min() >= 6
        # every slice of 64 points mixes view counts: padding lanes beside valid ones, and the slots past the registers / LDS
        for s in range(psa.slices(P)):
            v = mdl.views[64 * s:64 * s + 64]
            assert v.min() < v.max() and (v.max() == max(views) or case.shape.startswith("trip"))
    # the slot edges: kReg, kReg + 1, kReg + kLds, kReg + kLds + 1 of every instance occur as view counts of its pad
    for cyc, edges in ((psa.VIEWS_64, (9, 10, 11, 20, 21, 24)), (psa.VIEWS_128, (9, 10, 11, 16, 17, 20))):
        assert set(edges) <= set(cyc)
    # the forms the settings name
    forms = {(psa._tag_free(e), i, c): psa.expected_form(psa.BY_NAME[c], e, i) for e, i, cs in psa.SETTINGS for c in cs}
    assert forms[("", 1, "v64")] == "proj<64,10+10>" and forms[("", 1, "v64_huber")] == "proj<64,9+11,loss>"
    assert forms[("", 1, "v128")] == "proj<128,10+6>" and forms[("", 1, "v128_huber")] == "proj<128,9+7,loss>"
    assert forms[("", 1, "v256")] == "proj<256,10+10>" and forms[("", 1, "trip256_huber")] == "proj<256,10+10,loss>"
    assert forms[("RSBA_BACKSUB_PROJ=0", 1, "v64")] == "staged fused" and forms[("RSBA_BACKSUB_PROJ=0", 1, "v256")] == "plain fused"
    assert forms[("", 0, "v64")] == "staged not fused" and forms[("", 0, "v256")] == "plain not fused"
    assert forms[("RSBA_FUSED_LIN=0", 1, "v64")] == "staged not fused"
    assert 130 * psa.BACKSUB_LDS_PER_CAMERA > 60 * 1024 >= 26 * psa.BACKSUB_LDS_PER_CAMERA
