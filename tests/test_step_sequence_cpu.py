"""The step sequences of tests/step_sequence.py hold in the references, without a GPU: on every case of tests/test_gpu_point_sequence.py
and tests/test_gpu_marker_sequence.py,

  * the reference walks the case's accept / reject pattern at the case's threshold, every relative decrease at least MARGIN = 1e-3
    from it, and MARGIN is at least 1000 times what the step tests' scalar tolerances leave open of a relative decrease, so a device
    whose scalars pass them takes the same decisions; the radii follow Ceres' rule (a rejection divides by 2, 4, 8 ...: exact);
  * the reference's own fp64 step stays within the bar of point_step_accuracy.py / marker_step_accuracy.py at every held (accepted)
    step, through the same x_k = fl(x_base + delta) round trip;
  * each of these mutations of the held step behind a rejection exceeds that bar (no new bar, nothing fitted):
      (i)   the step taken at the un-reduced radius (the rejection's division lost);
      (ii)  after two rejections, radius / 4 instead of / 8 (the decrease factor not doubled);
      (iii) 'ARA' with radius / 4 instead of / 2 (the decrease factor not reset to 2 by the acceptance);
      (iv)  point model: the point rows damped at the previous radius and the camera rows at the new one (a stale decrease factor
            on the device, which damps the points itself);
      (v)   the scale-visible cases: the Jacobi scale re-taken at the new point ('AA': at x1; 'RA': at the rejected candidate, the
            only other point a linearisation exists at) instead of iteration 0's;
      (vi)  the step solved from the rejected candidate's linearisation instead of the kept one;
  * on the scale-visible cases the clip to min_lm_diagonal is active on every free column at every point a step starts from when the
    scale is that point's own (sqrt(diag H) < 1999), which is what iteration 0 and mutation (v) compute.  With iteration 0's scale at
    a LATER point, diag(H) s0^2 exceeds 0.999 wherever diag H grew by more than about 2 / sqrt(diag H): there a correct step is damped
    with diag(H) / radius, and so is the reference; the count of columns still clipped is printed and is at least a quarter of the free
    columns (a condition on the case, so that a change of cases cannot empty the check), and what shows that the kept scale is
    visible is mutation (v) itself."""
import numpy as np
import pytest

import marker_step_accuracy as msa
import point_step_accuracy as psa
import step_sequence as ss

# A condition on a scale-visible case, like the margin: at a later base point iteration 0's scale still sets the damping of at least a
# quarter of the free columns (counted in the reference alone; the cases have 54 of 114 on hongo and 1917 of 1926 on v256).
MIN_KEPT = 0.25
ALL_CASES = ss.POINT_CASES + ss.MARKER_CASES
# the numpy side does not depend on the switches: one case per (reference walk)
_UNIQUE = {}
for _c in ALL_CASES:
    _b = _c.base
    _k = (_c.model, _b.shape if _c.model == "point" else (_b.prob, _b.impl == 0), getattr(_b, "huber", None) or getattr(_b, "loss", None),
          _b.radius, _c.thr, _c.pattern, _c.min_lm)
    _UNIQUE.setdefault(_k, _c)
CASES = list(_UNIQUE.values())


def _trailing_rejections(pattern):
    return len(pattern) - 1 - len(pattern[:-1].rstrip("R"))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_pattern_margins_and_reference_steps(case):
    ad, steps = ss.reference_walk(case)
    x0 = ss.start(case, ad)
    assert np.linalg.norm(x0[ad.free(steps[0].system)]) > 1.0   # (parameter_tolerance = -1 ends a run only below |x| = 1)
    assert ss.pattern_of(steps) == case.pattern, [(s.radius, s.rho) for s in steps]
    assert case.pattern.endswith("A")
    f, radius = 2.0, case.base.radius
    for st in steps:
        unc = ss.rho_uncertainty(st)
        print("\n%-32s step %d %s radius %-10.6g rho %.5f (thr %.5g) uncertainty %.1e" % (case.name, st.index, "A" if st.accepted else "R", st.radius, st.rho,
                                                                                   case.thr, unc))
        assert abs(st.rho - case.thr) >= ss.MARGIN and ss.MARGIN >= 1000.0 * unc, (st.rho, case.thr, unc)
        assert st.radius == radius and st.factor == f
        if st.accepted:
            assert st.next_radius == ss.next_radius_accepted(radius, st.rho) and st.next_factor == 2.0
            r = st.system.check(st.x_cand)
            print("%-32s step %d held: eta/bar %.3f" % (case.name, st.index, r["ratio"]))
            assert r["ratio"] <= 1.0, r
            nd, tol = st.system.step_norm_tolerance(st.x_cand)
            assert abs(float(np.linalg.norm((st.x_cand - st.x)[ad.free(st.system)])) - nd) <= tol
        else:
            assert st.next_radius == radius / f and st.next_factor == 2.0 * f
        f, radius = st.next_factor, st.next_radius
    # a step behind k rejections: the radius of the first of them over 2, 8, 64 ...
    k = _trailing_rejections(case.pattern)
    if k:
        assert steps[-1].radius == steps[-1 - k].radius / (2.0, 8.0, 64.0)[k - 1] and np.array_equal(steps[-1].x, steps[-1 - k].x)
    if case.model == "point" and case.base.huber:
        past = int(np.sum(steps[0].system.sumsq > case.base.huber ** 2))
        print("%-32s %d of %d observations past the loss's threshold" % (case.name, past, ad.mdl.N))
        assert 0 < past < ad.mdl.N, past
    if case.min_lm == ss.MIN_LM_VISIBLE:
        s0 = steps[0].system.s
        for st in steps:   # (every base point; the held step's system clips with iteration 0's scale, mutation (v)'s with the point's own)
            own = ad.system(st.x, 1.0, None)
            free = ad.free(own)
            dH = (own.diagH if case.model == "point" else np.diagonal(own.H)).astype(np.float64)[free]
            kept = dH * s0[free] ** 2 < case.min_lm
            print("%-32s step %d: largest diag(H) s^2 %.4f; with iteration 0's scale the clip is active on %d of %d free columns" % (
                case.name, st.index, (dH * own.s[free] ** 2).max(), kept.sum(), kept.size))
            assert np.all(dH * own.s[free] ** 2 < case.min_lm)
            assert kept.all() if np.array_equal(st.x, x0) else kept.sum() >= MIN_KEPT * kept.size, (kept.sum(), kept.size)


def _mutations(case, ad, steps):
    """{mutation: eta / bar of the mutated step against the held step's system} of the case's last step."""
    st, scale0 = steps[-1], steps[0].system.s
    k = _trailing_rejections(case.pattern)
    out = {}

    def ratio(sysm_mut):
        return st.system.check(st.x + ad.step(sysm_mut))["ratio"]

    if k:
        first = steps[-1 - k]
        out["(i) un-reduced radius"] = ratio(ad.system(st.x, first.radius, scale0))
        out["(vi) the rejected candidate's linearisation"] = ratio(ad.system(steps[-2].x_cand, st.radius, scale0))
        if case.model == "point":
            stale = psa.System(ad.mdl, st.x, st.radius, scale=scale0, min_lm=case.min_lm)   # (its own object: D is changed)
            stale.D[ad.mdl.nc:] *= st.radius / steps[-2].radius
            out["(iv) point rows at the previous radius"] = ratio(stale)
    if k == 2:
        out["(ii) radius / 4 after two rejections"] = ratio(ad.system(st.x, first.radius / 4.0, scale0))
    if case.pattern == "ARA":
        out["(iii) decrease factor not reset"] = ratio(ad.system(st.x, first.radius / 4.0, scale0))
    if case.min_lm == ss.MIN_LM_VISIBLE:
        where = st.x if case.pattern == "AA" else steps[-2].x_cand
        own = ad.system(where, st.radius, None)
        assert np.abs(own.s / scale0 - 1.0)[ad.free(own)].max() > 1e-6   # (the scales do differ)
        retaken = (psa.System(ad.mdl, st.x, st.radius, scale=own.s, min_lm=case.min_lm) if case.model == "point" else
                   msa.System(ad.mc, st.x, st.radius, dense=ad.dense, min_lm=case.min_lm, scale=own.s))
        out["(v) scale re-taken"] = ratio(retaken)
    return out


def test_mutations_are_above_the_bar():
    seen = {}
    for case in CASES:
        if case.pattern == "AA" and case.min_lm != ss.MIN_LM_VISIBLE:
            continue
        ad, steps = ss.reference_walk(case)
        for k, v in _mutations(case, ad, steps).items():
            print("%-34s %-46s eta/bar %.3g" % (case.name, k, v))
            seen.setdefault(k[:k.index(")") + 1], []).append((case.name, v))
    assert sorted(seen) == ["(i)", "(ii)", "(iii)", "(iv)", "(v)", "(vi)"]
    for k, rows in seen.items():
        # every case a mutation applies to sees it: the bar is not merely crossed somewhere
        assert all(v > 1.0 for _, v in rows), (k, rows)
    # (v) on both models, an 'AA' and an 'RA' each
    assert sorted(n for n, _ in seen["(v)"]) == sorted(c.name for c in CASES if c.min_lm == ss.MIN_LM_VISIBLE) and len(seen["(v)"]) >= 4


def test_case_lists():
    names = {c.name for c in ss.POINT_CASES}
    for env, impl, cases in ss.POINT_SETTINGS:
        assert set(cases) <= names and cases
    default = [n for e, i, cs in ss.POINT_SETTINGS if not e and i == 1 for n in cs]
    assert sorted(default) == sorted(names)
    for sw in ("RSBA_BACKSUB_PROJ", "RSBA_FUSED_LIN", "RSBA_DECIDED_DAMP", "RSBA_PIPELINE"):
        assert any(e == {sw: "0"} and cs == ["v64_plain_RA", "v64_plain_ARRA"] for e, i, cs in ss.POINT_SETTINGS)
    assert any(e == {"RSBA_FORCE_COMM": "1"} and cs == ["v64_plain_RA", "v64_plain_ARRA"] for e, i, cs in ss.POINT_SETTINGS)
    # schur_impl = 0: rejections from x0 only (see POINT_SETTINGS)
    assert [cs for e, i, cs in ss.POINT_SETTINGS if i == 0] == [["v64_plain_RA", "v64_plain_RRA"]]
    assert {c.pattern for c in ss.POINT_CASES if c.name.startswith("v64_plain")} == {"RA", "RRA", "ARA", "ARRA"}
    assert psa.SHAPES["v256"][0] > 64 and not any(c.base.shape.startswith("trip") for c in ss.POINT_CASES)
    # the stock cases are what they were: no perturbation
    assert all(c.perturb == 0.0 for c in psa.CASES)
    assert {(c.base.impl, c.pattern) for c in ss.MARKER_CASES if c.name.startswith("hongo_impl")} >= {(0, "RA"), (2, "RA"), (0, "RRA"), (2, "RRA")}
    assert sum(1 for c in ss.MARKER_CASES if c.pattern == "AA" and c.min_lm != ss.MIN_LM_VISIBLE) >= 3
    assert any(dict(c.base.env) == {"RSBA_MT_SPLIT": "0"} for c in ss.MARKER_CASES)
