"""Levenberg-Marquardt step SEQUENCES of the numpy references: the accept / reject patterns a step test can follow (host code, numpy only).

A solver run with min_relative_decrease = thr takes a step when its relative decrease rho exceeds thr and rejects it otherwise.
With thr between the reference's rho values of consecutive candidates a run follows a chosen pattern, 'RA', 'RRA', 'ARA', 'ARRA', 'AA':
a run that ends on a rejected step leaves x at its base point; the run one iteration longer that ends on an accepted step moved by
x_k - x_base, which solves the damped normal equations AT THE UNCHANGED BASE POINT with the radius the rejected step's log row reports
and iteration 0's Jacobi scale: exactly point_step_accuracy.System(mdl, x_base, radius, scale=...) (marker_step_accuracy.System on the
marker chain).  So the step after a rejection is observable through the public API, and is held to the bars of those two files.

walk() goes through Ceres' rules as TrustRegionMinimizer / LevenbergMarquardtStrategy state them:
    reject:  radius /= f;  f *= 2
    accept:  radius = min(max_trust_region_radius, radius / max(1/3, 1 - (2 rho - 1)^3));  f = 2
with the references' own fp64 steps (System.reference_step() on the point model, a numpy solve of System.A d = b on the marker
chain), and returns per iterate the base point, the radius, rho, the decision and the System the step solved.

Margin (a condition on the case, not a measurement): every rho of a pattern lies at least MARGIN = 1e-3 from thr, and MARGIN is at
least 1000 times the rho uncertainty the scalar tolerances of the step tests allow, (1e-12 cost + tol(model cost change) |rho|) /
model cost change: a device whose scalars pass those tolerances takes the reference's decisions.  tests/test_step_sequence_cpu.py
asserts both; the GPU tests assert the flags in any case.

Scale-visible cases.  D / s^2 = diag(H) / radius wherever the clip to [min_lm_diagonal, max_lm_diagonal] is inactive, so the Jacobi
scale drops out of the system and no step test sees a stale or wrong one.  With min_lm_diagonal = 0.999 the clip is active on every
free column (diag(H) s^2 = (sqrt(d) / (1 + sqrt(d)))^2 < 0.999 while sqrt(d) < 1999: asserted), the damping is
0.999 (1 + sqrt(diag H_0))^2 / radius, and iteration 0's scale enters the system a later step solves.
"""
from collections import namedtuple

import numpy as np

import marker_loss_ref as ref
import marker_step_accuracy as msa
import point_step_accuracy as psa

U = psa.U
MARGIN = 1e-3
MAX_RADIUS = 1e16          # rsba_options_default: max_trust_region_radius
MIN_LM_VISIBLE = 0.999     # min_lm_diagonal of the scale-visible cases

# One iterate: `system` the damped normal equations the step solved (base point x, radius, iteration 0's scale), x_cand = fl(x + delta),
# rho its relative decrease, mcc / mcc_tol the model cost change and the tolerance the step tests allow it, cost / cand the costs at x
# and x_cand, accepted the decision at thr, factor the decrease factor BEFORE the decision, next_radius / next_factor after it.
Step = namedtuple("Step", "index system x radius factor x_cand rho mcc mcc_tol cost cand accepted next_radius next_factor")


class PointAdapter:
    """The point model (point_step_accuracy): x is all 6 C + 3 P parameters."""

    def __init__(self, mdl, min_lm=psa.MIN_LM):
        self.mdl, self.min_lm, self._systems = mdl, min_lm, {}

    def system(self, x, radius, scale):
        """The System at (x, radius), built once: the patterns of one start share their systems (scale: None or iteration 0's, which
        is one vector per adapter)."""
        key = (np.asarray(x, float).tobytes(), float(radius), scale is None)
        if key not in self._systems:
            self._systems[key] = psa.System(self.mdl, x, radius, scale=scale, min_lm=self.min_lm)
        return self._systems[key]

    def step(self, sysm):
        return sysm.reference_step()

    def cost(self, x):
        return self.mdl.cost(x)

    def free(self, sysm):
        return self.mdl.free


class MarkerAdapter:
    """The marker chain (marker_step_accuracy): x is the free blocks' vector."""

    def __init__(self, mc, dense, min_lm=msa.MIN_LM):
        self.mc, self.dense, self.min_lm = mc, dense, min_lm

    def system(self, x, radius, scale):
        return msa.System(self.mc, x, radius, dense=self.dense, min_lm=self.min_lm, scale=scale)

    def step(self, sysm):
        return np.linalg.solve(np.asarray(sysm.A, np.float64), np.asarray(sysm.b, np.float64))

    def cost(self, x):
        return self.mc.cost(x)[0]

    def free(self, sysm):
        return np.ones(sysm.n, bool)


def next_radius_accepted(radius, rho, max_radius=MAX_RADIUS):
    return min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))


def rho_uncertainty(st):
    """What the step tests' scalar tolerances leave open of a step's rho: 1e-12 relative on each cost, the model cost change's own."""
    return (1e-12 * st.cost + st.mcc_tol * abs(st.rho)) / st.mcc


def candidate(ad, x, radius, scale):
    """(system, x_cand, rho, mcc, mcc_tol, cost, cand) of the reference's step from x at radius."""
    sysm = ad.system(x, radius, scale)
    x_cand = sysm.x + ad.step(sysm)
    mcc, mcc_tol = sysm.model_cost_change(x_cand)
    cand = ad.cost(x_cand)
    return sysm, x_cand, (sysm.cost - cand) / mcc, mcc, mcc_tol, sysm.cost, cand


def walk(ad, x0, radius0, thr, steps, max_radius=MAX_RADIUS):
    """`steps` iterations of the reference from x0 at radius0 under min_relative_decrease = thr -> [Step].  Every System carries
    iteration 0's scale."""
    x, radius, f, scale, out = np.asarray(x0, float).copy(), float(radius0), 2.0, None, []
    for k in range(steps):
        sysm, x_cand, rho, mcc, mcc_tol, cost, cand = candidate(ad, x, radius, scale)
        if scale is None:
            scale = sysm.s.copy()
        assert mcc > 0.0 and np.all(np.isfinite(x_cand)), "an invalid step: not what these sequences are about"
        ok = bool(rho > thr)
        nr, nf = (next_radius_accepted(radius, rho, max_radius), 2.0) if ok else (radius / f, 2.0 * f)
        out.append(Step(k + 1, sysm, x.copy(), radius, f, x_cand, rho, mcc, mcc_tol, cost, cand, ok, nr, nf))
        x, radius, f = (x_cand if ok else x), nr, nf
    return out


def pattern_of(steps):
    return "".join("A" if s.accepted else "R" for s in steps)


def held(steps):
    """The steps a sequence test holds to the bar: every accepted one (its System is the one the run's x_k - x_base must solve)."""
    return [s for s in steps if s.accepted]


# ------------------------------------------------------------------------------------------------ cases
# model 'point' | 'marker'; base: the point_step_accuracy.Case / marker_step_accuracy.Case whose problem, loss, constants, switches
# and start the sequence uses (its radius field is the sequence's R0); thr: min_relative_decrease; pattern: what the reference walks
# at thr; min_lm: min_lm_diagonal (MIN_LM_VISIBLE on the scale-visible cases); loss_a: the marker chain's loss scale (px).
SeqCase = namedtuple("SeqCase", "name model base thr pattern min_lm loss_a")
ACCEPT_ALL = -1e300

# The point model's starts are point_step_accuracy.perturbed_start's.  Relative decreases of the reference (this file's walk, CPU):
#   v64, sigma 0.2, no loss:  x0, R0 = 0.3: 0.92418 0.94562 0.98071 at R0, R0 / 2, R0 / 8;  R0 = 0.1: 0.95811, then x1, R1 = 0.3: 0.93241
#                             0.95187 0.98309
#   Huber.  With huber_delta = 1 px (point_step_accuracy.HUBER) nearly every residual of a perturbed start is on the loss's linear
#   branch; the relative decrease is then above 1 and GROWS with the radius (1.02 .. 1.85 over sigma 0.003 .. 0.5 and R0 0.03 .. 1e5,
#   both outside the grid the cases were first looked for in, sigma 0.1 / 0.2 and R0 0.03 .. 3), so no rejection can be followed by an
#   acceptance; at delta = 40 px, the median |r| of sigma 0.1, it is the same (1.025 .. 1.13 over R0 0.1 .. 1).  delta = 100 px leaves
#   2 % of the observations (95 of 4753 on v64) on the linear branch, the outliers among them (both branches asserted), and gives
#   v64 + outliers:   x0, R0 = 0.1: 0.98613 0.99213 0.99780;  x1, R1 = 0.3: 0.97219 0.98093 0.99373
#   v256 + outliers:  x0, R0 = 0.1: 0.98810 0.99328 0.99815;  x1, R1 = 0.3: 0.97963 0.98600 0.99537  (ARRA: a threshold needs
#                     0.98600 + 1e-3 <= thr <= 0.98810 - 1e-3: 0.98705, with margins of 1.05e-3 on both sides)
#   scale-visible (min_lm_diagonal 0.999): on v64 without a loss 52 camera columns have sqrt(diag H) >= 1999 and the clip is inactive
#   there; v256 (fewer observations a camera) has none: sigma 0.2, x0, R0 = 0.3: 0.93165 0.95128
SEQ_HUBER = 100.0


def _pt(shape, pattern, radius, thr, sigma, huber=0.0, min_lm=psa.MIN_LM):
    tag = ("huber" if huber else "plain") + ("_vis" if min_lm != psa.MIN_LM else "")
    base = psa.Case("%s_%s_s%g_r%g" % (shape, tag, sigma, radius), shape, huber, False, False, radius, None, sigma)
    return SeqCase("%s_%s_%s" % (shape, tag, pattern), "point", base, thr, pattern, min_lm, None)


POINT_CASES = [
    _pt("v64", "RA", 0.3, 0.935, 0.2), _pt("v64", "RRA", 0.3, 0.963, 0.2), _pt("v64", "ARA", 0.1, 0.942, 0.2), _pt("v64", "ARRA", 0.1, 0.9555, 0.2),
    _pt("v64", "RA", 0.1, 0.989, 0.1, SEQ_HUBER), _pt("v64", "RRA", 0.1, 0.995, 0.1, SEQ_HUBER), _pt("v64", "ARA", 0.1, 0.9765, 0.1, SEQ_HUBER),
    _pt("v64", "ARRA", 0.1, 0.9845, 0.1, SEQ_HUBER),
    _pt("v256", "RA", 0.1, 0.9907, 0.1, SEQ_HUBER), _pt("v256", "RRA", 0.1, 0.9957, 0.1, SEQ_HUBER), _pt("v256", "ARA", 0.1, 0.9828, 0.1, SEQ_HUBER),
    _pt("v256", "ARRA", 0.1, 0.98705, 0.1, SEQ_HUBER),
    _pt("v256", "AA", 0.3, ACCEPT_ALL, 0.2, min_lm=MIN_LM_VISIBLE), _pt("v256", "RA", 0.3, 0.941, 0.2, min_lm=MIN_LM_VISIBLE),
]
POINT_BY_NAME = {c.name: c for c in POINT_CASES}
assert len(POINT_BY_NAME) == len(POINT_CASES)

# (environment, schur_impl, case names): one child process each (RSBA_* is read once per process)
_DEFAULTS = [c.name for c in POINT_CASES]
_TWO = ["v64_plain_RA", "v64_plain_ARRA"]
POINT_SETTINGS = [
    ({}, 1, [n for n in _DEFAULTS if n.startswith("v64_plain")]), ({}, 1, [n for n in _DEFAULTS if n.startswith("v64_huber")]),
    ({}, 1, [n for n in _DEFAULTS if n.startswith("v256_huber_")]), ({}, 1, [n for n in _DEFAULTS if n.startswith("v256_plain_vis")]),
    # (schur_impl = 0 is not reproducible to the bit from one solver to the next, so the base point of a step behind an ACCEPTED
    #  step is not observable there: rejections from x0 only, 'RRA' in the place of 'ARRA')
    ({}, 0, ["v64_plain_RA", "v64_plain_RRA"]), ({"RSBA_BACKSUB_PROJ": "0"}, 1, _TWO), ({"RSBA_FUSED_LIN": "0"}, 1, _TWO), ({"RSBA_DECIDED_DAMP": "0"}, 1, _TWO),
    ({"RSBA_PIPELINE": "0"}, 1, _TWO), ({"RSBA_FORCE_COMM": "1"}, 1, _TWO),
]

# The marker chain.  Relative decreases of the reference (marker_step_accuracy.System, a numpy solve of A d = b):
#   hongo, R0 = 1e4:                      0.32507 0.49839 0.70396 at R0, R0 / 2, R0 / 8
#   6x8x6 displaced, Huber, R0 = 100:     1.17461, then x1, R1 = 300: 0.89989 0.92405 0.94067
#   8x24x12, R0 = 0.1:                    0.98881 0.99282
#   scale-visible: sqrt(diag H) reaches 2e4 on every marker-chain problem of the suite (the rotation columns of a block many corners
#   name), so min_lm_diagonal = 0.999 clips only half the columns; under Huber with a = 0.03 px every block is on the linear branch, the
#   rows are scaled by sqrt(a / |r|) and hongo's largest sqrt(diag H) is 1550: R0 = 1e4: 0.17493 0.51227;  R0 = 100: 1.40966 (AA)
VISIBLE_A = 0.03


def _mk(name, prob, pattern, radius, thr, impl, loss="none", env=None, min_lm=msa.MIN_LM, loss_a=None):
    base = msa.make_case("%s_impl%d" % (name, impl), prob, impl=impl, loss=loss, radius=radius, env=env)
    tag = ",".join("%s=%s" % (k[8:], v) for k, v in sorted((env or {}).items()))
    return SeqCase("%s_impl%d_%s%s" % (name, impl, pattern, "_" + tag if tag else ""), "marker", base, thr, pattern, min_lm,
                   loss_a if loss_a is not None else (msa.LOSS_A if loss != "none" else 0.0))


def _marker_cases():
    S = lambda C, T, M, keep=0.9: ("syn", C, T, M, keep)   # noqa: E731  (marker_step_accuracy's key of a synthetic problem)
    out = []
    for impl in (0, 2):
        out += [_mk("hongo", ("hongo",), "RA", 1e4, 0.4, impl), _mk("hongo", ("hongo",), "RRA", 1e4, 0.6, impl),
                _mk("disp_6x8x6_huber", ("disp", S(6, 8, 6)), "ARA", 100.0, 0.91, impl, loss="huber"),
                _mk("disp_6x8x6_huber", ("disp", S(6, 8, 6)), "ARRA", 100.0, 0.93, impl, loss="huber")]
    out += [_mk("8x24x12", S(8, 24, 12), "RA", 0.1, 0.991, 2), _mk("8x24x12", S(8, 24, 12), "RA", 0.1, 0.991, 2, env={"RSBA_MT_SPLIT": "0"})]
    out += [_mk("8x24x12", S(8, 24, 12), "AA", 1e4, ACCEPT_ALL, 2), _mk("dense_4x40x6", S(4, 40, 6), "AA", 1e4, ACCEPT_ALL, 0),
            _mk("hongo", ("hongo",), "AA", 1e4, ACCEPT_ALL, 2), _mk("hongo", ("hongo",), "AA", 1e4, ACCEPT_ALL, 0)]
    for impl in (0, 2):
        out += [_mk("hongo_vis", ("hongo",), "AA", 100.0, ACCEPT_ALL, impl, loss="huber", min_lm=MIN_LM_VISIBLE, loss_a=VISIBLE_A),
                _mk("hongo_vis", ("hongo",), "RA", 1e4, 0.35, impl, loss="huber", min_lm=MIN_LM_VISIBLE, loss_a=VISIBLE_A)]
    return out


MARKER_CASES = _marker_cases()
assert len({c.name for c in MARKER_CASES}) == len(MARKER_CASES)


def marker_chain(case, prob=None):
    """The reference model of a marker-chain case (at prob's parameters; None: the problem's own start)."""
    b = case.base
    prob = msa.problem(b.prob) if prob is None else prob
    return ref.MarkerChain(prob, b.variant, b.loss, case.loss_a, msa.constant_blocks(b, prob))


_ADAPTERS = {}


def adapter(case):
    """The adapter of a case, once per (problem, loss, min_lm_diagonal): the patterns of one start share its systems."""
    b = case.base
    if case.model == "point":
        key = ("point", b.shape, b.huber, b.perturb, case.min_lm)
        if key not in _ADAPTERS:
            _ADAPTERS[key] = PointAdapter(psa.model(b), case.min_lm)
    else:
        key = ("marker", b.prob, b.variant, b.loss, case.loss_a, b.impl == 0, case.min_lm)
        if key not in _ADAPTERS:
            _ADAPTERS[key] = MarkerAdapter(marker_chain(case), b.impl == 0, case.min_lm)
    return _ADAPTERS[key]


def start(case, ad):
    return ad.mdl.x0 if case.model == "point" else ad.mc.x0()


_WALKS = {}


def reference_walk(case):
    """(adapter, [Step]) of a case: the reference's own len(pattern) iterations at the case's thr, once."""
    if case.name not in _WALKS:
        ad = adapter(case)
        _WALKS[case.name] = (ad, walk(ad, start(case, ad), case.base.radius, case.thr, len(case.pattern)))
    return _WALKS[case.name]
