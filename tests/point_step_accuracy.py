"""One LM step of the POINT model as a linear solve: its backward error, and the bar any correct fp64 step meets (host code).
The marker-chain counterpart, with the measure's derivation, is tests/marker_step_accuracy.py; this file restates it for the point
model's structure and adds the second step.

What is measured.  A capi.Solver run with max_num_iterations = 1 (2), the three tolerances at -1 and min_relative_decrease = -1e300
takes exactly one (two) accepted steps, so delta1 = x1 - x0 and delta2 = x2 - x1 over the free blocks are observable through the
public API whichever kernels formed them: the Schur kernels, the factorisation of the reduced camera system and one of the three
forms of the point back-substitution (LaunchPointBacksub, csrc/ba_solver.hip).  Each must solve the FULL damped normal equations

    A delta = b,     A = H + diag(D / s^2),   b = -g,   H = J~'J~,   g = J~'r~       (J~, r~: the rows scaled by sqrt(rho'))
    s = 1 / (1 + sqrt(diag H)) taken at ITERATION 0's parameters for both steps (the Jacobi scale is fixed there),
    D = clip(diag(H) s^2, min_lm_diagonal, max_lm_diagonal) / radius

Rows: per observation the residual and its 2 x 6 / 2 x 3 blocks from a vectorised complex step (h = 1e-30) of the residual of
tools/replay_point_model.py (rotate, residuals: six plus three perturbed evaluations of all observations at once); no code shared
with the product or the oracle.  The rows stay per observation: A is applied matrix-free in np.longdouble, J delta per observation
and J'(.) with np.add.at; no dense J is ever built.  Constant blocks and points no observation names are not in the system.

Measure (solve_accuracy.backward_errors' formula), per free row i, camera rows and point rows reported apart:

    eta_i = |b_i - (A delta)_i| / ( sqrt(A_ii) sum_j sqrt(A_jj) |delta_j| + |b_i| )

Bar.  Per row, the sum of four terms (u = 2^-53, gamma_k = k u / (1 - k u)); nothing in it is fitted to a measurement.

 1. Forming A and b:  gamma_{m+2c} / (1 - gamma_{m+2c}),  m = 2 x the most observations that name one free block (the longest sum
    behind an entry of A), c = 24 roundings behind one entry of the analytic rows (tests/test_gpu_jacobian.py's count for the point
    model), two factors a product.
 2. Elimination and solve.  G(n) = gamma_{3n+1} / (1 - gamma_{n+1}) is the componentwise backward error of a Cholesky solve of n
    unknowns in the metric of the diagonal (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 / 10.4 as in
    solve_accuracy.py); a block inverted explicitly stretches the terms that run through it by (1 + kappa_inf) of that block (sec.
    14.2).  Eliminating the points and factoring the reduced system is a block Cholesky factorisation of A with the points first;
    the marker chain's bar takes G(all unknowns) (1 + the largest kappa) for every row.  Here that would be vacuous (381 000
    unknowns on the trip problems, a one-view block's kappa ~ radius beside every other row), so the term follows the sparsity:
      * a point row (eliminated first, never filled in):  G(3 + 6 v) (1 + kappa_j),  v the free cameras that see the point.
        Derivation: delta_p = -s_p (V_j + D_j)^-1 (s_p g_p - sum_views W_cj' y_c) is computed from the device's OWN camera step, so
        the point's three equations hold for that camera step up to the roundings of this one chain, 6 multiply-adds per view and
        component and a 3 x 3 product: a solve whose unknowns are the point's 3 and the 6 of each such camera, whatever error the
        camera step itself carries (that error shows in the camera rows).  kappa_j = kappa_inf of the point's own 3 x 3 block
        V_j + D_j in Jacobi-scaled coordinates: PointBlockInverse (ba_math.hpp) inverts it explicitly (LL', L^-1, L^-T L^-1).  A
        one-view block is held by the damping alone: kappa ~ radius.
      * a camera row:  G(6 C_free) (1 + kappa_s)  +  G(3) (1 + max kappa_j)  +  gamma_{3 p}.
        Derivation: an error dS in the reduced system S = U - sum_j W_j (V_j + D_j)^-1 W_j' is the same error in A's camera block
        (the Schur complement of A + [dS 0; 0 0] is S + dS), so forming S adds to the backward error and is not stretched by the
        reduced solve.  Each point's term is a 3 x 3 solve through that point's explicit inverse, G(3) (1 + kappa_j), the largest
        over the free points the camera sees, and |W_j (V_j + D_j)^-1 W_j'| is bounded entrywise by sqrt(A_ii A_jj) (the term is a
        part of U, Cauchy-Schwarz); the p such points' terms are added up, three products each, gamma_{3 p}.  The reduced solve
        itself has the 6 C_free camera unknowns; kappa_s = the largest kappa_inf over the 32-wide diagonal blocks of the Cholesky
        factor of the reduced system, which the factorisations invert explicitly (solve_accuracy.diag_block_kappas on the host's own
        Schur complement, Jacobi-scaled).  No camera is held fixed, so at radius 1e12 the gauge directions of S are held by the
        damping alone: kappa_s ~ sqrt(radius) and the CAMERA rows' bar of that one case is 1e-7; its point rows stay at 1e-13.
 3. Recovery: delta is known only as x1 - x0 (exact in np.longdouble) with x1 = fl(x0 + delta), at most u |x1_i| per component,
    which moves row i's residual by at most (|A| u |x1|)_i: that over the row's denominator is added, per row (|A| from A's own
    blocks U_c, V_j and the per-observation W = Jc'Jp; every (camera, point) pair is observed at most once).
 4. 4 u for the candidate's addition and the negation / scaling delta = -s y in front of it.

The log's scalars, with marker_step_accuracy.py's tolerances unchanged: cost 1e-12 relative; gradient_max_norm 1e-11 relative;
step_norm 4 u sqrt(n) relative plus the recovery |u x1| / |delta|; the model cost change (cost_change / relative_decrease) at the
DEVICE's delta 1e-11 relative plus |(g + H delta)' u x1|; the candidate cost (cost - cost_change) at the downloaded x1 1e-12
relative plus u (|cost_change| + candidate) for the log's subtraction.

Problems.  synthetic.make_problem gives every point the same number of views; thin() removes observations so that point j keeps
views[j % len(views)] of its cameras (a seeded choice), which puts padding lanes (cam < 0) beside valid ones in every slice of 64
points and walks the projective kernel's slots: kReg records in registers, kLds in LDS, the rest streamed (10 + 10, 9 + 11 with a
loss up to 64 cameras; 10 + 6, 9 + 7 up to 128; 10 + 10 up to 256).  The trip problems are the smallest whose slice count exceeds
4 x grid, the second trip of the kernel's slice loop.  tests/test_point_step_accuracy_cpu.py shows the bar neither vacuous nor false.
"""
import os
import sys
from collections import namedtuple

import numpy as np

import marker_loss_ref
import solve_accuracy as sa
import step_path_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import replay_point_model as rp  # noqa: E402

U = sa.U
LD = np.longdouble
C_JAC = 24                    # roundings behind one entry of the analytic rows (tests/test_gpu_jacobian.py, point model)
MIN_LM, MAX_LM = 1e-6, 1e32   # rsba_options_default
BAR_CAP = 1e-9                # no row's bar exceeds this but the camera rows at radius 1e12 (test_point_step_accuracy_cpu.py)
HUBER = 1.0
H_STEP = 1e-30
BACKSUB_LDS_PER_CAMERA = 576  # kBacksubLdsBytesPerCamera (ba_step_plan.hpp)

VIEWS_64 = (0, 1, 2, 8, 9, 10, 11, 19, 20, 21, 24)
VIEWS_128 = (0, 1, 2, 8, 9, 10, 11, 15, 16, 17, 20)
VIEWS_TRIP = (2, 3)
P_V = 6 * 64 + 37


def backsub_grid(C):
    """Workgroups of k_backsub_candidate_proj before the cap by the slice count (LaunchPointBacksub)."""
    return 2 * step_path_ref.CUS - 16 if C <= 128 else step_path_ref.CUS - 8


def trip_points(C):
    """The smallest point count with a partial last slice of 37 whose slices exceed 4 x grid."""
    return 64 * (4 * backsub_grid(C) + 1) + 37


# name -> (C, P, views cycled)
SHAPES = {"v64": (26, P_V, VIEWS_64), "v128": (70, P_V, VIEWS_128), "v256": (130, P_V, VIEWS_64),
          "trip64": (8, trip_points(8), VIEWS_TRIP), "trip128": (70, trip_points(70), VIEWS_TRIP), "trip256": (130, trip_points(130), VIEWS_TRIP)}


# ------------------------------------------------------------------------------------------------ problems
def _syn():
    from realsensecalibration_amd import synthetic as syn
    return syn


def thin(prob, views, seed):
    """prob (every point seen by prob['k'] cameras, observations sorted by point, then camera) with point j keeping views[j % len(views)]
    of its observations, chosen by a seeded generator."""
    P, k = prob["P"], prob["k"]
    assert prob["N"] == P * k and max(views) <= k
    want = np.asarray(views)[np.arange(P) % len(views)]
    rank = np.argsort(np.argsort(np.random.default_rng([seed, 0x7415]).random((P, k)), axis=1), axis=1)
    keep = (rank < want[:, None]).ravel()
    out = dict(prob)
    out["cam_idx"] = np.ascontiguousarray(prob["cam_idx"][keep])
    out["pt_idx"] = np.ascontiguousarray(prob["pt_idx"][keep])
    out["obs"] = np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1))
    out["N"] = int(keep.sum())
    out["views"] = want
    return out


def view_histogram(prob):
    return np.bincount(np.bincount(prob["pt_idx"], minlength=prob["P"]))


def expected_histogram(P, views):
    h = np.zeros(max(views) + 1, int)
    for j, v in enumerate(views):
        h[v] += len(range(j, P, len(views)))
    return h


def in_the_frame_of_camera(prob, c0):
    """The same problem in camera c0's initial orientation (X' = R0 X, R' = R R0'): camera c0's angle-axis vector is exactly zero,
    AngleAxisRotatePoint's first-order branch."""
    syn = _syn()
    C = prob["C"]
    par = prob["params"].copy()
    cams = par[:6 * C].reshape(C, 6)
    R = syn._matrix_from_rotvec(cams[:, :3])
    cams[:, :3] = syn._rotvec_from_matrix(R @ R[c0].T)
    cams[c0, :3] = 0.0
    par[6 * C:] = (par[6 * C:].reshape(-1, 3) @ R[c0].T).reshape(-1)
    return dict(prob, params=par)


_PROBLEMS = {}


def problem(shape, outliers=False, views=None, zero_cam=None):
    """The thinned problem of a shape, built once."""
    key = (shape, outliers, views, zero_cam)
    if key not in _PROBLEMS:
        C, P, cyc = SHAPES[shape]
        cyc = views or cyc
        seed = 700 + C
        p = thin(_syn().make_problem(C, P, max(cyc), seed=seed, outlier_frac=0.05 if outliers else 0.0), cyc, seed)
        assert np.array_equal(view_histogram(p), expected_histogram(P, cyc)), (view_histogram(p), expected_histogram(P, cyc))
        if zero_cam is not None:
            p = in_the_frame_of_camera(p, zero_cam)
            assert np.all(p["params"][6 * zero_cam:6 * zero_cam + 3] == 0.0)
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ cases
# perturb: sigma of a seeded perturbation of the start (perturbed_start); 0: the problem's own start, bit for bit
Case = namedtuple("Case", "name shape huber const zero radius views perturb", defaults=(0.0,))
ZERO_CAM = 3


def _case(shape, tag="", huber=0.0, const=False, zero=False, radius=1e4, views=None, perturb=0.0):
    return Case(shape + ("_" + tag if tag else ""), shape, huber, const, zero, radius, views, perturb)


def _cases():
    out = []
    for sh in ("v64", "v128", "v256"):
        out += [_case(sh), _case(sh, "huber", huber=HUBER), _case(sh, "const", const=True), _case(sh, "zero", zero=True)]
    # (radius 1e12: a one-view block is held by the damping alone, kappa ~ radius, and its rows' bar would be vacuous)
    out += [_case("v64", "r2.5", radius=2.5), _case("v64", "r1e12", radius=1e12, views=tuple(v for v in VIEWS_64 if v != 1))]
    out += [_case("trip64"), _case("trip128", "huber", huber=HUBER), _case("trip256", "huber", huber=HUBER)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# (environment, schur_impl, case names): one child process each (RSBA_* is read once per process)
SETTINGS = [
    ({}, 1, [c.name for c in CASES if c.shape in ("v64", "v128")]),
    ({}, 1, [c.name for c in CASES if c.shape == "v256"]),
    ({}, 1, ["trip64"]), ({}, 1, ["trip128_huber"]), ({}, 1, ["trip256_huber"]),
    ({"RSBA_BACKSUB_PROJ": "0"}, 1, ["v64", "v64_huber", "v256", "v256_huber"]),
    ({}, 0, ["v64", "v256"]),
    ({"RSBA_FUSED_LIN": "0"}, 1, ["v64"]),
    ({"RSBA_DECIDED_DAMP": "0"}, 1, ["v64"]),
    ({"RSBA_FIRST_STAGED": "0"}, 1, ["v64"]),
    ({"RSBA_PIPELINE": "0"}, 1, ["v64"]),
    ({"RSBA_FORCE_COMM": "1"}, 1, ["v64", "v256"]),
    ({"RSBA_FORCE_COMM": "1", "RSBA_BACKSUB_PROJ": "0"}, 1, ["v64"]),
]


def perturbed_start(prob, sigma):
    """prob with its start moved away from the minimum: a seeded normal of scale sigma on translations and points, 0.2 sigma on
    rotations (the stock starts are so close that every step's relative decrease is 1.0001 whatever the radius)."""
    C = prob["C"]
    par = np.asarray(prob["params"], float).copy()
    rng = np.random.default_rng([911, C])
    cams = par[:6 * C].reshape(C, 6)
    cams[:, :3] += 0.2 * sigma * rng.normal(size=(C, 3))
    cams[:, 3:] += sigma * rng.normal(size=(C, 3))
    par[6 * C:] += sigma * rng.normal(size=par.size - 6 * C)
    return dict(prob, params=par)


def case_problem(case):
    C = SHAPES[case.shape][0]
    assert ZERO_CAM not in (0, C - 1)
    p = problem(case.shape, case.huber > 0.0, case.views, ZERO_CAM if case.zero else None)
    return perturbed_start(p, case.perturb) if case.perturb else p


def constants(case, prob):
    """(constant cameras, constant points) of the case."""
    return ((0, prob["C"] - 1), (5, 70, prob["P"] - 1)) if case.const else ((), ())


def model(case):
    prob = case_problem(case)
    cc, cp = constants(case, prob)
    return PointModel(prob, case.huber, cc, cp)


def expected_form(case, env, impl):
    """The form of the point back-substitution PlanStep (csrc/ba_step_plan.hpp) picks; tests/test_step_plan_host.py holds the rule.
    The kernel statistics name all forms alike, so this is stated, not observed."""
    C = SHAPES[case.shape][0]
    on = lambda k: env.get(k, "1") != "0"   # noqa: E731
    fused = impl != 0 and on("RSBA_FUSED_LIN")
    if fused and on("RSBA_BACKSUB_PROJ") and C <= 256:
        pad = 64 if C <= 64 else (128 if C <= 128 else 256)
        loss = case.huber > 0.0
        reg, lds = {64: ((10, 10), (9, 11)), 128: ((10, 6), (9, 7)), 256: ((10, 10), (10, 10))}[pad][1 if loss else 0]
        return "proj<%d,%d+%d%s>%s" % (pad, reg, lds, ",loss" if loss else "", "" if on("RSBA_DECIDED_DAMP") else " host-damped")
    form = "staged" if C * BACKSUB_LDS_PER_CAMERA <= 60 * 1024 else "plain"
    return form + (" fused" if fused else " not fused")


def _tag_free(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items()))


def slices(P):
    return (P + 63) // 64


# ------------------------------------------------------------------------------------------------ the reference rows
class PointModel:
    """The point model's corrected rows per observation, by complex step."""

    def __init__(self, prob, huber=0.0, const_cams=(), const_pts=()):
        self.prob, self.huber = prob, float(huber)
        self.C, self.P, self.N = prob["C"], prob["P"], prob["N"]
        self.ci, self.pi = np.asarray(prob["cam_idx"], np.int64), np.asarray(prob["pt_idx"], np.int64)
        assert np.all(np.diff(self.pi) >= 0) and np.unique(self.pi * self.C + self.ci).size == self.N   # sorted by point; a pair once
        self.views = np.bincount(self.pi, minlength=self.P)
        self.start = np.concatenate([[0], np.cumsum(self.views)])[:-1]
        self.cam_obs = np.bincount(self.ci, minlength=self.C)
        self.cam_free = np.ones(self.C, bool)
        self.cam_free[list(const_cams)] = False
        self.pt_const = np.zeros(self.P, bool)
        self.pt_const[list(const_pts)] = True
        self.pt_free = ~self.pt_const & (self.views > 0)
        self.cam_free &= self.cam_obs > 0
        self.nc, self.n = 6 * self.C, 6 * self.C + 3 * self.P
        self.free = np.concatenate([np.repeat(self.cam_free, 6), np.repeat(self.pt_free, 3)])
        self.n_free = int(self.free.sum())
        self.x0 = np.asarray(prob["params"], float).copy()
        # m: 2 x the most observations that name one free block
        self.m = 2 * int(max(self.cam_obs[self.cam_free].max(initial=0), self.views[self.pt_free].max(initial=0)))
        # free cameras that see a point, free points a camera sees (the lengths of the bar's chains)
        self.free_views = np.bincount(self.pi, weights=self.cam_free[self.ci].astype(float), minlength=self.P).astype(int)
        self.free_pts = np.bincount(self.ci, weights=self.pt_free[self.pi].astype(float), minlength=self.C).astype(int)

    def raw(self, x):
        """r (N, 2), Jc (N, 2, 6), Jp (N, 2, 3) at x, uncorrected."""
        C, N = self.C, self.N
        x = np.asarray(x, float)
        r = rp.residuals(x.astype(complex), self.prob).real.reshape(N, 2)
        Jc, Jp = np.zeros((N, 2, 6)), np.zeros((N, 2, 3))
        for d in range(6):
            xx = x.astype(complex)
            xx[d:6 * C:6] += 1j * H_STEP
            Jc[:, :, d] = rp.residuals(xx, self.prob).imag.reshape(N, 2) / H_STEP
        for d in range(3):
            xx = x.astype(complex)
            xx[6 * C + d::3] += 1j * H_STEP
            Jp[:, :, d] = rp.residuals(xx, self.prob).imag.reshape(N, 2) / H_STEP
        return r, Jc, Jp

    def cost(self, x):
        r = rp.residuals(np.asarray(x, float).astype(complex), self.prob).real.reshape(self.N, 2)
        rho, _ = marker_loss_ref.rho_and_rho1(np.sum(r * r, axis=1), "huber" if self.huber > 0 else "none", self.huber)
        return 0.5 * float(np.sum(rho.astype(LD)))

    def linearise(self, x):
        """cost, r~ (N, 2), Jc~ (N, 2, 6), Jp~ (N, 2, 3) (the blocks of constant cameras / points zero), |r|^2 per observation."""
        r, Jc, Jp = self.raw(x)
        s = np.sum(r * r, axis=1)
        rho, rho1 = marker_loss_ref.rho_and_rho1(s, "huber" if self.huber > 0 else "none", self.huber)
        sq = np.sqrt(rho1)
        Jc = Jc * (sq * self.cam_free[self.ci])[:, None, None]
        Jp = Jp * (sq * self.pt_free[self.pi])[:, None, None]
        return 0.5 * float(np.sum(rho.astype(LD))), r * sq[:, None], Jc, Jp, s


def _scatter(idx, vals, size):
    out = np.zeros((size,) + vals.shape[1:], vals.dtype)
    np.add.at(out, idx, vals)
    return out


Reduced = namedtuple("Reduced", "S rhs Vinv Ws sc sp bp rows kappa_p")


class System:
    """The full damped normal equations at x, matrix-free, with the per-row bar.  scale: (s_c (C, 6), s_p (P, 3)) of iteration 0, or
    None to take it here (x is iteration 0's state)."""

    def __init__(self, mdl, x, radius, scale=None, min_lm=MIN_LM, max_lm=MAX_LM):
        assert sa.longdouble_ok()
        self.mdl, self.x, self.radius = mdl, np.asarray(x, float).copy(), float(radius)
        C, P, ci, pi = mdl.C, mdl.P, mdl.ci, mdl.pi
        self.cost, self.r, self.Jc, self.Jp, self.sumsq = mdl.linearise(self.x)
        self.rl, self.Jcl, self.Jpl = self.r.astype(LD), self.Jc.astype(LD), self.Jp.astype(LD)
        dHc = _scatter(ci, np.sum(self.Jcl * self.Jcl, axis=1), C)
        dHp = _scatter(pi, np.sum(self.Jpl * self.Jpl, axis=1), P)
        self.diagH = np.concatenate([dHc.ravel(), dHp.ravel()])
        self.g = np.concatenate([_scatter(ci, np.einsum("nra,nr->na", self.Jcl, self.rl), C).ravel(),
                                 _scatter(pi, np.einsum("nra,nr->na", self.Jpl, self.rl), P).ravel()])
        d64 = self.diagH.astype(np.float64)
        self.s = 1.0 / (1.0 + np.sqrt(d64)) if scale is None else np.asarray(scale, float).copy()
        self.D = np.clip(d64 * self.s ** 2, min_lm, max_lm) / self.radius
        self.damp = (self.D / self.s ** 2).astype(LD)
        self.diagA = self.diagH + self.damp
        self.b = -self.g
        free = mdl.free
        self.gmax = float(np.abs(self.g[free]).max())
        self._d = np.sqrt(self.diagA)
        # |A| from A's own blocks, for the recovery term
        self._Uabs = np.abs(_scatter(ci, np.einsum("nra,nrb->nab", self.Jc, self.Jc), C)) + 0.0
        self._Vabs = np.abs(_scatter(pi, np.einsum("nra,nrb->nab", self.Jp, self.Jp), P))
        self._Wabs = np.abs(np.einsum("nra,nrb->nab", self.Jc, self.Jp))
        # conditioning of what the kernels invert explicitly, in Jacobi-scaled coordinates, from the host's own elimination
        red = self.reduced()
        self.kappa_s = float(sa.diag_block_kappas(red.S[np.ix_(red.rows, red.rows)]).max()) if red.rows.size else 0.0
        self.kappa_p = red.kappa_p
        self.kappa_pmax = float(self.kappa_p[mdl.pt_free].max(initial=0.0))
        gf = sa.gamma(mdl.m + 2 * C_JAC)
        self.forming = gf / (1.0 - gf)
        G = lambda n: sa.gamma(3 * n + 1) / (1.0 - sa.gamma(n + 1))   # noqa: E731
        kappa_seen = np.zeros(C)   # the largest kappa of a free point's block among the points a camera sees
        np.maximum.at(kappa_seen, ci, np.where(mdl.pt_free[pi], self.kappa_p[pi], 0.0))
        solve_c = G(6 * int(mdl.cam_free.sum())) * (1.0 + self.kappa_s) + G(3) * (1.0 + kappa_seen) + sa.gamma(3 * mdl.free_pts)
        solve_p = G(3 + 6 * mdl.free_views) * (1.0 + self.kappa_p)
        self.solve = np.concatenate([np.repeat(solve_c, 6), np.repeat(solve_p, 3)])

    # ---- A
    def apply(self, d):
        """A d in np.longdouble (d over all 6 C + 3 P parameters; the rows of blocks outside the system are only damped)."""
        mdl = self.mdl
        d = np.asarray(d, LD)
        dc, dp = d[:mdl.nc].reshape(-1, 6), d[mdl.nc:].reshape(-1, 3)
        Jd = np.einsum("nra,na->nr", self.Jcl, dc[mdl.ci]) + np.einsum("nra,na->nr", self.Jpl, dp[mdl.pi])
        out = np.concatenate([_scatter(mdl.ci, np.einsum("nra,nr->na", self.Jcl, Jd), mdl.C).ravel(),
                              _scatter(mdl.pi, np.einsum("nra,nr->na", self.Jpl, Jd), mdl.P).ravel()])
        return out + self.damp * d, Jd

    def abs_apply(self, v):
        mdl = self.mdl
        vc, vp = v[:mdl.nc].reshape(-1, 6), v[mdl.nc:].reshape(-1, 3)
        oc = np.einsum("cab,cb->ca", self._Uabs, vc) + _scatter(mdl.ci, np.einsum("nab,nb->na", self._Wabs, vp[mdl.pi]), mdl.C)
        op = np.einsum("pab,pb->pa", self._Vabs, vp) + _scatter(mdl.pi, np.einsum("nab,na->nb", self._Wabs, vc[mdl.ci]), mdl.P)
        return np.concatenate([oc.ravel(), op.ravel()]) + self.damp.astype(float) * v

    def delta(self, x1):
        """x1 - x over all parameters, exact."""
        return np.asarray(x1, LD) - self.x.astype(LD)

    # ---- the measure
    def check(self, x1):
        """Row-wise eta and bar of the step that led to x1: a dict per row class ('cam', 'pt') with eta, bar, ratio, recovery at the
        row of the largest eta / bar, that row's description, eta_max; 'bar_max' the largest bar of any free row."""
        mdl = self.mdl
        free = mdl.free
        d = self.delta(x1)
        assert not np.any(d[~free] != 0), "a block outside the system moved"
        Ad, _ = self.apply(d)
        res = np.abs(self.b - Ad)
        den = self._d * np.sum((self._d * np.abs(d))[free]) + np.abs(self.b)
        eta = (res / np.where(den > 0, den, 1)).astype(np.float64)
        rec = self.abs_apply(U * np.abs(np.asarray(x1, float))) / np.where(den > 0, den, 1).astype(np.float64)
        bar = self.forming + self.solve + rec + 4 * U
        out = {"bar_max": float(bar[free].max())}
        for cls, sel in (("cam", np.arange(mdl.n) < mdl.nc), ("pt", np.arange(mdl.n) >= mdl.nc)):
            idx = np.flatnonzero(free & sel)
            if not idx.size:
                out[cls] = dict(eta=0.0, bar=1.0, ratio=0.0, recovery=0.0, eta_max=0.0, bar_max=0.0, row="none")
                continue
            i = int(idx[np.argmax(eta[idx] / bar[idx])])
            out[cls] = dict(eta=float(eta[i]), bar=float(bar[i]), ratio=float(eta[i] / bar[i]), recovery=float(rec[i]),
                            eta_max=float(eta[idx].max()), bar_max=float(bar[idx].max()), row=self.describe(i))
        out["ratio"] = max(out["cam"]["ratio"], out["pt"]["ratio"])
        return out

    def describe(self, i):
        mdl = self.mdl
        if i < mdl.nc:
            return "camera %d component %d (%d observations)" % (i // 6, i % 6, mdl.cam_obs[i // 6])
        j = (i - mdl.nc) // 3
        return "point %d component %d (%d views, slice %d lane %d, kappa %.3g)" % (j, (i - mdl.nc) % 3, mdl.views[j], j // 64, j % 64, self.kappa_p[j])

    # ---- the scalars
    def step_norm_tolerance(self, x1):
        d = self.delta(x1)
        nd = float(np.sqrt(np.sum(d * d)))
        return nd, 4 * U * np.sqrt(self.mdl.n_free) * nd + U * float(np.linalg.norm(np.asarray(x1, float)[self.mdl.free]))

    def model_cost_change(self, x1):
        """The reference's model cost change at the step that led to x1, and its tolerance."""
        d = self.delta(x1)
        Ad, Jd = self.apply(d)
        mcc = -float(np.sum(Jd * (self.rl + 0.5 * Jd)))
        slope = np.abs(self.g + (Ad - self.damp * d))
        return mcc, 1e-11 * abs(mcc) + float(np.sum(slope * U * np.abs(np.asarray(x1, LD))))

    # ---- the reference's own fp64 step: Schur complement, Cholesky, points back-substituted with explicit 3 x 3 inverses
    def reduced(self):
        mdl = self.mdl
        C, P, ci, pi = mdl.C, mdl.P, mdl.ci, mdl.pi
        sc, sp = self.s[:mdl.nc].reshape(C, 6), self.s[mdl.nc:].reshape(P, 3)
        Dc, Dp = self.D[:mdl.nc].reshape(C, 6), self.D[mdl.nc:].reshape(P, 3)
        Us = _scatter(ci, np.einsum("nra,nrb->nab", self.Jc, self.Jc), C) * sc[:, :, None] * sc[:, None, :]
        Vs = _scatter(pi, np.einsum("nra,nrb->nab", self.Jp, self.Jp), P) * sp[:, :, None] * sp[:, None, :]
        Ws = np.einsum("nra,nrb->nab", self.Jc, self.Jp) * sc[ci][:, :, None] * sp[pi][:, None, :]
        bc = sc * _scatter(ci, np.einsum("nra,nr->na", self.Jc, self.r), C)
        bp = sp * _scatter(pi, np.einsum("nra,nr->na", self.Jp, self.r), P)
        Vd = Vs + Dp[:, :, None] * np.eye(3)[None]
        Vinv = np.linalg.inv(Vd)
        kappa_p = np.abs(Vd).sum(axis=2).max(axis=1) * np.abs(Vinv).sum(axis=2).max(axis=1)
        S4 = np.zeros((C, C, 6, 6))
        S4[np.arange(C), np.arange(C)] = Us + Dc[:, :, None] * np.eye(6)[None]
        for k in np.unique(mdl.views[mdl.views > 0]):
            pts = np.flatnonzero(mdl.views == k)
            for lo in range(0, pts.size, 16384):
                q = pts[lo:lo + 16384]
                idx = mdl.start[q][:, None] + np.arange(k)[None, :]
                Wk = Ws[idx]
                T = np.einsum("pkab,pbc->pkac", Wk, Vinv[q])
                cams = ci[idx]
                np.subtract.at(S4, (cams[:, :, None], cams[:, None, :]), np.einsum("pkac,plec->pklae", T, Wk))
        S = S4.transpose(0, 2, 1, 3).reshape(6 * C, 6 * C)
        rhs = bc - _scatter(ci, np.einsum("nab,nbc,nc->na", Ws, Vinv[pi], bp[pi]), C)
        rows = np.flatnonzero(np.repeat(mdl.cam_free, 6))
        return Reduced(S, rhs.ravel(), Vinv, Ws, sc, sp, bp, rows, kappa_p)

    def reference_step(self, mutation=None, stale=None):
        """delta (all parameters) of the numpy Schur-complement step.  mutation: None | 'drop_view' (one observation left out of a
        21-view point's W_j' dc sum) | 'inverse_entry' (one entry of one point's (V_j + D_j)^-1 off by 1e-9 relative) | 'neighbour_gp'
        (one point back-substituted with its neighbour's g_p) | 'stale_point' (one point's kept g_p that of the System `stale`, an
        earlier state: what a back-substitution that leaves part of one record unwritten does to the next step)."""
        mdl = self.mdl
        red = self.reduced()
        Vinv, bp = red.Vinv, red.bp
        if mutation == "stale_point":
            j = int(np.flatnonzero(mdl.pt_free & (mdl.views == 21))[0])
            old = stale.reduced()
            bp = bp.copy()
            bp[j] = old.bp[j]
            red = _Mutated(self, red._replace(bp=bp))
        if mutation == "inverse_entry":
            j = int(np.flatnonzero(mdl.pt_free & (mdl.views == 2))[0])
            Vinv = Vinv.copy()
            Vinv[j, 0, 0] *= 1.0 + 1e-9
            red = _Mutated(self, red._replace(Vinv=Vinv))   # (the kernels keep one copy of the inverse: S and rhs are formed with it too)
        yc = np.zeros(mdl.nc)
        if red.rows.size:
            L = np.linalg.cholesky(red.S[np.ix_(red.rows, red.rows)])
            yc[red.rows] = np.linalg.solve(L.T, np.linalg.solve(L, red.rhs[red.rows]))
        terms = np.einsum("nab,na->nb", red.Ws, yc.reshape(-1, 6)[mdl.ci])
        if mutation == "drop_view":
            j = int(np.flatnonzero(mdl.pt_free & (mdl.views == 21))[0])
            terms[mdl.start[j] + 7] = 0.0
        if mutation == "neighbour_gp":
            j = int(np.flatnonzero(mdl.pt_free & (mdl.views == 21))[0])
            bp = bp.copy()
            bp[j] = red.sp[j] * (bp[j + 1] / red.sp[j + 1])
        yp = np.einsum("pab,pb->pa", red.Vinv, bp - _scatter(mdl.pi, terms, mdl.P))
        delta = np.concatenate([(-red.sc * yc.reshape(-1, 6)).ravel(), (-red.sp * yp).ravel()])
        delta[~mdl.free] = 0.0
        return delta


def _Mutated(sysm, red):
    """red with S and rhs formed again from red.Vinv (the other fields unchanged)."""
    mdl = sysm.mdl
    C, ci, pi = mdl.C, mdl.ci, mdl.pi
    Dc = sysm.D[:mdl.nc].reshape(C, 6)
    Us = _scatter(ci, np.einsum("nra,nrb->nab", sysm.Jc, sysm.Jc), C) * red.sc[:, :, None] * red.sc[:, None, :]
    S4 = np.zeros((C, C, 6, 6))
    S4[np.arange(C), np.arange(C)] = Us + Dc[:, :, None] * np.eye(6)[None]
    for k in np.unique(mdl.views[mdl.views > 0]):
        q = np.flatnonzero(mdl.views == k)
        idx = mdl.start[q][:, None] + np.arange(k)[None, :]
        Wk = red.Ws[idx]
        T = np.einsum("pkab,pbc->pkac", Wk, red.Vinv[q])
        cams = ci[idx]
        np.subtract.at(S4, (cams[:, :, None], cams[:, None, :]), np.einsum("pkac,plec->pklae", T, Wk))
    bc = red.sc * _scatter(ci, np.einsum("nra,nr->na", sysm.Jc, sysm.r), C)
    rhs = bc - _scatter(ci, np.einsum("nab,nbc,nc->na", red.Ws, red.Vinv[pi], red.bp[pi]), C)
    return red._replace(S=S4.transpose(0, 2, 1, 3).reshape(6 * C, 6 * C), rhs=rhs.ravel())


# ------------------------------------------------------------------------------------------------ the scalars of a log row
def scalar_checks(sysm, x1, cost0, gmax0, cost_change, step_norm, rel, label):
    """[(what, ok, detail)] of one step's scalars: sysm the system the step was taken from, x1 where it led; cost0 / gmax0 the log's
    values at sysm.x, cost_change / step_norm / rel the step's row."""
    mdl = sysm.mdl
    nd, tol = sysm.step_norm_tolerance(x1)
    mcc, mcc_tol = sysm.model_cost_change(x1)
    cand_ref = mdl.cost(x1)
    cand = cost0 - cost_change
    fig = dict(cost=abs(cost0 - sysm.cost) / sysm.cost, gmax=abs(gmax0 - sysm.gmax) / sysm.gmax, step_norm=abs(step_norm - nd) / nd,
               step_norm_tol=tol / nd, mcc=abs(cost_change / rel - mcc) / abs(mcc), mcc_tol=mcc_tol / abs(mcc), candidate=abs(cand - cand_ref) / cand_ref)
    checks = [
        (label + " cost", abs(cost0 - sysm.cost) <= 1e-12 * sysm.cost, (cost0, sysm.cost)),
        (label + " gradient_max_norm", abs(gmax0 - sysm.gmax) <= 1e-11 * sysm.gmax, (gmax0, sysm.gmax)),
        (label + " step_norm", abs(step_norm - nd) <= tol, (step_norm, nd, tol)),
        (label + " model cost change", abs(cost_change / rel - mcc) <= mcc_tol + 2 * U * abs(mcc), (cost_change / rel, mcc, mcc_tol)),
        (label + " candidate cost", abs(cand - cand_ref) <= 1e-12 * cand_ref + U * (abs(cost_change) + cand_ref), (cand, cand_ref)),
    ]
    return checks, fig
