"""One LM step of the marker-chain model as a linear solve: its backward error, and the bar any correct fp64 step meets (host code).

What is measured.  A capi.Solver run with max_num_iterations = 1 and the three tolerances at -1 takes exactly one step; with the
step accepted the downloaded parameters are x1 = fl(x0 + delta), so delta = x1 - x0 over the free blocks is observable through the
public API, whichever kernels formed it: the split elimination (csrc/ba_marker_split.hpp), k_time_eliminate and the reduced solves
(ba_marker_schur.hpp) or the dense one-workgroup solver (ba_marker_kernels.hpp).  delta must solve the FULL damped normal equations

    A delta = b,     A = H + diag(D / s^2),   b = -g,   H = J~'J~,   g = J~'r~       (J~, r~: the corrected rows)
    s = 1 / (1 + sqrt(diag H)),   D = clip(diag(H) s^2, min_lm_diagonal, max_lm_diagonal) / radius

which are built here from tests/marker_loss_ref.py (complex-step Jacobians, no code shared with the product), H and g summed in
np.longdouble.  Eliminating the time blocks, Jacobi scaling and the order of the sums are ways of solving this one system.

Measure (Oettli-Prager, componentwise in the metric of A's own diagonal; solve_accuracy.backward_errors), per free row i:

    eta_i = |b_i - sum_j A_ij delta_j| / ( sqrt(A_ii) sum_j sqrt(A_jj) |delta_j| + |b_i| )

eta_i is the smallest epsilon with (A + dA) delta = b + db, |dA_ij| <= epsilon sqrt(A_ii A_jj), |db_i| <= epsilon |b_i|.  The metric
is invariant under a diagonal scaling of the unknowns, so the few ulps between the device's Jacobi scale and this file's do not
enter (they move D by a few ulps of a term that is 1 / radius of the diagonal).

Bar.  Per row, the sum of four terms (u = 2^-53, gamma_k = k u / (1 - k u)); nothing in it is fitted to a measurement.

 1. Forming A and b:  gamma_{m+2c} / (1 - gamma_{m+2c}).  An entry of A is a sum of products J~_ra J~_rb over the residual rows r that
    meet in both blocks; m is the longest such sum of the case: 8 rows x the largest number of residual blocks that name one free
    parameter block (block_rows, from the index arrays; the chunks' partial sums and their reduction only reorder it).  Every factor
    J~_ra carries the roundings of the analytic chain rule (MarkerCornerResidualJacobian, ba_math.hpp) along its longest path, a
    rotation column of the marker block: c = 37, counted step by step in tests/test_gpu_jacobian.py's docstring (pose constants 10,
    three rigid transforms 12, iz / al / ga 4, Q_t 2, Q_m 3, w x Q_m 2, the product with Jl 3, the corrector's product 1).  A product
    has two factors, hence 2c (its own rounding is the first of the m).  The count treats a rounding as a relative perturbation
    of the entry it feeds (first order, as gamma_k does).  By Cauchy-Schwarz over the rows |dA_ij| <= gamma sqrt(A_ii A_jj), and
    |db_i| <= gamma sqrt(A_ii) |r~|, which the measure's denominator absorbs at the same order (|r~| changes by J~ delta over the step).
 2. Elimination and solve: eliminating the time blocks and factoring the reduced system is a block Cholesky factorisation of A as a
    whole, n = all free parameters: (A + dA) delta = b with |dA_ij| <= gamma_{3n+1} / (1 - gamma_{n+1}) sqrt(A_ii A_jj) (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 / 10.4, as in solve_accuracy.py).  The kernels replace
    substitutions with products by explicit inverses of triangular blocks: M_t = L_t^-1 of the 6 x 6 factor of V_t + D_t
    (InvertSpd6Lanes, E_t = M_t'M_t) and T_k = L_kk^-1 of the 32-wide diagonal blocks of the reduced (dense path: the whole) system's
    factor (DiagFactorInverse).  Each stretches the terms that run through it by at most (1 + kappa_inf) of that block (Higham sec.
    14.2); the bar takes the largest over all of them, in Jacobi-scaled coordinates, from the host's own factorisation
    (solve_accuracy.diag_block_kappas on the host's Schur complement):   gamma_{3n+1} / (1 - gamma_{n+1}) (1 + max kappa_inf).
 3. Recovery: delta is known only as x1 - x0 (exact in np.longdouble) with x1 = fl(x0 + delta), an error of at most u |x1_i| per
    component, which moves row i's residual by at most (|A| u |x1|)_i: that over the row's denominator is added, per row.  Where
    the step is small against the parameters (the second state, near the solution) this term leads the bar, and says so.
 4. 4 u for the candidate's own addition and the negation / scaling delta = -s y in front of it.

What the measure sees: a wrong entry of relative size d in one time's W_t or (V_t + D_t)^-1 changes eta by about d times that time's
share of sum sqrt(A_jj) |delta_j| — tests/test_marker_step_accuracy_cpu.py holds three such mutations above the bar, and both numpy
references' own fp64 steps below it, on every shape listed here.

The log row's scalars (each tolerance is a count of roundings or one of test_reduced_system_and_step_match_oracle's stage bars):
    cost (iteration 0)            reference cost, 1e-12 relative
    gradient_max_norm (it. 0)     max |g|, 1e-11 relative
    step_norm                     |delta|, 4 u sqrt(n) relative (n squares summed in trees and short runs, then a square root) plus the
                                  recovery term |u x1| / |delta|
    cost_change / relative_decrease   the model cost change (two roundings: the subtraction and the division) against
                                  MarkerChain.model_cost_change(r~, J~, delta) at the DEVICE's delta (no solve error enters), 1e-11
                                  relative plus the recovery term |(g + H delta)' u x1| / model cost change
    cost - cost_change            the candidate cost against the reference's cost at the downloaded x1: 1e-12 relative plus
                                  u (|cost_change| + candidate) / candidate for the subtraction in the log and the one that undoes it
The iteration-1 row's own cost is re-evaluated at x1 by the library and is held to the reference at 1e-12 as well.
"""
from collections import namedtuple

import numpy as np

import marker_loss_ref as ref
import solve_accuracy as sa

U = sa.U
C_JAC = 37                  # roundings behind one corrected Jacobian entry (tests/test_gpu_jacobian.py's count)
MIN_LM, MAX_LM = 1e-6, 1e32   # rsba_options_default
MT_TILE, MT_MAXD, SP_LDS, MRS_MAXP = 32, 1020, 65, 5   # csrc/ba_marker_plan.hpp: RSBA_MT_TILE, RSBA_MT_MAXD, RSBA_SP_LDS, RSBA_MRS_MAXP
CHOL_MAXN, PB, PLD = 384, 32, 33                       # csrc/ba_schur_plan.hpp: RSBA_CHOL_MAXN, RSBA_PB, RSBA_PLD
LDS_CAP = 156 * 1024                                   # RSBA_LDS_CAP
LOSS_A = 40.0   # px: about the median |r| of a residual block at the jittered start, so that the loss's two branches both occur in one step


# ------------------------------------------------------------------------------------------------ problems
def _syn():
    from realsensecalibration_amd import synthetic as syn
    return syn


def full_visibility(prob, seed, noise_px=0.3):
    """prob with every (time, camera, marker) observed: the corners projected at the truth (MarkerChain's own projection) plus noise."""
    C, T, M = prob["C"], prob["T"], prob["M"]
    t, c, m = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(T), np.arange(C), np.arange(M), indexing="ij"))
    out = dict(prob, N=t.size, t=t, c=c, m=m, obs=np.zeros((t.size, 8)))
    proj = ref.MarkerChain(dict(out, params=prob["truth"]), 0).residuals(np.asarray(prob["truth"], float).reshape(-1, 6))
    out["obs"] = proj + np.random.default_rng([seed, 0x51]).normal(0.0, noise_px, proj.shape)
    return out


def _keep_rows(prob, keep):
    keep = np.asarray(keep, bool)
    return dict(prob, N=int(keep.sum()), t=prob["t"][keep], c=prob["c"][keep], m=prob["m"][keep], obs=np.asarray(prob["obs"])[keep])


def rows_per_shot():
    """6 x 8 x 6 with observations removed: shots of 36, 33, 32, 31, 1 and 1 residual blocks (RSBA_MT_TILE = 32: below, at and above
    a tile, a tile plus one, a tile plus a rest), shot 4 seen only by camera 0 through marker 0 (no reduced column), shot 5 a single
    residual whose camera (2, made constant by the case) is constant."""
    p = full_visibility(_syn().make_marker_chain(6, 8, 6, seed=20, keep=1.0), 20)
    t, c, m = p["t"], p["c"], p["m"]
    pair = 6 * c + m                                   # 0 .. 35 within a shot
    keep = np.ones(p["N"], bool)
    keep &= ~((t == 1) & (pair >= 33))
    keep &= ~((t == 2) & (pair >= 32))
    keep &= ~((t == 3) & (pair >= 31))
    keep &= ~((t == 4) & ~((c == 0) & (m == 0)))
    keep &= ~((t == 5) & ~((c == 2) & (m == 3)))
    p = _keep_rows(p, keep)
    assert [int((p["t"] == k).sum()) for k in range(8)] == [36, 33, 32, 31, 1, 1, 36, 36]
    return p


_PROBLEMS = {}


def problem(key):
    """The problem of a case, built once.  key: ('syn', C, T, M, keep) | ('full', C, T, M) | ('rows',) | ('hongo',) | ('test2',) |
    ('disp', key) (5 % of the corners 40 px off)."""
    if key not in _PROBLEMS:
        kind = key[0]
        if kind == "syn":
            _, C, T, M, keep = key
            p = _syn().make_marker_chain(C, T, M, seed=60 + C + T + M, keep=keep)
        elif kind == "full":
            _, C, T, M = key
            p = full_visibility(_syn().make_marker_chain(C, T, M, seed=60 + C + T + M, keep=1.0), C + T + M)
        elif kind == "rows":
            p = rows_per_shot()
        elif kind == "hongo":
            p = ref.hongo()
        elif kind == "test2":
            p = ref.test2()
        elif kind == "disp":
            base = problem(key[1])
            p = ref.displace_corners(base, 0.05, 40.0, base["C"] * base["T"] * base["M"])
        else:
            raise ValueError(key)
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ cases
# prob: the problem's key; variant 1: Test2's wiring (marker 0 free); impl: schur_impl (0 dense, 2 time-eliminating); const: 'one_each'
# (a camera, a time and a marker constant), 'cam2' or none; env: the switches; state 'second': the step taken from the solution
# perturbed by 1e-3; force: min_relative_decrease = -1e300 (the first step would be rejected at the default threshold; the CPU module
# checks the flag against the reference's relative decrease).
Case = namedtuple("Case", "name prob variant impl loss const env radius state force")


def _case(name, prob, variant=0, impl=2, loss="none", const="", env=None, radius=1e4, state="start", force=False):
    return Case(name, prob, variant, impl, loss, const, tuple(sorted((env or {}).items())), radius, state, force)


make_case = _case   # (public: tests/step_sequence.py builds its sequence cases on these)


def _cases():
    out = []
    S = lambda C, T, M, keep=0.9: ("syn", C, T, M, keep)   # noqa: E731
    # minimal: n_r = 12 on the chain variant; Test2's wiring frees marker 0 (n_r = 18)
    out += [_case("minimal_2x3x2", S(2, 3, 2, 1.0)), _case("minimal_2x3x2_test2", S(2, 3, 2, 1.0), variant=1)]
    out += [_case("rows_per_shot_6x8x6", ("rows",), const="cam2")]
    # reduced width at each hand-over (AccMfmaTiles: 45 tiles = 3 a wavefront at 144 columns, 55 = 4 -> the eight-tile kernel at 150; 120
    # = 8 at 240, 136 = 9 -> VALU at 246; the triangle in LDS up to 160 columns; one workgroup up to 384).  The accumulation's variants
    # and the two one-workgroup solves share a kernel-statistics name each: the expected one is computed from the thresholds (expected_path)
    for C, T, M, keep in ((13, 8, 13, 0.9), (13, 8, 14, 0.9), (21, 6, 21, 0.9), (21, 6, 22, 0.9), (14, 8, 14, 0.9), (14, 8, 15, 0.9),
                          (33, 6, 33, 0.5), (33, 6, 34, 0.5)):
        out.append(_case("width_%dx%dx%d" % (C, T, M), S(C, T, M, keep)))
    # wide shots: 118 blocks (split kernels, chunk sums in memory), 122 (k_time_eliminate), 96 residual blocks a shot (k_time_backsub_wg's
    # domain; the default back-substitution is the split one: the workgroup kernel itself runs in the switch cases below and here)
    out += [_case("wide_60x3x60", S(60, 3, 60, 1.0)), _case("wide_62x3x62", S(62, 3, 62, 1.0)),
            _case("wide_8x6x12", ("full", 8, 6, 12)),
            _case("wide_8x6x12_backsub_wg", ("full", 8, 6, 12), env={"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "1"})]
    switches = [{}, {"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SOLVE_LDS": "0"},
                {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "1"},
                {"RSBA_MT_CHUNKS": "1"}, {"RSBA_MT_CHUNKS": "7"}, {"RSBA_MT_CHUNKS": "1000"}]
    for shape in ((8, 24, 12), (3, 60, 4)):
        for env in switches:
            tag = ",".join("%s=%s" % (k[8:], v) for k, v in sorted(env.items())) or "default"
            out.append(_case("switch_%dx%dx%d_%s" % (shape + (tag,)), S(*shape), env=env))
    for shape in ((6, 8, 6), (8, 24, 12)):
        nm = "%dx%dx%d" % shape
        for loss in ("huber", "cauchy"):
            out.append(_case("loss_%s_%s" % (nm, loss), ("disp", S(*shape)), loss=loss))
        for loss in ("none", "huber"):
            out.append(_case("const_%s_%s" % (nm, loss), ("disp", S(*shape)), loss=loss, const="one_each"))
    for r in (2.5, 1e4, 1e12):
        out.append(_case("radius_8x24x12_%g" % r, S(8, 24, 12), radius=r))
    out += [_case("dense_4x40x6", S(4, 40, 6), impl=0), _case("dense_hongo", ("hongo",), impl=0), _case("dense_test2", ("test2",), variant=1, impl=0),
            _case("elim_hongo", ("hongo",)), _case("elim_test2", ("test2",), variant=1)]
    out += [_case("second_8x24x12", S(8, 24, 12), state="second"), _case("second_hongo", ("hongo",), state="second")]
    return out


CASES = _cases()


def shape_key(case):
    """What the numpy side of a case depends on: the switches and the path do not change the system."""
    return (case.prob, case.variant, case.loss, case.const, case.radius, case.state)


def constant_blocks(case, prob):
    C, T = prob["C"], prob["T"]
    return {"": (), "cam2": (2,), "one_each": (2, C + 5, C + T + 3)}[case.const]


def chain(case):
    prob = problem(case.prob)
    return ref.MarkerChain(prob, case.variant, case.loss, LOSS_A if case.loss != "none" else 0.0, constant_blocks(case, prob))


def perturbed(x, seed=7):
    """The second state: x times (1 + 1e-3 N(0, 1)) per component (fixed seed)."""
    return x * (1.0 + 1e-3 * np.random.default_rng(seed).normal(size=x.shape))


# ------------------------------------------------------------------------------------------------ the system and the bar
def block_rows(mc):
    """m: 8 x the largest number of residual blocks that name one free parameter block."""
    first = mc.cols[:, ::6]
    first = first[first >= 0] // 6
    return 8 * int(np.bincount(first).max()) if first.size else 0


def _longdouble_normal_equations(mc, rt, Jt):
    n = mc.n
    Jl, rl = Jt.astype(np.longdouble), rt.astype(np.longdouble)
    cl = np.where(mc.cols >= 0, mc.cols, n)
    Hx = np.zeros((n + 1, n + 1), np.longdouble)
    np.add.at(Hx, (cl[:, :, None], cl[:, None, :]), np.einsum("kra,krb->kab", Jl, Jl))
    gx = np.zeros(n + 1, np.longdouble)
    np.add.at(gx, cl, np.einsum("kra,kr->ka", Jl, rl))
    return Hx[:n, :n], gx[:n]


class System:
    """The full damped normal equations at x (the free blocks' vector), their conditioning and the bar's row-independent part.
    scale: the Jacobi scale s (n) of iteration 0, or None to take it here (x is iteration 0's state)."""

    def __init__(self, mc, x, radius, dense, min_lm=MIN_LM, max_lm=MAX_LM, scale=None):
        assert sa.longdouble_ok()
        self.mc, self.x, self.radius, self.n = mc, np.asarray(x, float).copy(), radius, mc.n
        self.cost, self.rt, self.Jt, H64, g64, _ = mc.linearise(self.x)
        self.H, self.g = _longdouble_normal_equations(mc, self.rt, self.Jt)
        dH = np.diagonal(self.H).astype(np.float64)
        self.s = 1.0 / (1.0 + np.sqrt(dH)) if scale is None else np.asarray(scale, float).copy()
        self.D = np.clip(dH * self.s ** 2, min_lm, max_lm) / radius
        self.A = self.H + np.diag((self.D / self.s ** 2).astype(np.longdouble))
        self.b = -self.g
        self.gmax = float(np.abs(self.g).max())
        self.m = block_rows(mc)
        # conditioning of the blocks the kernels invert explicitly, in Jacobi-scaled coordinates
        As = np.asarray(self.H, np.float64) * np.outer(self.s, self.s) + np.diag(self.D)
        C, T = mc.C, mc.T
        is_time = np.repeat((mc.free_blocks >= C) & (mc.free_blocks < C + T), 6)
        if dense:
            self.kappa_t, self.kappa_s = 0.0, float(sa.diag_block_kappas(As).max())
        else:
            ti, ri = np.flatnonzero(is_time), np.flatnonzero(~is_time)
            kt, S = [0.0], As[np.ix_(ri, ri)].copy()
            for k in range(0, ti.size, 6):
                q = ti[k:k + 6]
                kt.append(float(sa.diag_block_kappas(As[np.ix_(q, q)], 6).max()))
                W = As[np.ix_(q, ri)]
                S -= W.T @ np.linalg.solve(As[np.ix_(q, q)], W)
            self.kappa_t = max(kt)
            self.kappa_s = float(sa.diag_block_kappas(S).max()) if ri.size else 0.0
        self.kappa = max(self.kappa_t, self.kappa_s)
        gf = sa.gamma(self.m + 2 * C_JAC)
        self.forming = gf / (1.0 - gf)
        self.solve = sa.gamma(3 * self.n + 1) / (1.0 - sa.gamma(self.n + 1)) * (1.0 + self.kappa)
        self._d = np.sqrt(np.maximum(np.diagonal(self.A), 0))
        self._absA = np.abs(self.A)

    def delta(self, x1):
        """x1 - x over the free blocks, exact."""
        return np.asarray(x1, np.longdouble) - self.x.astype(np.longdouble)

    def check(self, x1):
        """Row-wise eta and bar of the step that led to x1 -> dict(eta, bar (their values in the row of the largest eta / bar), ratio,
        recovery (that row's recovery term))."""
        d = self.delta(x1)
        eta = sa.backward_errors(self.A, self.b, d)
        den = self._d * np.sum(self._d * np.abs(d)) + np.abs(self.b)
        rec = (self._absA @ (U * np.abs(np.asarray(x1, np.longdouble)))) / np.where(den > 0, den, 1)
        bar = self.forming + self.solve + rec.astype(np.float64) + 4 * U
        i = int(np.argmax(eta / bar))
        return dict(eta=float(eta[i]), bar=float(bar[i]), ratio=float(eta[i] / bar[i]), recovery=float(rec[i]), eta_max=float(eta.max()))

    def step_norm_tolerance(self, x1):
        d = self.delta(x1)
        nd = float(np.sqrt(np.sum(d * d)))
        return nd, 4 * U * np.sqrt(self.n) * nd + U * float(np.linalg.norm(np.asarray(x1, float)))

    def model_cost_change(self, x1):
        """The reference's model cost change at the step that led to x1, and its tolerance."""
        d = self.delta(x1)
        mcc = self.mc.model_cost_change(self.rt, self.Jt, d.astype(np.float64))
        slope = np.abs(self.g + self.H @ d)
        return mcc, 1e-11 * abs(mcc) + float(np.sum(slope * U * np.abs(np.asarray(x1, np.longdouble))))


# ------------------------------------------------------------------------------------------------ the path
def structure(mc):
    """n_r, dmax, pmax (free / all camera + marker blocks of the widest shot, in columns / blocks), the widest shot's residual blocks."""
    C, T = mc.C, mc.T
    free = set(int(b) for b in mc.free_blocks)
    nr = 6 * sum(1 for b in free if b < C or b >= C + T)
    dmax = pmax = widest = 0
    for t in range(T):
        sel = mc.t == t
        if not sel.any():
            continue
        blocks = {int(c) for c in mc.c[sel & mc.has_cam]} | {C + T + int(m) for m in mc.m[sel & mc.has_mar]}
        dmax = max(dmax, 6 * len(blocks & free))
        pmax = max(pmax, len(blocks))
        widest = max(widest, int(sel.sum()))
    return nr, dmax, pmax, widest


def _marker_solve_lds_doubles(nr):
    np_ = (nr + PB - 1) // PB
    npad = PB * np_
    rows = sum(npad + 1 - PB * p for p in range(np_))
    return rows * PLD + 2 * PB * PLD + PB + 2 * npad


def _acc_lds_bytes(dmax, s_doubles):
    smax = dmax // 6
    return (2 * smax * SP_LDS + 6 * dmax + 96 + s_doubles) * 8 + 2 * ((smax + 2) & ~1) * 4


def expected_path(case, mc, subset=False, priors=False):
    """What PlanMarkerChain decides for the case (csrc/ba_marker_plan.hpp; tests/test_marker_plan_host.py holds the planner itself to
    this function), as a dict:
    elim 'dense' | 'split' | 'k_time_eliminate'; acc 'mfma3' | 'mfma8' | 'valu_lds' | 'valu_mem' | ''; solve 'lds' | 'panel' | 'multi' | 'none';
    backsub 'split' | 'wg' | 'terms'.
    subset: some block in the program carries a non-zero subset mask (the cases themselves have none) — the split elimination and the
    split back-substitution then, whatever the switches say, and never k_time_backsub_wg.  priors: the problem carries block priors,
    which count as a loss."""
    if case.impl == 0:
        return dict(elim="dense", acc="", solve="dense", backsub="")
    env = dict(case.env)
    off = lambda k: k in env and int(env[k]) == 0   # noqa: E731
    nr, dmax, pmax, widest = structure(mc)
    assert 6 * pmax <= MT_MAXD
    with_loss = case.loss != "none" or priors
    split = with_loss or subset or not off("RSBA_MT_SPLIT")
    acc = ""
    if split:
        nt = (nr + 15) // 16
        per_wave = (nt * (nt + 1) // 2 + 15) // 16
        packed = nr * (nr + 1) // 2 + 3 * nr
        if per_wave <= 8 and not off("RSBA_MT_ACC_MFMA"):
            acc = "mfma3" if per_wave <= 3 else "mfma8"
        else:
            lds_s = _acc_lds_bytes(dmax, packed) <= LDS_CAP
            acc = "valu_lds" if lds_s else "valu_mem"
            if _acc_lds_bytes(dmax, packed if lds_s else 0) > LDS_CAP:
                assert not with_loss and not subset   # (the planner: RSBA_ERR_UNSUPPORTED, the dense path)
                split, acc = False, ""
    if nr == 0:
        solve = "none"
    elif nr <= CHOL_MAXN:
        solve = "lds" if nr <= PB * MRS_MAXP and _marker_solve_lds_doubles(nr) * 8 <= LDS_CAP and not off("RSBA_MT_SOLVE_LDS") else "panel"
    else:
        solve = "multi"
    backsub_wg = not with_loss and not subset and widest <= 128 and not off("RSBA_MT_BACKSUB_WG")
    split_backsub = split and (subset or not off("RSBA_MT_SPLIT_BACKSUB"))
    return dict(elim="split" if split else "k_time_eliminate", acc=acc, solve=solve, backsub="split" if split_backsub else ("wg" if backsub_wg else "terms"),
                loss=with_loss)


def path_failures(path, eliminates, stats):
    """What the solver's own report contradicts of `path` (eliminates_times() and the kernel statistics' names)."""
    has = lambda k: k in stats   # noqa: E731
    want = {}
    if path["elim"] == "dense":
        want.update(k_marker_system=True, k_mc_accumulate=False, k_time_eliminate=False, k_marker_reduced_solve=False, k_marker_chol_finish=False)
    else:
        want.update(k_marker_system=False, k_mc_accumulate=path["elim"] == "split", k_time_eliminate=path["elim"] != "split",
                    k_mc_slot_products=path["elim"] == "split", k_marker_reduce=True,
                    k_marker_reduced_solve=path["solve"] in ("lds", "panel"), k_marker_chol_finish=path["solve"] == "multi",
                    k_sys_build=path["solve"] == "multi", k_time_backsub_terms=True, k_marker_schur_finish=True,
                    k_mc_block_weight=path["elim"] == "split" and path.get("loss", False))
    out = ["eliminates_times() = %d" % eliminates] if eliminates != (0 if path["elim"] == "dense" else 1) else []
    out += ["%s %s" % (k, "missing" if v else "ran") for k, v in want.items() if has(k) != v]
    if path["solve"] == "multi" and not (has("k_chol_tiles_persistent") or has("k_chol_step(all panels)")):
        out.append("no multi-launch factorisation kernel ran")
    return out


def path_text(path):
    return "/".join(v for v in (path["elim"], path["acc"], path["solve"], path["backsub"]) if v)


def start_problem(case, converged=None):
    """The problem whose params are the case's starting state.  'second': `converged` (all parameters of a converged solve of the
    case's problem) with the free blocks perturbed by 1e-3 relative."""
    prob = problem(case.prob)
    if case.state != "second":
        return prob
    mc = chain(case)
    full = np.asarray(converged, float).reshape(-1, 6).copy()
    full[mc.free_blocks] = perturbed(full[mc.free_blocks].ravel()).reshape(-1, 6)
    return dict(prob, params=full.ravel())


def chain_at(case, prob):
    return ref.MarkerChain(prob, case.variant, case.loss, LOSS_A if case.loss != "none" else 0.0, constant_blocks(case, prob))

