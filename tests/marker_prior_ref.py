"""The numpy reference of tests/marker_subset_ref.py with Gaussian priors on camera and marker blocks
(ceres::NormalPrior(A, b); rsba_problem_set_block_prior).

A prior on block B is six more residuals A (x_B - b) with no loss and the Jacobian A, in the block's own coordinates (rvec, tvec), the
plain difference of the six parameters.  Here they are appended to the program the parent classes build: the cost gets
1/2 |A (x_B - b)|^2, H gets A~'A~ on the block's columns and g gets A~'A (x_B - b), where A~ keeps the columns of the block's free
components only (marker_subset_ref REMOVES masked components; the residual still uses the held values).  A block that is constant as a
whole has no column: its prior counts in the cost only.  No loss, no weight and no raw sum of squares ever sees a prior.

Shares no code with the product; minimise is marker_subset_ref.minimise.
"""
import numpy as np

import marker_distortion_ref as dref
import marker_step_accuracy as msa
import marker_subset_ref as sref
import marker_weight_ref as wref
import solve_accuracy as sa

minimise = sref.minimise
SIGMA = 0.02


class PriorMixin:
    def _init_priors(self, priors):
        """priors: {block in [C | T | M]: (A 6 x 6, b 6)}; walked in ascending block order everywhere."""
        self.priors = {int(b): (np.asarray(A, float).reshape(6, 6).copy(), np.asarray(v, float).reshape(6).copy()) for b, (A, v) in sorted(priors.items())}
        C, T = self.C, self.T
        for b in self.priors:
            assert not (C <= b < C + T), "no priors on time blocks"
        comp = np.tile(np.arange(6), self.free_blocks.size)[self.keep]   # component of every kept column
        self.prior_cols = {}
        for b in self.priors:
            at = np.flatnonzero(self.col_block == b)                     # the block's kept columns (none: constant as a whole)
            self.prior_cols[b] = (at, comp[at])
        self._lins = {}

    def prior_rows(self, x):
        """-> [(block, r (6), columns, A~ (6 x len(columns)))] at x, ascending block order."""
        full = self.full(x)
        out = []
        for b, (A, v) in self.priors.items():
            at, q = self.prior_cols[b]
            out.append((b, A @ (full[b] - v), at, A[:, q]))
        return out

    def prior_cost(self, x):
        return 0.5 * float(sum(np.sum(r * r) for _, r, _, _ in self.prior_rows(x)))

    def cost(self, x):
        c, sumsq = super().cost(x)
        return c + self.prior_cost(x), sumsq

    def linearise(self, x):
        cost, rt, Jt, H, g, sumsq = super().linearise(x)
        H, g = H.copy(), g.copy()
        rows = self.prior_rows(x)
        for _, r, at, Ak in rows:
            cost += 0.5 * float(np.sum(r * r))
            H[np.ix_(at, at)] += Ak.T @ Ak
            g[at] += Ak.T @ r
        self._lins[id(rt)] = (rt, rows)   # (rt is kept alive here, so its id names this linearisation for good)
        return cost, rt, Jt, H, g, sumsq

    def model_cost_change(self, rt, Jt, delta):
        assert id(rt) in self._lins and self._lins[id(rt)][0] is rt, "model_cost_change wants rows that linearise() returned"
        mcc = super().model_cost_change(rt, Jt, delta)
        for _, r, at, Ak in self._lins[id(rt)][1]:
            Jd = Ak @ np.asarray(delta)[at]
            mcc -= float(np.sum(Jd * (r + 0.5 * Jd)))
        return mcc

    def stacked_residuals(self, full):
        """[the observations' raw residuals; A (x_B - b) of every prior, ascending block order] at (C + T + M, 6) poses (complex allowed)."""
        parts = [self.residuals(full).ravel()]
        for b, (A, v) in self.priors.items():
            parts.append(A @ (full[b] - v))
        return np.concatenate(parts)


class PriorMarkerChain(PriorMixin, sref.SubsetMarkerChain):
    def __init__(self, prob, priors, masks=None, weights=None, variant=0, loss="none", a=0.0, constant_blocks=()):
        sref.SubsetMarkerChain.__init__(self, prob, masks or {}, weights, variant, loss, a, constant_blocks)
        self._init_priors(priors)


class PriorMarkerChainDist(PriorMixin, sref.SubsetMarkerChainDist):
    def __init__(self, prob, dist, priors, masks=None, weights=None, variant=0, loss="none", a=0.0, constant_blocks=()):
        sref.SubsetMarkerChainDist.__init__(self, prob, dist, masks or {}, weights, variant, loss, a, constant_blocks)
        self._init_priors(priors)


class PriorSystem(sref.SubsetSystem):
    """marker_subset_ref.SubsetSystem with the priors' rows appended: H and g get A~'A~ and A~'r in np.longdouble, and the bar's
    longest sum m counts the six extra rows of a prior block (8 x the residual blocks that name a free block, + 6 where it carries a
    prior).  A prior's row entries are the caller's values, not formed by the chain rule: counting them like the others (2 x 37
    roundings a product) only widens nothing that is measured here — m enters through gamma_{m + 74}, the same expression."""

    def __init__(self, mc, x, radius, dense, min_lm=msa.MIN_LM, max_lm=msa.MAX_LM):   # noqa: the parents' __init__ build H without the prior rows
        assert sa.longdouble_ok()
        self.mc, self.x, self.radius, self.n = mc, np.asarray(x, float).copy(), radius, mc.n
        self.cost, self.rt, self.Jt, _, _, _ = mc.linearise(self.x)
        H, g = msa._longdouble_normal_equations(mc, self.rt, self.Jt)
        self.H, self.g = H.copy(), g.copy()
        for _, r, at, Ak in mc.prior_rows(self.x):
            Al, rl = Ak.astype(np.longdouble), r.astype(np.longdouble)
            self.H[np.ix_(at, at)] += Al.T @ Al
            self.g[at] += Al.T @ rl
        dH = np.diagonal(self.H).astype(np.float64)
        self.s = 1.0 / (1.0 + np.sqrt(dH))
        self.D = np.clip(dH * self.s ** 2, min_lm, max_lm) / radius
        self.A = self.H + np.diag((self.D / self.s ** 2).astype(np.longdouble))
        self.b = -self.g
        self.gmax = float(np.abs(self.g).max())
        first = mc.ambient_cols[:, ::6]
        rows_of = 8 * np.bincount(first[first >= 0] // 6, minlength=mc.free_blocks.size)
        for b in mc.priors:
            at = np.flatnonzero(mc.free_blocks == b)
            rows_of[at] += 6
        self.m = int(rows_of.max())
        As = np.asarray(self.H, np.float64) * np.outer(self.s, self.s) + np.diag(self.D)
        C, T = mc.C, mc.T
        is_time = (mc.col_block >= C) & (mc.col_block < C + T)
        if dense:
            self.kappa_t, self.kappa_s = 0.0, float(sa.diag_block_kappas(As).max())
        else:
            ri = np.flatnonzero(~is_time)
            kt, S = [0.0], As[np.ix_(ri, ri)].copy()
            for b in np.unique(mc.col_block[is_time]):
                q = np.flatnonzero(mc.col_block == b)
                kt.append(float(sa.diag_block_kappas(As[np.ix_(q, q)], 6).max()))
                W = As[np.ix_(q, ri)]
                S -= W.T @ np.linalg.solve(As[np.ix_(q, q)], W)
            self.kappa_t = max(kt)
            self.kappa_s = float(sa.diag_block_kappas(S).max()) if ri.size else 0.0
        self.kappa = max(self.kappa_t, self.kappa_s)
        gf = sa.gamma(self.m + 2 * msa.C_JAC)
        self.forming = gf / (1.0 - gf)
        self.solve = sa.gamma(3 * self.n + 1) / (1.0 - sa.gamma(self.n + 1)) * (1.0 + self.kappa)
        self._d = np.sqrt(np.maximum(np.diagonal(self.A), 0))
        self._absA = np.abs(self.A)


def rank4():
    """A dense 6 x 6 of rank 4 (two zero rows), entries of the size of 1 / SIGMA (fixed seed)."""
    A = np.random.default_rng(7).standard_normal((6, 6)) / SIGMA / 2.0
    A[4:] = 0.0
    return A


def priors_of(prob, variant=0, sigma=SIGMA):
    """The issue's set: A = diag(1 / sigma) on camera 2 and on every non-base marker, b = the start values; the last marker carries the
    dense rank-4 A instead.  (variant 1, Test2's wiring: marker 0 is a block like any other and carries one too.)"""
    C, T, M = prob["C"], prob["T"], prob["M"]
    start = np.asarray(prob["params"], float).reshape(-1, 6)
    blocks = [2] + [C + T + m for m in range(0 if variant == 1 else 1, M)]
    out = {b: (np.eye(6) / sigma, start[b].copy()) for b in blocks}
    out[C + T + M - 1] = (rank4() * (SIGMA / sigma), start[C + T + M - 1].copy())
    return out


def third_of_blocks(prob, sigma=SIGMA):
    """Priors on every third camera / marker block (the fixed bases left out), b = the start values."""
    C, T, M = prob["C"], prob["T"], prob["M"]
    start = np.asarray(prob["params"], float).reshape(-1, 6)
    blocks = [b for b in list(range(1, C)) + list(range(C + T + 1, C + T + M)) if b % 3 == 0]
    return {b: (np.eye(6) / sigma, start[b].copy()) for b in blocks}


def case(pid):
    """-> dict(prob, variant, loss, a, constant_blocks, masks, weights, priors[, dist]): the issue's table.
    P3: const_mask_huber's problem and constants (camera 2 and marker 3, both prior blocks, are constant as a whole: their priors
    count in the cost only) and marker_subset_ref's masks (marker 1 and marker 2, both prior blocks, carry one)."""
    if pid == "D1":
        cs = dref.case("4x40x6")
        return dict(prob=cs["prob"], dist=cs["dist"], variant=cs["variant"], loss=cs["loss"], a=cs["a"], constant_blocks=tuple(cs["constant_blocks"]),
                    masks={}, weights=cs["weights"], priors=priors_of(cs["prob"], cs["variant"]))
    if pid == "X12":
        cs = wref.case("12x40x20_mask_none")
        return dict(prob=cs["prob"], variant=0, loss="none", a=0.0, constant_blocks=(), masks={}, weights=None, priors=third_of_blocks(cs["prob"]))
    if pid == "P1w":
        cs = wref.case("4x40x6_frac_huber")
        return dict(prob=cs["prob"], variant=0, loss=cs["loss"], a=cs["a"], constant_blocks=(), masks={}, weights=cs["weights"], priors=priors_of(cs["prob"]))
    if pid == "P3":
        cs = wref.case("const_mask_huber")
        p = cs["prob"]
        consts = tuple(cs["constant_blocks"])   # camera 2 and marker 3 among them: prior blocks that are constant as a whole
        masks = {b: m for b, m in sref.masks_of(p).items() if b not in consts}
        return dict(prob=p, variant=cs["variant"], loss=cs["loss"], a=cs["a"], constant_blocks=consts, masks=masks, weights=None,
                    priors=priors_of(p, cs["variant"]))
    name, variant = {"P1": ("4x40x6_mask_none", 0), "P2": ("hongo_mask_huber", 0), "P4": ("4x40x6_mask_none", 1)}[pid]
    cs = wref.case(name)
    loss, a = (cs["loss"], cs["a"]) if pid == "P2" else ("none", 0.0)
    return dict(prob=cs["prob"], variant=variant, loss=loss, a=a, constant_blocks=(), masks={}, weights=None, priors=priors_of(cs["prob"], variant))


def chain_of(cs, priors=None):
    pri = cs["priors"] if priors is None else priors
    if cs.get("dist") is not None:
        return PriorMarkerChainDist(cs["prob"], cs["dist"], pri, cs["masks"], cs.get("weights"), cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
    return PriorMarkerChain(cs["prob"], pri, cs["masks"], cs.get("weights"), cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])


_RUNS = {}


def reference_run(pid, with_priors=True):
    """(case, chain, summary, rows, final (C + T + M, 6)) of the reference's minimisation, once per process (with_priors False: the
    same program without its priors)."""
    key = (pid, with_priors)
    if key not in _RUNS:
        cs = case(pid)
        mc = chain_of(cs, None if with_priors else {})
        x, summary, rows = minimise(mc)
        _RUNS[key] = (cs, mc, summary, rows, mc.full(x))
    return _RUNS[key]
