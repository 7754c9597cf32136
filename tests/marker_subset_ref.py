"""The numpy reference of tests/marker_loss_ref.py / marker_weight_ref.py with constant components of a pose block
(ceres::SubsetParameterization(6, constant_parameters); rsba_problem_set_parameter_subset_constant).

Ceres evaluates a partly constant block through its 6 x (6 - k) local Jacobian.  Here the masked components are REMOVED from the
program: `cols` is compacted, n is the number of free components, x0 / full scatter through the kept components only.  Nothing here
knows about zero columns or unit diagonals, so the reference is independent of how the device decouples a masked component;
tests/test_marker_subset_ref_cpu.py shows the two formulations agree.

The convergence tests use the AMBIENT norms, as TrustRegionMinimizer does (x_.norm() over the parameter vector of the reduced
program): |x| counts the constant components of a partly constant block, |step| gets 0 from them; a wholly constant block is not in
the program at all.  minimise() below is marker_loss_ref.minimise with that one difference (marker_loss_ref's takes |x| over x0()).

A mask on a block that is constant as a whole, a fixed base block or a block no residual names is ignored.
"""
import numpy as np

import marker_distortion_ref as dref
import marker_loss_ref as ref
import marker_step_accuracy as msa
import marker_weight_ref as wref
import solve_accuracy as sa


def masks_of(prob):
    """The issue's masks, by block index in [C | T | M] order: camera 1's rotation held, two components of a time, three of marker 2,
    all but one of marker 1."""
    C, T = prob["C"], prob["T"]
    return {1: 0b000111, C + 3: 0b100100, C + T + 2: 0b100011, C + T + 1: 0b011111}


class SubsetMixin:
    def _init_subset(self, masks):
        nb = self.C + self.T + self.M
        bits = np.zeros((nb, 6), bool)
        for b, m in masks.items():
            assert 0 <= m < 63
            bits[b] = [(m >> q) & 1 for q in range(6)]
        self.masks = dict(masks)
        self.ambient_n = self.n
        self.ambient_cols = self.cols                  # (N, 18) columns in the ambient free vector (the parent's)
        self.keep = ~bits[self.free_blocks].ravel()    # ambient free component -> kept
        newpos = -np.ones(self.ambient_n + 1, np.int64)
        newpos[:self.ambient_n][self.keep] = np.arange(int(self.keep.sum()))
        self.cols = np.where(self.cols >= 0, newpos[np.maximum(self.cols, 0)], -1)
        self.n = int(self.keep.sum())
        self.col_block = np.repeat(self.free_blocks, 6)[self.keep]   # block of every kept column
        self.masked_slots = (6 * self.free_blocks[:, None] + np.arange(6))[bits[self.free_blocks]]   # flat offsets in [C | T | M] x 6

    def x0(self):
        return self.full0[self.free_blocks].ravel()[self.keep].copy()

    def compact(self, full):
        """The kept components of (C + T + M, 6) parameters."""
        return np.asarray(full).reshape(-1, 6)[self.free_blocks].ravel()[self.keep].copy()

    def full(self, x):
        f = self.full0.copy()
        v = f[self.free_blocks].ravel()
        v[self.keep] = np.asarray(x, float)
        f[self.free_blocks] = v.reshape(-1, 6)
        return f

    def ambient_norm(self, x):
        """|x| over every component of the blocks in the program, the constant components included."""
        return float(np.linalg.norm(self.full(x)[self.free_blocks]))

    def lift(self, v):
        """A vector over the kept components -> the ambient free vector, zeros in the masked components."""
        out = np.zeros(self.ambient_n)
        out[self.keep] = v
        return out


class SubsetMarkerChain(SubsetMixin, wref.WeightedMarkerChain):
    def __init__(self, prob, masks, weights=None, variant=0, loss="none", a=0.0, constant_blocks=()):
        wref.WeightedMarkerChain.__init__(self, prob, np.ones(prob["N"]) if weights is None else weights, variant, loss, a, constant_blocks)
        self._init_subset(masks)


class SubsetMarkerChainDist(SubsetMixin, dref.WeightedMarkerChainDist):
    def __init__(self, prob, dist, masks, weights=None, variant=0, loss="none", a=0.0, constant_blocks=()):
        dref.WeightedMarkerChainDist.__init__(self, prob, dist, np.ones(prob["N"]) if weights is None else weights, variant, loss, a, constant_blocks)
        self._init_subset(masks)


def minimise(mc, max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
             max_lm_diagonal=1e32, max_invalid=5, ambient=True):
    """marker_loss_ref.minimise with |x| of the parameter tolerance taken over the ambient vector (ambient = False: over x0()'s
    components, marker_loss_ref's rule — kept to show that the two differ).  Rows also carry x_norm."""
    x = mc.x0()
    rows = []
    cost, r, J, H, g, sumsq = mc.linearise(x)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    rows.append(dict(iteration=0, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()), step_norm=0.0, relative_decrease=0.0,
                     trust_region_radius=initial_radius, valid=0, successful=0, x_norm=0.0))
    out = dict(initial_cost=cost)

    def done(term, reason):
        return x, dict(out, termination=term, reason=reason, final_cost=cost, final_sumsq=sumsq), rows

    if np.abs(g).max() <= gradient_tolerance:
        return done("CONVERGENCE", "gradient")
    radius, dec, invalid, it = initial_radius, 2.0, 0, 0
    while True:
        if it >= max_num_iterations:
            return done("NO_CONVERGENCE", "max_iterations")
        if np.abs(g).max() <= gradient_tolerance:
            return done("CONVERGENCE", "gradient")
        if radius < min_radius:
            return done("CONVERGENCE", "min_radius")
        it += 1
        row = dict(iteration=it, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()), step_norm=0.0, relative_decrease=0.0,
                   trust_region_radius=radius, valid=0, successful=0, x_norm=0.0)
        Hs = H * np.outer(scale, scale)
        D2 = np.clip(np.diag(Hs), min_lm_diagonal, max_lm_diagonal) / radius
        ok = True
        try:
            L = np.linalg.cholesky(Hs + np.diag(D2))
            y = np.linalg.solve(L.T, np.linalg.solve(L, scale * g))
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            delta = -y * scale
            mcc = mc.model_cost_change(r, J, delta)
            ok = bool(np.all(np.isfinite(delta))) and mcc > 0.0
        if not ok:
            invalid += 1
            radius /= dec
            dec *= 2.0
            row["trust_region_radius"] = radius
            rows.append(row)
            if invalid >= max_invalid:
                return done("FAILURE", "invalid_steps")
            continue
        invalid = 0
        row["valid"] = 1
        xc = x + delta
        cand, _ = mc.cost(xc)
        row["step_norm"] = float(np.linalg.norm(delta))
        row["x_norm"] = mc.ambient_norm(x) if ambient else float(np.linalg.norm(x))
        if row["step_norm"] <= parameter_tolerance * (row["x_norm"] + parameter_tolerance):
            rows.append(row)
            return done("CONVERGENCE", "parameter")
        row["cost_change"] = cost - cand
        if abs(cost - cand) <= function_tolerance * cost:
            rows.append(row)
            return done("CONVERGENCE", "function")
        rel = (cost - cand) / mcc
        row["relative_decrease"] = rel
        if np.isfinite(cand) and rel > min_relative_decrease:
            x = xc
            cost, r, J, H, g, sumsq = mc.linearise(x)
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            dec = 2.0
            row.update(successful=1, cost=cost, gradient_max_norm=float(np.abs(g).max()))
        else:
            radius /= dec
            dec *= 2.0
        row["trust_region_radius"] = radius
        rows.append(row)


def lm_step(H, g, radius, min_lm=1e-6, max_lm=1e32):
    """One damped step of minimise() on (H, g): Jacobi scale from H's diagonal, D = clip / radius, Cholesky."""
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    Hs = H * np.outer(scale, scale)
    D2 = np.clip(np.diag(Hs), min_lm, max_lm) / radius
    L = np.linalg.cholesky(Hs + np.diag(D2))
    return -scale * np.linalg.solve(L.T, np.linalg.solve(L, scale * g))


def zero_column_system(mc, H, g):
    """The formulation a device may use instead of removing columns: the ambient system with the masked components' rows, columns
    and gradient entries zero and a unit diagonal there."""
    Ha = np.zeros((mc.ambient_n, mc.ambient_n))
    Ha[np.ix_(mc.keep, mc.keep)] = H
    Ha[~mc.keep, ~mc.keep] = 1.0
    return Ha, mc.lift(g)


def covariance(mc, x):
    """Ceres' lift through the parameterisations' Jacobians: the inverse of J~'J~ over the free components, zeros in the rows and
    columns of the masked ones -> (6 F x 6 F over the free blocks, free block ids)."""
    _, _, _, H, _, _ = mc.linearise(x)
    cov = np.zeros((mc.ambient_n, mc.ambient_n))
    cov[np.ix_(mc.keep, mc.keep)] = np.linalg.inv(H)
    return cov, mc.free_blocks


class SubsetSystem(msa.System):
    """marker_step_accuracy.System for a chain with removed components: the damped normal equations over the kept components (n the
    free count), the conditioning of the blocks a device inverts explicitly — a time's kept components form its block — and the bar's
    row-independent part.  No arithmetic is added to row formation by a mask (an omitted seed, or a product with an exact 0 or 1), so
    the rounding count of an entry stays marker_step_accuracy's; m is counted on the unmasked columns."""

    def __init__(self, mc, x, radius, dense, min_lm=msa.MIN_LM, max_lm=msa.MAX_LM):   # noqa: super().__init__ not called: it assumes 6 columns a block
        assert sa.longdouble_ok()
        self.mc, self.x, self.radius, self.n = mc, np.asarray(x, float).copy(), radius, mc.n
        self.cost, self.rt, self.Jt, _, _, _ = mc.linearise(self.x)
        self.H, self.g = msa._longdouble_normal_equations(mc, self.rt, self.Jt)
        dH = np.diagonal(self.H).astype(np.float64)
        self.s = 1.0 / (1.0 + np.sqrt(dH))
        self.D = np.clip(dH * self.s ** 2, min_lm, max_lm) / radius
        self.A = self.H + np.diag((self.D / self.s ** 2).astype(np.longdouble))
        self.b = -self.g
        self.gmax = float(np.abs(self.g).max())
        first = mc.ambient_cols[:, ::6]
        first = first[first >= 0] // 6
        self.m = 8 * int(np.bincount(first).max())
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


# ---- the cases tests/test_marker_subset_ref_cpu.py pins and tests/test_gpu_marker_subset.py solves on the device
CASES = {"S1": "4x40x6_mask_none", "S2": "hongo_mask_huber", "S3": "const_mask_huber"}   # marker_weight_ref.case(name)["prob"], weights unused


def scattered_masks(prob, fraction, seed):
    """Masks of one to five random components on about `fraction` of the blocks of [C | T | M] (fixed seed)."""
    rng = np.random.default_rng(seed)
    nb = prob["C"] + prob["T"] + prob["M"]
    return {int(b): int(rng.integers(1, 63)) for b in np.flatnonzero(rng.random(nb) < fraction)}


def case(sid):
    """-> dict(prob, variant, loss, a, constant_blocks, masks, weights).  S1 - S3: the issue's table.  X12: (12, 40, 20), 432 unknowns
    — the default path rule eliminates the times, the accumulation runs on the matrix cores — with masks on a tenth of its blocks.
    S1w: S1's data and masks under 4x40x6_frac_huber's weights and Huber loss.  D1: marker_distortion_ref's 4x40x6 rig (detections
    made through its coefficients) with the issue's masks."""
    if sid == "D1":
        cs = dref.case("4x40x6")
        return dict(prob=cs["prob"], dist=cs["dist"], variant=cs["variant"], loss=cs["loss"], a=cs["a"], constant_blocks=cs["constant_blocks"],
                    masks=masks_of(cs["prob"]), weights=cs["weights"])
    if sid == "X12":
        cs = wref.case("12x40x20_mask_none")
        return dict(prob=cs["prob"], variant=0, loss="none", a=0.0, constant_blocks=(), masks=scattered_masks(cs["prob"], 0.1, 16), weights=None)
    if sid == "S1w":
        cs = wref.case("4x40x6_frac_huber")
        return dict(prob=cs["prob"], variant=0, loss=cs["loss"], a=cs["a"], constant_blocks=(), masks=masks_of(cs["prob"]), weights=cs["weights"])
    cs = wref.case(CASES[sid])
    return dict(prob=cs["prob"], variant=cs["variant"], loss=cs["loss"], a=cs["a"], constant_blocks=cs["constant_blocks"],
                masks=masks_of(cs["prob"]), weights=None)


def chain_of(cs, prob=None, masks=None):
    if cs.get("dist") is not None:
        return SubsetMarkerChainDist(cs["prob"] if prob is None else prob, cs["dist"], cs["masks"] if masks is None else masks, cs.get("weights"),
                                     cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
    return SubsetMarkerChain(cs["prob"] if prob is None else prob, cs["masks"] if masks is None else masks, cs.get("weights"),
                             cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])


_RUNS = {}


def reference_run(sid):
    """(case, chain, summary, rows, final (C + T + M, 6)) of the subset reference's minimisation, once per process."""
    if sid not in _RUNS:
        cs = case(sid)
        mc = chain_of(cs)
        x, summary, rows = minimise(mc)
        _RUNS[sid] = (cs, mc, summary, rows, mc.full(x))
    return _RUNS[sid]
