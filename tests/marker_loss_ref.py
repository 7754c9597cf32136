"""A numpy reference for the marker-chain models with a robust loss (Ceres' HuberLoss / CauchyLoss and its corrector).

It shares no code with the product or with oracle/ (whose marker-chain models have no loss):

  residual block   one observation: the four marker corners (-h,+h) (+h,+h) (+h,-h) (-h,-h) through marker -> time -> camera and
                   the pinhole projection, 8 residuals (Main_Calibration/bundle_adjustment.h:56-343; variant 1 is Test2's wiring:
                   the marker transform always applied, marker 0 a block like any other)
  Jacobian         per block, 8 x 18 (camera | time | marker), by 18 complex-step passes (h = 1e-30).  Pass q perturbs local
                   parameter q of EVERY block of that kind at once, which is exact: a residual block depends on one pose of each kind.
  loss             s = |r|^2 over the block's 8 residuals, cost 1/2 sum rho(s); rho'' <= 0 for both losses, so the corrector
                   scales r and J by sqrt(rho'(s)) (ceres/corrector.cc with alpha = 0)
  normal equations J'J and J'r scattered block by block into a dense n x n matrix (no dense J)
  minimiser        SURVEY.md Appendix A.2 as tools/replay_point_model.minimise runs it: Jacobi scaling fixed at iteration 0,
                   D^2 = clamp(diag) / radius, Cholesky, the model cost change from the corrected rows, the tolerances in Ceres'
                   order, the candidate discarded on function tolerance, rho > 1e-3 accepts.
"""
import os
import re

import numpy as np

EPS = np.finfo(float).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HONGO_SERIALS = ["821312061029", "816612062327", "821212062536", "821212061326"]
TEST2_SERIALS = ["819612072493", "825312072048"]
HONGO_SIDE, TEST2_SIDE = 0.0148, 0.048


def read_intrinsics(serial):
    txt = open(os.path.join(GOLDEN, "intrinsics", "%s.xml" % serial)).read()
    K = np.array(re.search(r"<intrinsics[^>]*>.*?<data>(.*?)</data>", txt, re.S).group(1).split(), float).reshape(3, 3)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def load_correspondence(path, serials, marker_side):
    """correspondence.txt (header T C M N, T count rows, N rows 't c m u0 v0 .. u3 v3', then 6 (C + T + M) parameters)."""
    tok = open(path).read().split()
    T, C, M, N = (int(v) for v in tok[:4])
    q = 4 + T * (1 + C)
    rows = np.array(tok[q:q + 11 * N], float).reshape(N, 11)
    q += 11 * N
    params = np.array(tok[q:q + 6 * (C + T + M)], float)
    return dict(T=T, C=C, M=M, N=N, t=rows[:, 0].astype(np.int32), c=rows[:, 1].astype(np.int32), m=rows[:, 2].astype(np.int32),
                obs=rows[:, 3:].copy(), params=params, intr=np.stack([read_intrinsics(s) for s in serials]), marker_side=marker_side)


def hongo():
    return load_correspondence(os.path.join(GOLDEN, "hongo", "correspondence.txt"), HONGO_SERIALS, HONGO_SIDE)


def test2():
    return load_correspondence(os.path.join(GOLDEN, "test2", "correspondence_test.txt"), TEST2_SERIALS, TEST2_SIDE)


def rho_and_rho1(s, loss, a):
    """rho(s), rho'(s) of ceres::HuberLoss(a) / CauchyLoss(a); loss 'none' or a <= 0: s, 1."""
    if loss == "none" or a <= 0.0:
        return s, np.ones_like(s)
    b = a * a
    if loss == "huber":
        out = s > b
        rt = np.sqrt(np.where(out, s, 1.0))
        return np.where(out, 2.0 * a * rt - b, s), np.where(out, np.maximum(np.finfo(float).tiny, a / rt), 1.0)
    if loss == "cauchy":
        t = 1.0 + s / b
        return b * np.log(t), np.maximum(np.finfo(float).tiny, 1.0 / t)
    raise ValueError(loss)


def _rotate(w, X):
    """ceres::AngleAxisRotatePoint on rows (complex), the branch chosen on the real part of theta^2."""
    th2 = np.sum(w * w, axis=1)
    big = th2.real > EPS
    th = np.sqrt(np.where(big, th2, 1.0))
    c, s = np.cos(th), np.sin(th)
    k = w / th[:, None]
    rod = X * c[:, None] + np.cross(k, X) * s[:, None] + k * (np.sum(k * X, axis=1) * (1.0 - c))[:, None]
    return np.where(big[:, None], rod, X + np.cross(w, X))


class MarkerChain:
    """variant 0: Main_Calibration (camera 0 and marker 0 are left out of the chain and of the problem); 1: Test2 (camera 0 left out)."""

    def __init__(self, prob, variant=0, loss="none", a=0.0, constant_blocks=()):
        self.C, self.T, self.M, self.N = prob["C"], prob["T"], prob["M"], prob["N"]
        self.c, self.t, self.m = (np.asarray(prob[k], np.int64) for k in ("c", "t", "m"))
        self.obs = np.asarray(prob["obs"], float).reshape(self.N, 8)
        self.intr = np.asarray(prob["intr"], float).reshape(-1, 4)
        self.h = prob["marker_side"] / 2.0
        self.full0 = np.asarray(prob["params"], float).reshape(-1, 6).copy()
        self.loss, self.a = loss, a
        C, T = self.C, self.T
        self.has_cam = self.c != 0
        self.has_mar = np.ones(self.N, bool) if variant == 1 else self.m != 0
        blk = np.stack([np.where(self.has_cam, self.c, -1), C + self.t, np.where(self.has_mar, C + T + self.m, -1)], 1)   # (N, 3)
        nb = C + T + self.M
        used = np.zeros(nb, bool)
        used[blk[blk >= 0]] = True
        used[list(constant_blocks)] = False
        self.free_blocks = np.flatnonzero(used)
        pos = -np.ones(nb, np.int64)
        pos[self.free_blocks] = 6 * np.arange(self.free_blocks.size)
        self.n = 6 * self.free_blocks.size
        bp = np.where(blk >= 0, pos[np.maximum(blk, 0)], -1)                      # (N, 3) first column of each block, -1: none
        self.cols = np.where(np.repeat(bp, 6, axis=1) >= 0, np.repeat(bp, 6, axis=1) + np.tile(np.arange(6), 3), -1)   # (N, 18)

    # ---- parameters: the free blocks' values as one vector x (the blocks' order)
    def x0(self):
        return self.full0[self.free_blocks].ravel().copy()

    def full(self, x):
        f = self.full0.copy()
        f[self.free_blocks] = np.asarray(x, float).reshape(-1, 6)
        return f

    def residuals(self, full):
        """(N, 8) residuals at the (C + T + M, 6) poses (complex allowed)."""
        N, C, T, h = self.N, self.C, self.T, self.h
        corners = np.array([[-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [-h, -h, 0.0]])
        p = np.tile(corners, (N, 1)).astype(full.dtype)
        rep = lambda v: np.repeat(v, 4)   # noqa: E731
        mar, tim, cam = full[C + T + rep(self.m)], full[C + rep(self.t)], full[rep(self.c)]
        p = np.where(rep(self.has_mar)[:, None], _rotate(mar[:, :3], p) + mar[:, 3:], p)
        p = _rotate(tim[:, :3], p) + tim[:, 3:]
        p = np.where(rep(self.has_cam)[:, None], _rotate(cam[:, :3], p) + cam[:, 3:], p)
        K = self.intr[rep(self.c)]
        o = self.obs.reshape(-1, 2)
        u = K[:, 0] * p[:, 0] / p[:, 2] + K[:, 2] - o[:, 0]
        v = K[:, 1] * p[:, 1] / p[:, 2] + K[:, 3] - o[:, 1]
        return np.stack([u, v], axis=1).reshape(N, 8)

    def jacobians(self, full):
        """(N, 8, 18): columns camera | time | marker of each block; a column of an absent or constant block is zero."""
        C, T, M = self.C, self.T, self.M
        J = np.zeros((self.N, 8, 18))
        ranges = [(0, C), (C, C + T), (C + T, C + T + M)]
        for q in range(18):
            lo, hi = ranges[q // 6]
            f = full.astype(complex)
            f[lo:hi, q % 6] += 1e-30j
            J[:, :, q] = self.residuals(f).imag / 1e-30
        J[self.cols[:, None, :].repeat(8, axis=1) < 0] = 0.0
        return J

    def cost(self, x):
        r = self.residuals(self.full(x))
        s = np.sum(r * r, axis=1)
        rho, _ = rho_and_rho1(s, self.loss, self.a)
        return 0.5 * float(np.sum(rho)), float(np.sum(s))

    def linearise(self, x):
        """cost, corrected rows (r~ (N, 8), J~ (N, 8, 18)), H = J~'J~ and g = J~'r~ (dense, n), raw sum of squares."""
        full = self.full(x)
        r = self.residuals(full)
        J = self.jacobians(full)
        s = np.sum(r * r, axis=1)
        rho, rho1 = rho_and_rho1(s, self.loss, self.a)
        sq = np.sqrt(rho1)
        rt, Jt = r * sq[:, None], J * sq[:, None, None]
        n = self.n
        H = np.zeros((n, n))
        g = np.zeros(n)
        cl = np.where(self.cols >= 0, self.cols, n)             # a dump row / column n for the absent ones
        Hb = np.einsum("kra,krb->kab", Jt, Jt)
        gb = np.einsum("kra,kr->ka", Jt, rt)
        Hx = np.zeros((n + 1, n + 1))
        np.add.at(Hx, (cl[:, :, None], cl[:, None, :]), Hb)
        gx = np.zeros(n + 1)
        np.add.at(gx, cl, gb)
        H, g = Hx[:n, :n], gx[:n]
        return 0.5 * float(np.sum(rho)), rt, Jt, H, g, float(np.sum(s))

    def model_cost_change(self, rt, Jt, delta):
        d = np.where(self.cols >= 0, np.append(delta, 0.0)[np.where(self.cols >= 0, self.cols, self.n)], 0.0)   # (N, 18)
        Jd = np.einsum("krq,kq->kr", Jt, d)
        return -float(np.sum(Jd * (rt + 0.5 * Jd)))


def minimise(mc, max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
             max_lm_diagonal=1e32, max_invalid=5):
    """Ceres' LM -> (x, summary, iteration rows)."""
    x = mc.x0()
    rows = []
    cost, r, J, H, g, sumsq = mc.linearise(x)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    rows.append(dict(iteration=0, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()), step_norm=0.0, relative_decrease=0.0,
                     trust_region_radius=initial_radius, valid=0, successful=0))
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
                   trust_region_radius=radius, valid=0, successful=0)
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
        if row["step_norm"] <= parameter_tolerance * (np.linalg.norm(x) + parameter_tolerance):
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


def covariance(mc, x):
    """(J~'J~)^-1 over the free blocks at x (the corrector of mc's loss), with the free blocks' order -> (S^-1, free block ids)."""
    _, _, _, H, _, _ = mc.linearise(x)
    return np.linalg.inv(H), mc.free_blocks


def displace_corners(prob, frac, pixels, seed):
    """A copy of prob with about frac of its corners moved by `pixels` in a random direction (fixed seed)."""
    rng = np.random.default_rng(seed)
    out = dict(prob)
    obs = np.array(prob["obs"], float).reshape(-1, 4, 2)
    hit = rng.random(obs.shape[:2]) < frac
    ang = rng.uniform(0.0, 2.0 * np.pi, obs.shape[:2])
    obs[..., 0] += np.where(hit, pixels * np.cos(ang), 0.0)
    obs[..., 1] += np.where(hit, pixels * np.sin(ang), 0.0)
    out["obs"] = obs.reshape(-1, 8)
    return out
