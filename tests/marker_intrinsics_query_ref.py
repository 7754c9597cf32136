"""A numpy reference for the queries of a marker-chain solver with free intrinsics under the extended layout
(rsba_solver_set_extended_layout): cost, residuals, gradient and covariance at any extended vector

    xe = [the problem's parameters, 6 per block of C | T | M  |  fx fy cx cy k1 k2 of EVERY camera index, camera k at 6 (C + T + M) + 6 k]

It builds on tests/marker_intrinsics_ref.py (imported, not edited) and shares no code with the product.  `MarkerChainIntr` keeps the
values of what it does not solve for — constant and unreferenced blocks, cameras without a mask — from the problem it was built
from, so the chain is built FROM xe (`Queries.at`): every value of the extended vector is then the one the formulas read, held or not.
`linearise` gives cost, corrected residuals, H and g over [free pose blocks | 6 per camera with a mask]; this module maps that vector
to and from the extended offsets, scatters g with zeros elsewhere, and takes the covariance as inv(H[keep, keep]), keep = ~held,
scattered likewise.
"""
import numpy as np

import marker_intrinsics_ref as iref

U = 2.0 ** -53


def extended_x0(cs):
    """The extended vector a solver created from the case starts at."""
    prob = cs["prob"]
    six = np.concatenate([np.asarray(prob["intr"], float).reshape(-1, 4), np.asarray(cs["dist"], float).reshape(-1, 5)[:, :2]], axis=1)
    return np.concatenate([np.asarray(prob["params"], float).ravel(), six.ravel()])


def case_at(cs, xe):
    """The case whose problem holds xe's values: parameters, intrinsics and k1 k2 (p1 p2 k3 stay)."""
    prob = cs["prob"]
    nb = prob["C"] + prob["T"] + prob["M"]
    xe = np.asarray(xe, float)
    assert xe.shape == (6 * nb + 6 * prob["C"],)
    six = xe[6 * nb:].reshape(-1, 6)
    dist = np.asarray(cs["dist"], float).reshape(-1, 5).copy()
    dist[:, :2] = six[:, 4:]
    p2 = dict(prob, params=xe[:6 * nb].copy(), intr=six[:, :4].copy(), dist=dist)
    return dict(cs, prob=p2, dist=dist)


def perturbed(cs, seed=11):
    """The issue's perturbation of the start: poses (rvec 0.01, tvec 0.02 of the largest translation's scale), fx fy by 1 %, cx cy by
    3 px, k1 k2 by 0.01 — every slot, held or not."""
    rng = np.random.default_rng(seed)
    xe = extended_x0(cs)
    prob = cs["prob"]
    nb = prob["C"] + prob["T"] + prob["M"]
    poses = xe[:6 * nb].reshape(-1, 6)
    poses[:, :3] += rng.uniform(-0.01, 0.01, (nb, 3))
    poses[:, 3:] += rng.uniform(-0.02, 0.02, (nb, 3)) * max(1e-3, float(np.abs(poses[:, 3:]).max())) / 10.0
    six = xe[6 * nb:].reshape(-1, 6)
    six[:, :2] *= 1.0 + rng.uniform(-0.01, 0.01, (prob["C"], 2))
    six[:, 2:4] += rng.uniform(-3.0, 3.0, (prob["C"], 2))
    six[:, 4:] += rng.uniform(-0.01, 0.01, (prob["C"], 2))
    return xe


class Queries:
    """The reference at one extended vector."""

    def __init__(self, cs, xe):
        self.cs = case_at(cs, xe)
        self.mc = mc = iref.chain_of(self.cs)
        self.xe = np.asarray(xe, float).copy()
        self.C, self.T, self.M, self.N = mc.C, mc.T, mc.M, mc.N
        self.nb = mc.C + mc.T + mc.M
        self.npar, self.next = 6 * self.nb, 6 * self.nb + 6 * mc.C
        self.x = mc.x0()
        # extended offset of every entry of the chain's vector
        self.ext_of = np.concatenate([(6 * mc.free_blocks[:, None] + np.arange(6)).ravel(), (self.npar + 6 * mc.cams[:, None] + np.arange(6)).ravel()]).astype(np.int64)
        assert self.ext_of.shape == (mc.n,) and np.array_equal(self.xe[self.ext_of], self.x)
        self.lin = mc.linearise(self.x)

    # ---- the mapping
    def to_chain(self, xe):
        return np.asarray(xe, float)[self.ext_of]

    def to_extended(self, v, fill=0.0):
        out = np.full(self.next, fill)
        out[self.ext_of] = v
        return out

    def computed(self):
        """bool [next]: the gradient slots that are computed; the others are literal 0.0 (constant, base and unreferenced blocks,
        constant components, held intrinsics, cameras without a block)."""
        m = np.zeros(self.next, bool)
        m[self.ext_of] = ~self.mc.held
        return m

    # ---- evaluate
    def cost(self):
        return self.lin[0]

    def residuals(self):
        """8 N corrected residuals in the problem's observation order, then six per prior in ascending block order."""
        rt = self.lin[1]
        return np.concatenate([rt[:self.N].ravel(), rt[self.N:, :6].ravel()])

    def gradient(self):
        return self.to_extended(self.lin[4])

    def raw_rounding(self):
        """d_r: the largest difference between the raw float64 residuals and the same formulas run in np.longdouble."""
        mc = self.mc
        full, six = mc.full(self.x), mc.six(self.x)
        r64 = mc.residuals_at(full, six)
        rld = mc.residuals_at(full.astype(np.longdouble), six.astype(np.longdouble))
        assert rld.dtype == np.longdouble and np.finfo(np.longdouble).eps < np.finfo(float).eps
        return float(np.abs(rld - r64.astype(np.longdouble)).max())

    def rbar(self):
        coord = float(np.abs(self.mc.obs).max())
        return 16.0 * max(self.raw_rounding(), 4.0 * np.spacing(coord))

    def gradient_bars(self, rbar):
        """test_gpu_evaluate's bar per entry: sum_i |J_ik| rbar + (64 + n_k) u sum_i |J_ik r_i|, extended offsets."""
        mc, (_, rt, Jt, _, _, _) = self.mc, self.lin
        n = mc.n
        cl = np.where(mc.cols_all >= 0, mc.cols_all, n)
        a, b, cnt = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
        np.add.at(a, cl, np.abs(Jt).sum(axis=1))
        np.add.at(b, cl, np.abs(Jt * rt[:, :, None]).sum(axis=1))
        np.add.at(cnt, cl, 8.0)
        return self.to_extended(a[:n] * rbar + (64.0 + cnt[:n]) * U * b[:n])

    def cost_bar(self, rbar):
        r = self.residuals()
        return rbar * float(np.abs(r).sum()) + r.size * U * self.cost()

    # ---- covariance
    def covariance(self, how="inv"):
        """(n, n) over the chain's vector: inv(H[keep, keep]) scattered, zeros in the held rows and columns.  how: "inv"
        (np.linalg.inv) or "chol" (the Cholesky inverse of the Jacobi-scaled matrix)."""
        H = self.lin[3]
        keep = ~self.mc.held
        Hk = H[np.ix_(keep, keep)]
        if how == "inv":
            Ck = np.linalg.inv(Hk)
        else:
            d = 1.0 / np.sqrt(np.diag(Hk))
            Li = np.linalg.inv(np.linalg.cholesky(Hk * d[:, None] * d[None, :]))
            Ck = (Li.T @ Li) * d[:, None] * d[None, :]
        Cv = np.zeros_like(H)
        Cv[np.ix_(keep, keep)] = Ck
        return Cv

    def position(self, offset):
        """The chain-vector position of the block at an extended offset; -1: a block without columns (constant, or a camera with
        mask 0): zeros.  Unreferenced blocks are the caller's to avoid."""
        at = np.flatnonzero(self.ext_of == offset)
        return int(at[0]) if at.size else -1

    def block(self, Cv, off_a, off_b):
        pa, pb = self.position(off_a), self.position(off_b)
        if pa < 0 or pb < 0:
            return np.zeros((6, 6))
        return Cv[pa:pa + 6, pb:pb + 6].copy()

    def held6(self, offset):
        """bool [6]: the held components of the block at the offset (all False for a block without columns)."""
        p = self.position(offset)
        return self.mc.held[p:p + 6].copy() if p >= 0 else np.zeros(6, bool)
