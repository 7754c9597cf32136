"""A numpy reference for the marker-chain models with lens distortion (OpenCV's five coefficients k1 k2 p1 p2 k3).

It shares no code with the product.  `MarkerChainDist` is `marker_loss_ref.MarkerChain` with ONE method replaced, `residuals()`:
the corner in the detecting camera's frame (X, Y, Z) goes through

    x = X / Z, y = Y / Z, r2 = x^2 + y^2,  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
    xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y,  u = fx xd + ppx, v = fy yd + ppy

(cv::projectPoints with a 5 x 1 distCoeffs), written with + and * only, so it is complex-safe: every Jacobian, `linearise`,
`minimise`, the covariance and the weights of the existing reference modules run on it unchanged (complex step).
The coefficients are per camera index, indexed as the intrinsics are (the detecting camera).
"""
import numpy as np

import marker_loss_ref as ref
import marker_weight_ref as wref

WIDTH, HEIGHT = 640, 480


class MarkerChainDist(ref.MarkerChain):
    def __init__(self, prob, dist, variant=0, loss="none", a=0.0, constant_blocks=()):
        super().__init__(prob, variant=variant, loss=loss, a=a, constant_blocks=constant_blocks)
        self.dist = np.asarray(dist, float).reshape(self.C, 5)

    def residuals(self, full):
        """(N, 8) residuals at the (C + T + M, 6) poses (complex allowed): MarkerChain.residuals' chain, then the distorted projection."""
        N, C, T, h = self.N, self.C, self.T, self.h
        corners = np.array([[-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [-h, -h, 0.0]])
        p = np.tile(corners, (N, 1)).astype(full.dtype)
        rep = lambda v: np.repeat(v, 4)   # noqa: E731
        mar, tim, cam = full[C + T + rep(self.m)], full[C + rep(self.t)], full[rep(self.c)]
        p = np.where(rep(self.has_mar)[:, None], ref._rotate(mar[:, :3], p) + mar[:, 3:], p)
        p = ref._rotate(tim[:, :3], p) + tim[:, 3:]
        p = np.where(rep(self.has_cam)[:, None], ref._rotate(cam[:, :3], p) + cam[:, 3:], p)
        K = self.intr[rep(self.c)]
        o = self.obs.reshape(-1, 2)
        # fx xd = (fx X / Z) rad + fx (tangential terms): with zero coefficients the first product is MarkerChain's own fx X / Z times
        # one and the second an exact zero, so the residuals are that class's bit for bit
        d = self.dist[rep(self.c)]
        k1, k2, p1, p2, k3 = (d[:, i] for i in range(5))
        x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        u = (K[:, 0] * p[:, 0] / p[:, 2]) * rad + K[:, 0] * (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)) + K[:, 2] - o[:, 0]
        v = (K[:, 1] * p[:, 1] / p[:, 2]) * rad + K[:, 1] * (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y) + K[:, 3] - o[:, 1]
        return np.stack([u, v], axis=1).reshape(N, 8)


def coefficients(C, seed):
    """Realistic per-camera sets for a 640 x 480 image with fx ~ 600: k1 in [-0.30, 0.15], k2 in +-0.10, p1 and p2 in +-2e-3, k3 in
    +-0.05; camera 0 all zeros, camera 1 tangential only, camera 2 k3 only.  No fold-over: rad > 0.5 over the whole image."""
    rng = np.random.default_rng([seed, 0xD157])
    d = np.stack([rng.uniform(-0.30, 0.15, C), rng.uniform(-0.10, 0.10, C), rng.uniform(-2e-3, 2e-3, C), rng.uniform(-2e-3, 2e-3, C),
                  rng.uniform(-0.05, 0.05, C)], axis=1)
    d[0] = 0.0
    if C > 1:
        d[1, [0, 1, 4]] = 0.0
    if C > 2:
        d[2, :4] = 0.0
    # the image corners of the widest camera the generator makes (fx >= 600, principal point within 35 px of the middle)
    r2 = ((WIDTH / 2 + 35) / 600.0) ** 2 + ((HEIGHT / 2 + 35) / 600.0) ** 2
    for t in np.linspace(0.0, r2, 65):
        rad = 1.0 + t * (d[:, 0] + t * (d[:, 1] + t * d[:, 4]))
        assert (rad > 0.5).all(), (t, rad)
    return d


def redetect(prob, dist, noise_px, seed):
    """A copy of prob whose detections are prob["truth"] projected through the distorted model plus Gaussian noise (the generator's own
    detections are pinhole): a problem whose start is consistent with the coefficients.  Rows, wiring and start stay."""
    out = dict(prob)
    out["obs"] = np.zeros_like(np.asarray(prob["obs"], float))
    mc = MarkerChainDist(out, dist)
    proj = mc.residuals(np.asarray(prob["truth"], float).reshape(-1, 6))   # observations are zero: the projection itself
    rng = np.random.default_rng([seed, 0x0B5E])
    out["obs"] = proj + rng.normal(0.0, noise_px, proj.shape) if noise_px > 0.0 else proj
    out["dist"] = np.asarray(dist, float).reshape(-1, 5).copy()
    return out


def rms(mc, x):
    """ReprojectionCheck's RMS per coordinate at x (raw residuals)."""
    _, sumsq = mc.cost(x)
    return float(np.sqrt(sumsq / (8 * mc.N)))


class WeightedMarkerChainDist(MarkerChainDist, wref.WeightedMarkerChain):
    """The distorted residuals under marker_weight_ref's weighted cost and rows (its cost() and linearise(), unchanged)."""

    def __init__(self, prob, dist, weights, variant=0, loss="none", a=0.0, constant_blocks=()):
        wref.WeightedMarkerChain.__init__(self, prob, weights, variant, loss, a, constant_blocks)
        self.dist = np.asarray(dist, float).reshape(self.C, 5)


# ---- the whole-solve cases tests/test_marker_distortion_ref_cpu.py pins and tests/test_gpu_marker_distortion.py solves on the device.
# Synthetic rigs are redetected (0.3 px noise) with coefficients(C, seed); the fixtures keep their committed detections.
SOLVE_CASES = ["4x40x6", "test2wiring_3x60x4", "hongo", "test2", "4x40x6_huber", "4x40x6_weights", "4x40x6_const"]
RIG_SEED, COEFF_SEED = 50, 1


def case(name):
    """-> dict(prob (with "dist"), dist, variant, loss, a, weights (or None), constant_blocks)."""
    from realsensecalibration_amd import synthetic as syn
    variant, loss, a, weights, const = 0, "none", 0.0, None, ()
    if name == "hongo":
        prob = ref.hongo()
        dist = coefficients(prob["C"], COEFF_SEED)
        prob["dist"] = dist
    elif name == "test2":
        prob, variant = ref.test2(), 1
        dist = coefficients(prob["C"], COEFF_SEED + 1)
        dist[0] = dist[1] * 0.5   # (two cameras: camera 0 would be all zeros and camera 1 tangential only; give both something)
        prob["dist"] = dist
    elif name == "test2wiring_3x60x4":
        variant = 1
        dist = coefficients(3, COEFF_SEED)
        prob = redetect(syn.make_marker_chain(3, 60, 4, seed=RIG_SEED + 1), dist, 0.3, 2)
    else:
        dist = coefficients(4, COEFF_SEED)
        prob = redetect(syn.make_marker_chain(4, 40, 6, seed=RIG_SEED), dist, 0.3, 1)
        kind = name.split("_", 1)[1] if "_" in name else ""
        if kind == "huber":
            prob = dict(ref.displace_corners(prob, 0.05, 40.0, 4 * 40 * 6), dist=dist)
            loss, a = "huber", 2.0
        elif kind == "weights":
            weights = np.random.default_rng(7).choice([0.0, 0.25, 1.0, 4.0], prob["N"])
        elif kind == "const":
            const = (2, prob["C"] + 5, prob["C"] + prob["T"] + 3)
        elif kind:
            raise ValueError(name)
    return dict(prob=prob, dist=dist, variant=variant, loss=loss, a=a, weights=weights, constant_blocks=const)


def chain_of(cs, prob=None):
    prob = cs["prob"] if prob is None else prob
    if cs["weights"] is not None:
        return WeightedMarkerChainDist(prob, cs["dist"], cs["weights"], cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
    return MarkerChainDist(prob, cs["dist"], cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])


_RUNS = {}


def reference_run(name):
    """(case, chain, summary, rows, final (C + T + M, 6)) of the reference's minimisation, once per process."""
    if name not in _RUNS:
        cs = case(name)
        mc = chain_of(cs)
        x, summary, rows = ref.minimise(mc)
        _RUNS[name] = (cs, mc, summary, rows, mc.full(x))
    return _RUNS[name]


def zero_noise_problem():
    """4 x 40 x 6 redetected without noise: the truth is the minimum of the distorted model, and not of the pinhole one."""
    from realsensecalibration_amd import synthetic as syn
    base = syn.make_marker_chain(4, 40, 6, seed=RIG_SEED)
    dist = coefficients(4, COEFF_SEED)
    return redetect(base, dist, 0.0, 1), dist, np.asarray(base["truth"], float).reshape(-1, 6)
