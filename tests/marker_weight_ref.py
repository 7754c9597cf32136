"""The numpy reference of tests/marker_loss_ref.py with per-observation weights (ceres::ScaledLoss around each block's loss).

Block i contributes 1/2 a_i rho(s_i); rho'' <= 0 still holds, so the corrector scales the block's rows by sqrt(a_i rho'(s_i)).  The raw
sum of squares is not weighted.  Everything else — residuals, Jacobians, the minimiser, the covariance — is the parent's.
"""
import numpy as np

import marker_loss_ref as ref


class WeightedMarkerChain(ref.MarkerChain):
    def __init__(self, prob, weights, variant=0, loss="none", a=0.0, constant_blocks=()):
        super().__init__(prob, variant, loss, a, constant_blocks)
        self.w = np.asarray(weights, float).copy()
        assert self.w.shape == (self.N,) and np.all(self.w >= 0.0) and np.all(np.isfinite(self.w))

    def weighted(self, s):
        rho, rho1 = ref.rho_and_rho1(s, self.loss, self.a)
        return self.w * rho, self.w * rho1

    def cost(self, x):
        r = self.residuals(self.full(x))
        s = np.sum(r * r, axis=1)
        rho, _ = self.weighted(s)
        return 0.5 * float(np.sum(rho)), float(np.sum(s))

    def linearise(self, x):
        full = self.full(x)
        r = self.residuals(full)
        J = self.jacobians(full)
        s = np.sum(r * r, axis=1)
        rho, rho1 = self.weighted(s)
        sq = np.sqrt(rho1)
        rt, Jt = r * sq[:, None], J * sq[:, None, None]
        n = self.n
        cl = np.where(self.cols >= 0, self.cols, n)             # a dump row / column n for the absent ones
        Hb = np.einsum("kra,krb->kab", Jt, Jt)
        gb = np.einsum("kra,kr->ka", Jt, rt)
        Hx = np.zeros((n + 1, n + 1))
        np.add.at(Hx, (cl[:, :, None], cl[:, None, :]), Hb)
        gx = np.zeros(n + 1)
        np.add.at(gx, cl, gb)
        return 0.5 * float(np.sum(rho)), rt, Jt, Hx[:n, :n], gx[:n], float(np.sum(s))


def hit_rows(clean, displaced):
    """The rows (residual blocks) of which marker_loss_ref.displace_corners moved a corner."""
    a = np.asarray(clean["obs"], float).reshape(-1, 8)
    b = np.asarray(displaced["obs"], float).reshape(-1, 8)
    return np.any(a != b, axis=1)


def mask_of(hit):
    """Weight 0 on the hit rows, 1 elsewhere."""
    return np.where(hit, 0.0, 1.0)


def select_rows(prob, index):
    """prob with the rows `index` (an index array: rows may repeat) and everything else as it was."""
    out = dict(prob)
    for k in ("t", "c", "m"):
        out[k] = np.asarray(prob[k])[index]
    out["obs"] = np.asarray(prob["obs"], float).reshape(-1, 8)[index]
    out["N"] = int(out["obs"].shape[0])
    return out


# ---- the cases tests/test_marker_weight_ref_cpu.py pins and tests/test_gpu_marker_weights.py solves on the device
RIG_SEEDS = {(4, 40, 6): 50, (12, 40, 20): 112, (8, 400, 16): 464}


def rig(shape):
    """A synthetic rig (its seed above) with 5 % of its corners 40 px off, displace_corners' seed C T M -> (clean, displaced)."""
    from realsensecalibration_amd import synthetic as syn
    C, T, M = shape
    clean = syn.make_marker_chain(C, T, M, seed=RIG_SEEDS[shape])
    return clean, ref.displace_corners(clean, 0.05, 40.0, C * T * M)


def _hongo():
    clean = ref.hongo()
    return clean, ref.displace_corners(clean, 0.05, 30.0, 11)


def _test2():
    clean = ref.test2()
    return clean, ref.displace_corners(clean, 0.05, 25.0, 12)


def _const_rig():
    from realsensecalibration_amd import synthetic as syn
    clean = syn.make_marker_chain(4, 30, 6, seed=31)
    return clean, ref.displace_corners(clean, 0.05, 40.0, 31)


def _fractions(seed, n):
    return np.random.default_rng(seed).choice([0.25, 1.0, 4.0], n)


def case(name):
    """-> dict(prob, variant, weights, loss, a, constant_blocks, hit): variant 0 Main_Calibration's wiring, 1 Test2's."""
    const = ()
    variant = 0
    if name.startswith("hongo"):
        clean, prob = _hongo()
    elif name.startswith("test2"):
        clean, prob = _test2()
        variant = 1
    elif name.startswith("const"):
        clean, prob = _const_rig()
        const = (2, prob["C"] + 5, prob["C"] + prob["T"] + 3)
    else:
        clean, prob = rig(tuple(int(v) for v in name.split("_")[0].split("x")))
    hit = hit_rows(clean, prob)
    mask = mask_of(hit)
    kind = name.split("_", 1)[1]
    if kind == "mask_none":
        w, loss, a = mask, "none", 0.0
    elif kind == "mask_huber":
        w, loss, a = mask, "huber", 2.0
    elif kind == "mask_cauchy":
        w, loss, a = mask, "cauchy", 1.5
    elif kind == "frac_huber":
        w, loss, a = _fractions(5 if name.startswith("hongo") else 6, prob["N"]), "huber", 2.0
    elif kind == "fracmask_cauchy":
        w, loss, a = _fractions(6, prob["N"]) * mask, "cauchy", 2.0
    elif kind == "time7_huber":
        w, loss, a = np.where(np.asarray(prob["t"]) == 7, 0.0, mask), "huber", 2.0
    else:
        raise ValueError(name)
    return dict(prob=prob, variant=variant, weights=w, loss=loss, a=a, constant_blocks=const, hit=hit)


# the issue's table, then the shapes the device test adds
TABLE = ["hongo_mask_none", "hongo_mask_huber", "hongo_frac_huber", "test2_mask_cauchy", "4x40x6_mask_none", "4x40x6_frac_huber",
         "4x40x6_fracmask_cauchy", "4x40x6_time7_huber"]
EXTRA = ["4x40x6_mask_huber", "12x40x20_mask_none", "8x400x16_mask_huber", "const_mask_huber"]

_RUNS = {}


def reference_run(name):
    """(case, chain, summary, rows, final (C + T + M, 6)) of the weighted reference's minimisation, once per process."""
    if name not in _RUNS:
        cs = case(name)
        mc = WeightedMarkerChain(cs["prob"], cs["weights"], cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
        x, summary, rows = ref.minimise(mc)
        _RUNS[name] = (cs, mc, summary, rows, mc.full(x))
    return _RUNS[name]
