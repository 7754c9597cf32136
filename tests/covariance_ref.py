"""numpy reference of ceres::Covariance for the point model: the dense Jacobian from the oracle's per-observation blocks, put
through the loss corrector as the solve does (sqrt(rho') on J; Huber and Cauchy have rho'' <= 0, so Ceres' corrector keeps only
that term), the columns of constant and unreferenced blocks dropped, then inv(J'J)."""
import numpy as np


def sqrt_rho1(sq_norm, huber_delta=0.0, cauchy=False):
    """sqrt(rho'(s)) of ceres::HuberLoss(a) / CauchyLoss(a) at s = |r|^2 (1 without a loss)."""
    if huber_delta <= 0.0:
        return 1.0
    if cauchy:
        return np.sqrt(1.0 / (1.0 + sq_norm / huber_delta ** 2))
    return 1.0 if sq_norm <= huber_delta ** 2 else np.sqrt(huber_delta / np.sqrt(sq_norm))


def point_jacobian(oracle, prob, params, huber_delta=0.0, cauchy=False):
    """Dense corrected Jacobian (2N x (6C + 3P)) of the point model at params."""
    C, N = prob["C"], prob["N"]
    J = np.zeros((2 * N, len(params)))
    intr = prob["intr"].reshape(-1, 4)
    for i in range(N):
        c, p = int(prob["cam_idx"][i]), int(prob["pt_idx"][i])
        r, jc, jp = oracle.point_residual_jacobian(params[6 * c:6 * c + 6], params[6 * C + 3 * p:6 * C + 3 * p + 3], intr[c],
                                                   prob["obs"][2 * i:2 * i + 2])
        s = sqrt_rho1(float(r @ r), huber_delta, cauchy)
        J[2 * i:2 * i + 2, 6 * c:6 * c + 6] = s * jc
        J[2 * i:2 * i + 2, 6 * C + 3 * p:6 * C + 3 * p + 3] = s * jp
    return J


def point_covariance(oracle, prob, params, constant_cameras=(), constant_points=(), huber_delta=0.0, cauchy=False):
    """-> (cov, keep, kappa): cov = inv(J'J) over the kept columns, keep = the parameter indices of those columns, kappa = the
    condition number of J'J."""
    C, P = prob["C"], prob["P"]
    J = point_jacobian(oracle, prob, params, huber_delta, cauchy)
    ref_cam = np.zeros(C, bool); ref_cam[prob["cam_idx"]] = True
    ref_pt = np.zeros(P, bool); ref_pt[prob["pt_idx"]] = True
    for c in constant_cameras:
        ref_cam[c] = False
    for p in constant_points:
        ref_pt[p] = False
    keep = np.concatenate([np.repeat(ref_cam, 6), np.repeat(ref_pt, 3)]).nonzero()[0]
    H = J[:, keep].T @ J[:, keep]
    return np.linalg.inv(H), keep, np.linalg.cond(H)


def block(cov, keep, offset_a, na, offset_b, nb):
    """The (na x nb) block of the parameters at offsets a and b out of the kept-column covariance."""
    pos = {int(k): i for i, k in enumerate(keep)}
    ia = [pos[offset_a + t] for t in range(na)]
    ib = [pos[offset_b + t] for t in range(nb)]
    return cov[np.ix_(ia, ib)]


def marker_jacobian(oracle, prob, params, variant, marker_side, intr):
    """Dense Jacobian (8N x 6(C + T + M)) of the marker-chain models at params (no loss).  variant 0: camera 0 and marker 0 are the
    fixed base blocks (bundle_adjustment_manager.cpp); 1 (Test2): camera 0 only."""
    C, T, N = prob["C"], prob["T"], prob["N"]
    intr = np.asarray(intr, float).reshape(-1, 4)
    J = np.zeros((8 * N, len(params)))
    for i in range(N):
        c, t, m = int(prob["c"][i]), int(prob["t"][i]), int(prob["m"][i])
        cb, tb, mb = c, C + t, C + T + m
        cam = params[6 * cb:6 * cb + 6] if c != 0 else None
        mar = params[6 * mb:6 * mb + 6] if (variant == 1 or m != 0) else None
        _, j = oracle.marker_residual_jacobian(cam, params[6 * tb:6 * tb + 6], mar, marker_side, intr[c], np.ravel(prob["obs"])[8 * i:8 * i + 8])
        if cam is not None:
            J[8 * i:8 * i + 8, 6 * cb:6 * cb + 6] = j[:, 0:6]
        J[8 * i:8 * i + 8, 6 * tb:6 * tb + 6] = j[:, 6:12]
        if mar is not None:
            J[8 * i:8 * i + 8, 6 * mb:6 * mb + 6] = j[:, 12:18]
    return J


def marker_covariance(oracle, prob, params, variant, marker_side, intr, constant_blocks=()):
    """-> (cov, keep, kappa) over the blocks some residual references, less the constant ones."""
    J = marker_jacobian(oracle, prob, params, variant, marker_side, intr)
    nb = len(params) // 6
    used = np.array([np.any(J[:, 6 * b:6 * b + 6] != 0.0) for b in range(nb)])
    used[list(constant_blocks)] = False
    keep = np.repeat(used, 6).nonzero()[0]
    H = J[:, keep].T @ J[:, keep]
    return np.linalg.inv(H), keep, np.linalg.cond(H)
