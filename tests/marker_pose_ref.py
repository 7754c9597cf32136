"""TEST INFRASTRUCTURE: numpy restatement of the single-marker pose fit (csrc/ba_marker_pose.hpp), the checker for
rsba_marker_pose_from_corners, rsba_marker_poses_from_corners and rsba_problem_initial_time_poses.  Only tests and tools import it.

What aruco::estimatePoseSingleMarkers does for one detection (Main_Calibration/correspondencer.cpp:80): the pose of a square
marker of side s from its four image corners, as the local minimiser of the corners' reprojection error reached from the
homography of the square (SOLVEPNP_ITERATIVE on a planar target).  Deliberately NOT the product's arithmetic:
  homography        the 8 x 9 DLT's null vector by LAPACK's SVD       (product: the closed form of the square-to-quad map)
  nearest rotation  U V' of LAPACK's SVD                               (product: the symmetric orthonormalisation, closed form)
  Jacobian          complex-step differentiation of the projection    (product: the analytic rows of ba_math.hpp)
  normal equations  numpy.linalg.solve                                 (product: a 6 x 6 Cholesky in registers)
The Levenberg-Marquardt rules are the shared contract: damping lambda diag(J'J), lambda0 = 1e-3, a candidate is accepted when the
cost does not rise, lambda /= 10 (floor 1e-15) on acceptance and *= 10 on rejection, stop when the step's max-norm is below
1e-12 (1 + max |p|), at most MAX_ITERATIONS steps.  Status: 0 converged, 1 the cap was reached, 2 degenerate (pose zeros, rms -1).
"""
import numpy as np

MAX_ITERATIONS = 400
SYNTH_DIST = np.array([-0.28, 0.09, 1e-3, -5e-4, -0.01])


def object_points(side):
    h = side / 2.0
    return np.array([[-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [-h, -h, 0.0]])


def _rodrigues(w):
    """R(w) for real or complex w (complex: the complex-step derivative's argument; no modulus is taken anywhere)."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    K = np.array([[0 * w[0], -w[2], w[1]], [w[2], 0 * w[0], -w[0]], [-w[1], w[0], 0 * w[0]]])
    if abs(th2) < 1e-24:
        return np.eye(3) + K
    th = np.sqrt(th2)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th2) * (K @ K)


def rvec_from_matrix(R):
    """Angle-axis of a rotation matrix through the quaternion (stable at every angle below pi)."""
    q = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if q[0] < 1e-3 * 4:    # near pi: the largest diagonal element's row
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        v = np.zeros(3)
        v[i] = 1 + R[i, i] - R[j, j] - R[k, k]
        v[j] = R[j, i] + R[i, j]
        v[k] = R[k, i] + R[i, k]
        q = np.concatenate([[R[k, j] - R[j, k]], v])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    return np.zeros(3) if s < 1e-300 else q[1:] / s * (2 * np.arctan2(s, q[0]))


def distort(x, y, k):
    r2 = x * x + y * y
    rad = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    return x * rad + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x), y * rad + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y


def project(pose, side, intr, dist):
    """The four corners' pixels (4 x 2) under the project's camera model; also the depths."""
    pc = object_points(side) @ _rodrigues(pose[:3]).T + pose[3:]
    x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    if dist is not None:
        x, y = distort(x, y, dist)
    return np.stack([intr[0] * x + intr[2], intr[1] * y + intr[3]], 1), pc[:, 2]


def undistort_normalised(corners, intr, dist):
    """(u, v) -> the normalised point of the ideal pinhole camera, rsba_undistort_points' fixed-point iteration; None when it does
    not converge."""
    xd, yd = (corners[:, 0] - intr[0 + 2]) / intr[0], (corners[:, 1] - intr[3]) / intr[1]
    if dist is None or not np.any(dist):
        return np.stack([xd, yd], 1)
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(54):
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        if not np.all(rad > 0):
            return None
        xn = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad
        yn = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
        if not (np.all(np.isfinite(xn)) and np.all(np.isfinite(yn))):
            return None
        moved = max(np.abs(xn - x).max(), np.abs(yn - y).max())
        x, y = xn, yn
        if moved == 0.0:
            break
    return np.stack([x, y], 1) if moved < 1e-14 else None


def homography_start(corners8, intr, dist, side):
    """The start of the fit: DLT homography of the square -> (rvec, tvec); None when degenerate."""
    c = np.asarray(corners8, float).reshape(4, 2)
    n = undistort_normalised(c, intr, dist)
    if n is None:
        return None
    obj = object_points(side)
    A = np.zeros((8, 9))
    for i in range(4):
        X, Y = obj[i, 0], obj[i, 1]
        x, y = n[i]
        A[2 * i] = [X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x]
        A[2 * i + 1] = [0, 0, 0, X, Y, 1, -y * X, -y * Y, -y]
    # (column scaling: the side is ~1e-2, the third column 1)
    sc = np.array([side, side, 1.0] * 3)
    _, sv, Vt = np.linalg.svd(A * sc)
    if not sv[7] > 1e-9 * sv[0]:
        return None
    H = (Vt[8] * sc).reshape(3, 3)
    depth = obj[:, :2] @ H[2, :2] + H[2, 2]
    if depth.sum() < 0:
        H, depth = -H, -depth
    if not np.all(depth > 1e-9 * depth.max()):
        return None
    n1, n2 = np.linalg.norm(H[:, 0]), np.linalg.norm(H[:, 1])
    if not (n1 > 0 and n2 > 0):
        return None
    r1, r2 = H[:, 0] / n1, H[:, 1] / n2
    t = 2 * H[:, 2] / (n1 + n2)
    if np.linalg.norm(np.cross(r1, r2)) < 1e-9 or not np.all(np.isfinite(t)) or not t[2] > 0:
        return None
    U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], 1))
    R = U @ Vt
    return np.concatenate([rvec_from_matrix(R), t])


def _residuals(p, c, side, intr, dist):
    uv, z = project(p, side, intr, dist)
    return (uv - c).reshape(-1), z


def fit(corners8, intr, dist, side, start=None):
    """-> (pose6, rms, status, iterations).  start: another starting pose than the homography's (the basin check of the tests)."""
    c = np.asarray(corners8, float).reshape(4, 2)
    intr = np.asarray(intr, float)
    dist = None if dist is None else np.asarray(dist, float)
    bad = (np.zeros(6), -1.0, 2, 0)
    p = homography_start(c, intr, dist, side) if start is None else np.asarray(start, float).copy()
    if p is None:
        return bad
    r, z = _residuals(p, c, side, intr, dist)
    if not (np.all(np.isfinite(r)) and np.all(z > 0)):
        return bad
    cost, lam, status, it = r @ r, 1e-3, 1, 0
    need_j = True
    for it in range(1, MAX_ITERATIONS + 1):
        if need_j:
            J = np.zeros((8, 6))
            for k in range(6):
                pc = p.astype(complex)
                pc[k] += 1e-30j
                J[:, k] = _residuals(pc, c, side, intr, dist)[0].imag / 1e-30
            A, g = J.T @ J, J.T @ r
            need_j = False
        try:
            d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        except np.linalg.LinAlgError:
            d = None
        ok = d is not None and np.all(np.isfinite(d))
        if ok:
            rn, zn = _residuals(p + d, c, side, intr, dist)
            cn = rn @ rn
            ok = np.isfinite(cn) and np.all(zn > 0) and cn <= cost
        if ok:
            small = np.abs(d).max() < 1e-12 * (1 + np.abs(p).max())
            p, r, cost, lam, need_j = p + d, rn, cn, max(lam / 10, 1e-15), True
            if small:
                status = 0
                break
        else:
            if d is not None and np.all(np.isfinite(d)) and np.abs(d).max() < 1e-12 * (1 + np.abs(p).max()):
                status = 0
                break
            lam *= 10
    if not np.all(np.isfinite(p)):
        return bad
    return p, float(np.sqrt(cost / 8)), status, it


def pose_distance(a, b):
    """How far two poses are apart AS POSES: the largest difference of an entry of the rotation matrices or of the translations.
    (A marker that faces the camera is a rotation by nearly pi, where w and -w (2 pi - |w|) / |w| are the same rotation and two
    fits may stop on either side; for poses away from pi this is the difference of the six numbers to first order.)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return max(np.abs(_rodrigues(a[:3]) - _rodrigues(b[:3])).max(), np.abs(a[3:] - b[3:]).max())


# ------------------------------------------------------------------ the synthetic set the CPU and GPU tests share
def synthetic(n, seed, dist=None, intr=(620.0, 620.0, 320.0, 240.0), side=0.05, noise=0.2):
    """n detections: depth 0.25-0.5 m, tilt 25-60 degrees about a mostly in-plane axis, random in-plane spin, corner noise sigma.
    -> (corners n x 8, true poses n x 6).  The marker's centre projects inside a 640 x 480 image."""
    rng = np.random.default_rng(seed)
    intr = np.asarray(intr, float)
    corners, poses = np.zeros((n, 8)), np.zeros((n, 6))
    for i in range(n):
        a = rng.uniform(0, 2 * np.pi)
        axis = np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2)])
        axis /= np.linalg.norm(axis)
        tilt = np.radians(rng.uniform(25, 60))
        spin = rng.uniform(-np.pi, np.pi)
        # the marker faces the camera when its z axis points at it: a half turn about x, then spin and tilt
        R = _rodrigues(axis * tilt) @ _rodrigues(np.array([0, 0, spin])) @ np.diag([1.0, -1.0, -1.0])
        z = rng.uniform(0.25, 0.5)
        t = np.array([rng.uniform(-0.35, 0.35) * z, rng.uniform(-0.25, 0.25) * z, z])
        poses[i] = np.concatenate([rvec_from_matrix(R), t])
        uv, _ = project(poses[i], side, intr, dist)
        corners[i] = (uv + rng.normal(0, noise, (4, 2))).reshape(-1)
    return corners, poses


# Three cameras with different intrinsics (camera 0: the issue's fx = fy = 620) and three sets of coefficients: none, every camera
# distorted, and a mix of zero and non-zero rows.  Detection i belongs to camera i % 3 and is generated with that camera's model.
INTRINSICS3 = np.array([[620.0, 620.0, 320.0, 240.0], [600.0, 605.0, 315.0, 245.0], [640.0, 630.0, 330.0, 235.0]])
DIST3 = {"pinhole": None,
         "distorted": np.stack([SYNTH_DIST, 0.5 * SYNTH_DIST, SYNTH_DIST * [1, 1, -1, -1, 1]]),
         "mixed": np.stack([SYNTH_DIST, np.zeros(5), 0.5 * SYNTH_DIST])}
SIDE = 0.05
# Two reference fits of one detection, from the homography and from the true pose, count as the same minimiser below this: a tenth of the
# 1e-6 parameter bar the product is held to, so that no case can pass that bar from a wrong basin (the other planar solution is ~0.1 rad
# away).  The stopping rule (step < 1e-12 (1 + |p|)) leaves ~1e-9 along the flattest direction.
SAME_MINIMISER = 1e-7
_CACHE = {}


def batch(config, n, noise=0.2):
    """(corners n x 8, camera n int32, intrinsics 3 x 4, dist 3 x 5 or None, true poses n x 6): the first n detections of the set."""
    key = ("batch", config, noise)
    if key not in _CACHE:
        N = 257
        dist = DIST3[config]
        corners, truth = np.zeros((N, 8)), np.zeros((N, 6))
        for c in range(3):
            idx = np.arange(c, N, 3)
            cc, tt = synthetic(len(idx), 100 + 10 * sorted(DIST3).index(config) + c, None if dist is None else dist[c], INTRINSICS3[c], SIDE, noise)
            corners[idx], truth[idx] = cc, tt
        _CACHE[key] = (corners, (np.arange(N) % 3).astype(np.int32), truth)
    corners, cam, truth = _CACHE[key]
    return corners[:n].copy(), cam[:n].copy(), INTRINSICS3.copy(), None if DIST3[config] is None else DIST3[config].copy(), truth[:n].copy()


def reference(config, n):
    """(poses n x 6, rms n) of the reference on batch(config, n); computed once per detection and shared.  Every case is checked to be
    unambiguous: the fit from the homography and the fit from the true pose are the same minimiser, both converged."""
    corners, cam, intr, dist, truth = batch(config, n)
    done = _CACHE.setdefault(("ref", config), {})
    for i in range(n):
        if i not in done:
            d = None if dist is None else dist[cam[i]]
            a = fit(corners[i], intr[cam[i]], d, SIDE)
            b = fit(corners[i], intr[cam[i]], d, SIDE, start=truth[i])
            assert a[2] == 0 and b[2] == 0, (config, i, a, b)
            assert pose_distance(a[0], b[0]) < SAME_MINIMISER, (config, i, pose_distance(a[0], b[0]))
            done[i] = (a[0], a[1])
    return np.stack([done[i][0] for i in range(n)]), np.array([done[i][1] for i in range(n)])
