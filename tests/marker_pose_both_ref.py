"""TEST INFRASTRUCTURE: numpy restatement of the planar marker's second pose (csrc/ba_marker_pose.hpp: MirrorMarkerPose,
FitMarkerPoseBoth), the checker for rsba_marker_pose_from_corners_both, rsba_marker_poses_from_corners_both and the flagged starts.
Only tests and tools import it.

  mirror      R' = (I - 2 v v') R diag(1, 1, -1), t' = t with v = t / |t|: by numpy's matrix products and marker_pose_ref's
              rvec_from_matrix (the product: scalars, its own RotationMatrixToRvec)
  solution 1  marker_pose_ref.fit(start=mirror(solution 0)): the reference's complex-step Jacobian and LAPACK solve
  same        the largest difference of an entry of the two rotation matrices or translations below SAME_BELOW (the product's definition)

The "ambiguous" set: small, nearly frontal markers (tilt 5-30 degrees, depth 0.8-1.5 m, 0.3 px noise, side 0.05, fx = fy = 620), where
the homography start falls into the mirror image's basin in about a quarter of the cases.  The set checks itself (ambiguous_reference):
a test that passes on a set where nothing is ambiguous shows nothing.
"""
import numpy as np

import marker_pose_ref as mp

SAME_BELOW = 1e-5
STATUS_SAME = 3
AMBIGUOUS_N = 60
AMBIGUOUS_SEED = 1
AMBIGUOUS_INTR = np.array([620.0, 620.0, 320.0, 240.0])
_CACHE = {}


def mirror(pose):
    pose = np.asarray(pose, float)
    R, t = mp._rodrigues(pose[:3]), pose[3:]
    v = t / np.linalg.norm(t)
    Rm = (np.eye(3) - 2.0 * np.outer(v, v)) @ R @ np.diag([1.0, 1.0, -1.0])
    return np.concatenate([mp.rvec_from_matrix(Rm), t]), Rm


def fit_both(corners8, intr, dist, side):
    """-> (poses 2 x 6, rms 2, status 2): the contract of FitMarkerPoseBoth."""
    p0, e0, s0, _ = mp.fit(corners8, intr, dist, side)
    poses, rms, status = np.zeros((2, 6)), np.array([e0, -1.0]), np.array([s0, 2])
    poses[0] = p0
    if s0 > 1:
        return poses, rms, status
    start, _ = mirror(p0)
    if not np.all(np.isfinite(start)):
        return poses, rms, status
    p1, e1, s1, _ = mp.fit(corners8, intr, dist, side, start=start)
    if s1 > 1:
        return poses, rms, status
    if mp.pose_distance(p0, p1) < SAME_BELOW:
        status[1] = STATUS_SAME
        return poses, rms, status
    poses[1], rms[1], status[1] = p1, e1, s1
    return poses, rms, status


def ambiguous_set(n=AMBIGUOUS_N, seed=AMBIGUOUS_SEED, side=mp.SIDE, noise=0.3):
    """(corners n x 8, true poses n x 6): marker_pose_ref.synthetic's construction with tilt 5-30 degrees and depth 0.8-1.5 m."""
    key = ("set", n, seed, side, noise)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        corners, poses = np.zeros((n, 8)), np.zeros((n, 6))
        for i in range(n):
            a = rng.uniform(0, 2 * np.pi)
            axis = np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2)])
            axis /= np.linalg.norm(axis)
            tilt = np.radians(rng.uniform(5, 30))
            spin = rng.uniform(-np.pi, np.pi)
            R = mp._rodrigues(axis * tilt) @ mp._rodrigues(np.array([0, 0, spin])) @ np.diag([1.0, -1.0, -1.0])
            z = rng.uniform(0.8, 1.5)
            t = np.array([rng.uniform(-0.35, 0.35) * z, rng.uniform(-0.25, 0.25) * z, z])
            poses[i] = np.concatenate([mp.rvec_from_matrix(R), t])
            uv, _ = mp.project(poses[i], side, AMBIGUOUS_INTR, None)
            corners[i] = (uv + rng.normal(0, noise, (4, 2))).reshape(-1)
        _CACHE[key] = (corners, poses)
    corners, poses = _CACHE[key]
    return corners.copy(), poses.copy()


def ambiguous_reference():
    """(poses n x 2 x 6, rms n x 2, status n x 2) of the restatement on the ambiguous set, computed once and shared, and the set's check of
    itself: at most 1 detection in 20 lacks a distinct second solution, and in at least 10 of the 60 solution 1 is the nearer to the
    truth — the homography start's basin is the wrong one there."""
    if "ref" not in _CACHE:
        corners, truth = ambiguous_set()
        n = len(corners)
        poses, rms, status = np.zeros((n, 2, 6)), np.zeros((n, 2)), np.zeros((n, 2), int)
        for i in range(n):
            poses[i], rms[i], status[i] = fit_both(corners[i], AMBIGUOUS_INTR, None, mp.SIDE)
        have = status[:, 1] <= 1
        nearer = np.array([have[i] and mp.pose_distance(poses[i, 1], truth[i]) < mp.pose_distance(poses[i, 0], truth[i]) for i in range(n)])
        assert np.all(status[:, 0] <= 1), status[:, 0]
        assert (~have).sum() * 20 <= n, (~have).sum()
        assert nearer.sum() >= 10, nearer.sum()
        _CACHE["ref"] = (poses, rms, status, nearer)
    poses, rms, status, nearer = _CACHE["ref"]
    return poses.copy(), rms.copy(), status.copy(), nearer.copy()


# ------------------------------------------------------------------ the crafted block: two detections, two cameras, both own fits mirrored
CRAFTED_SEED, CRAFTED_TIME, CRAFTED_ROWS, CRAFTED_SIDE = 0, 0, (0, 5), 0.05


def own_truth(prob, i):
    """The true pose of detection i's marker in its camera: camera o time o marker of the truth."""
    C, T = prob["C"], prob["T"]
    tr = np.asarray(prob["truth"], float).reshape(-1, 6)
    cam, tim, mar = tr[prob["c"][i]], tr[C + prob["t"][i]], tr[C + T + prob["m"][i]]
    Rc, Rt = mp._rodrigues(cam[:3]), mp._rodrigues(tim[:3])
    return np.concatenate([mp.rvec_from_matrix(Rc @ Rt @ mp._rodrigues(mar[:3])), Rc @ (Rt @ mar[3:] + tim[3:]) + cam[3:]])


def crafted_rig(seed=CRAFTED_SEED, time=CRAFTED_TIME, rows=CRAFTED_ROWS, side=CRAFTED_SIDE, noise_px=0.3):
    """3 cameras x 4 times x 4 markers of 5 cm at 1.2-2.4 m (15-25 pixels, nearly frontal), every pair detected, except that time `time`
    keeps two detections only, from two cameras: `rows` of the full problem, chosen (searched on the CPU with
    rsba_marker_pose_from_corners_both) so that the own fit of BOTH is the mirror image.  Cameras and markers sit at the truth and are
    given; the times are zeroed and to be fitted.  -> (problem, flags over C + T + M, the crafted time's block index)."""
    from realsensecalibration_amd import synthetic as syn
    full = syn.make_marker_chain(3, 4, 4, seed=seed, keep=1.0, marker_side=side, noise_px=noise_px)
    t = np.asarray(full["t"])
    mask = t != time
    mask[list(rows)] = True
    assert all(t[r] == time for r in rows) and len({int(full["c"][r]) for r in rows}) == 2
    prob = dict(full)
    for k in ("t", "c", "m", "obs"):
        prob[k] = np.ascontiguousarray(np.asarray(full[k])[mask])
    prob["N"] = int(mask.sum())
    C, T, M = prob["C"], prob["T"], prob["M"]
    blocks = np.asarray(full["truth"], float).reshape(-1, 6).copy()
    blocks[C:C + T] = 0.0
    prob["params"] = blocks.ravel()
    return prob, [1] * C + [0] * T + [1] * M, C + time


def write_start_file(path, prob, model, known, sweeps, refits=()):
    """The `start` file of tests/marker_pose_both_driver.cpp; refits: (block, six values) pairs."""
    C, T, M, N = prob["C"], prob["T"], prob["M"], prob["N"]
    dist = prob.get("dist")
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, float).ravel())   # noqa: E731
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %r %d %d\n" % (1 if model == 2 else 0, C, T, M, N, 0 if dist is None else 1, float(prob["marker_side"]), sweeps,
                                                   0 if known is None else 1))
        f.write(num(prob["intr"]) + "\n")
        if dist is not None:
            f.write(num(dist) + "\n")
        f.write(num(prob["params"]) + "\n")
        if known is not None:
            f.write(" ".join(str(int(v)) for v in known) + "\n")
        for i in range(N):
            f.write("%d %d %d %s\n" % (prob["c"][i], prob["t"][i], prob["m"][i], num(prob["obs"][i])))
        f.write("%d\n" % len(refits))
        for block, value in refits:
            f.write("%d %s\n" % (block, num(value)))
