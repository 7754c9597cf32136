"""The numpy restatement of the single-marker pose fit (tests/marker_pose_ref.py) held to the fixture, on its own: the six time rows of
the committed hongo correspondence.txt are what the reference's aruco::estimatePoseSingleMarkers and correspondencer.cpp:100-127 wrote,
printed to six significant digits — the bar tests/test_initial_guess.py uses for printed digits is 2e-5."""
import os
import sys

import numpy as np

import marker_pose_ref as mp
import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, "oracle"))
import initial_guess_oracle as ig  # noqa: E402


def hongo_time_rows(fit_one):
    """The six base poses from camera 0's first detection per time; fit_one(row index, corners8, intrinsics4) -> pose6."""
    ref = ol.read_correspondence(os.path.join(ol.GOLDEN, "hongo", "correspondence.txt"))
    intr = ol.read_intrinsics(ol.SERIALS_MAIN[:1])[0]
    P, O, Cn, T = ref["params"].reshape(-1, 6), ref["obs"].reshape(-1, 8), ref["C"], ref["T"]
    rows, used = np.zeros((T, 6)), []
    for t in range(T):
        seen = [i for i in range(ref["N"]) if ref["t"][i] == t and ref["c"][i] == 0]
        i = min(seen, key=lambda k: ref["m"][k])
        assert i == seen[0]                      # the file lists a camera's detections by marker index
        pose, m = fit_one(i, O[i], intr), ref["m"][i]
        rows[t] = pose if m == 0 else ig.base_pose_from_marker_detection(pose, P[Cn + T + m])
        used.append(i)
    return rows, P[Cn:Cn + T], used


def test_the_reference_reproduces_the_committed_time_rows():
    def fit_one(i, corners, intr):
        pose, rms, status, _ = mp.fit(corners, intr, None, ol.MARKER_SIDE_MAIN)
        assert status == 0 and 0 <= rms < 1.0, (i, status, rms)
        return pose
    rows, committed, used = hongo_time_rows(fit_one)
    assert len(used) == 6
    dev = np.abs(rows - committed).max()
    print("largest deviation from the committed time rows: %.3g" % dev)
    assert dev < 2e-5, dev


def test_the_reference_recovers_exact_poses_and_flags_degenerate_corners():
    for config in mp.DIST3:
        corners, cam, intr, dist, truth = mp.batch(config, 12, noise=0.0)
        for i in range(12):
            pose, rms, status, _ = mp.fit(corners[i], intr[cam[i]], None if dist is None else dist[cam[i]], mp.SIDE)
            assert status == 0 and rms < 1e-8 and mp.pose_distance(pose, truth[i]) < 1e-8
    k = mp.INTRINSICS3[0]
    for bad in ([100.0, 100.0] * 4, [100.0, 100, 200, 100, 300, 100, 200, 200]):
        pose, rms, status, _ = mp.fit(bad, k, None, mp.SIDE)
        assert status == 2 and rms == -1.0 and not pose.any()
