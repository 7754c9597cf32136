"""k_marker_pose on the GPU (rsba_marker_poses_from_corners): batches of the synthetic set against the numpy restatement
(tests/marker_pose_ref.py) and against the host entry at 1e-6 per pose, independence of a detection's result from its place in the batch,
bit for bit, the hongo time rows from the device's fits, and detections -> time rows -> camera rows -> bundle adjustment end to end.
The measured maxima are in profiles/marker_pose_accuracy.txt."""
import os
import sys

import numpy as np
import pytest

import marker_pose_ref as mp
import oracle_lib as ol
from realsensecalibration_amd import capi

sys.path.insert(0, os.path.join(ol.ROOT, "oracle"))
import initial_guess_oracle as ig  # noqa: E402

pytestmark = pytest.mark.gpu
HONGO = os.path.join(ol.GOLDEN, "hongo", "correspondence.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def _host(corners, cam, intr, dist):
    out, rms = np.zeros((len(corners), 6)), np.zeros(len(corners))
    for i in range(len(corners)):
        out[i], rms[i], status = capi.marker_pose_from_corners(corners[i], intr[cam[i]], None if dist is None else dist[cam[i]], mp.SIDE)
        assert status == 0
    return out, rms


@pytest.mark.parametrize("config", sorted(mp.DIST3))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches_against_the_reference_and_the_host_entry(config, n):
    corners, cam, intr, dist, _ = mp.batch(config, n)
    want, want_rms = mp.reference(config, n)
    host, host_rms = _host(corners, cam, intr, dist)
    poses, rms, status = capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
    assert poses.shape == (n, 6) and np.all(status == 0)
    to_ref = max(mp.pose_distance(poses[i], want[i]) for i in range(n))
    to_host = max(mp.pose_distance(poses[i], host[i]) for i in range(n))
    rms_ref, rms_host = np.abs(rms - want_rms).max(), np.abs(rms - host_rms).max()
    print("ACCURACY %s n=%d: pose vs reference %.3g, pose vs host %.3g, rms vs reference %.3g px, rms vs host %.3g px"
          % (config, n, to_ref, to_host, rms_ref, rms_host))
    assert to_ref < 1e-6 and to_host < 1e-6 and rms_ref < 1e-6 and rms_host < 1e-6


def test_a_result_does_not_depend_on_its_place():
    corners, cam, intr, dist, _ = mp.batch("mixed", 257)
    full = capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
    again = capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)                                   # two identical calls
    for src in (0, 5, 100):
        alone = capi.marker_poses_from_corners(corners[src:src + 1], cam[src:src + 1], intr, dist, mp.SIDE)
        for place in (0, 63, 256):
            c2, k2 = corners.copy(), cam.copy()
            c2[place], k2[place] = corners[src], cam[src]
            moved = capi.marker_poses_from_corners(c2, k2, intr, dist, mp.SIDE)
            for a, b in zip(alone, moved):
                assert np.array_equal(a[0], b[place]), (src, place)
            keep = np.arange(257) != place
            for a, b in zip(full, moved):
                assert np.array_equal(a[keep], b[keep])               # ... and the others do not notice


def test_a_degenerate_detection_leaves_its_neighbours_alone():
    corners, cam, intr, dist, _ = mp.batch("distorted", 65)
    clean = capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
    for bad in (np.tile(corners[17, :2], 4), np.array([100.0, 100, 200, 100, 300, 100, 200, 200]), np.concatenate([[5000.0, 5000.0], corners[17, 2:]])):
        c2 = corners.copy()
        c2[17] = bad
        poses, rms, status = capi.marker_poses_from_corners(c2, cam, intr, dist, mp.SIDE)
        assert status[17] == 2 and rms[17] == -1.0 and not poses[17].any()
        keep = np.arange(65) != 17
        assert np.array_equal(poses[keep], clean[0][keep]) and np.array_equal(rms[keep], clean[1][keep]) and np.all(status[keep] == 0)


def test_no_camera_index_is_camera_zero_and_an_empty_batch_is_ok():
    corners, _, intr, dist, _ = mp.batch("distorted", 65)
    a = capi.marker_poses_from_corners(corners, None, intr, dist, mp.SIDE)
    b = capi.marker_poses_from_corners(corners, np.zeros(65, np.int32), intr, dist, mp.SIDE)
    c = capi.marker_poses_from_corners(corners, None, intr[:1], dist[:1], mp.SIDE)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    poses, rms, status = capi.marker_poses_from_corners(np.zeros((0, 8)), None, intr, None, mp.SIDE)
    assert poses.shape == (0, 6) and rms.shape == (0,) and status.shape == (0,)
    # the optional outputs
    lib, out = capi.load(), np.zeros((65, 6))
    assert lib.rsba_marker_poses_from_corners(65, capi._vp(corners), None, 3, capi._vp(intr), capi._vp(dist), mp.SIDE, -1, capi._vp(out), None, None) == capi.OK
    assert np.array_equal(out, a[0])
    assert lib.rsba_marker_poses_from_corners(65, capi._vp(corners), None, 3, capi._vp(intr), capi._vp(dist), mp.SIDE, 1 << 20, capi._vp(out), None, None) == capi.ERR_ARG


def test_hongo_time_rows_from_the_device():
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    ref = ol.read_correspondence(HONGO)
    p = capi.Problem.correspondence(HONGO, capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    poses, rms, status = p.detection_poses()
    assert poses.shape == (68, 6) and np.all((status == 0) | (status == 1)), status
    print("HONGO rms of the 68 detections [px]: " + " ".join("%.4f" % v for v in rms))
    print("HONGO status: " + " ".join(str(v) for v in status))
    Cn, T = ref["C"], ref["T"]
    P = ref["params"].reshape(-1, 6)
    worst = 0.0
    for t in range(T):
        i = [k for k in range(ref["N"]) if ref["t"][k] == t and ref["c"][k] == 0][0]
        m = ref["m"][i]
        row = poses[i] if m == 0 else ig.base_pose_from_marker_detection(poses[i], P[Cn + T + m])
        worst = max(worst, np.abs(row - P[Cn + t]).max())
    print("HONGO largest deviation of the six time rows from the committed ones: %.3g" % worst)
    assert worst < 2e-5
    p.close()


def test_from_the_corners_to_the_calibration():
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    p = capi.Problem.correspondence(HONGO, capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    Cn, T = p.num_cameras, p.num_times
    p.params[:6 * (Cn + T)] = 0.0
    assert p.initial_time_poses() == 0
    p.initial_camera_poses()
    s = p.solve()
    print("END TO END final cost %.9f, %d iterations" % (s.final_cost, s.num_iterations))
    assert s.termination_type == capi.CONVERGENCE and abs(s.final_cost - 143.629388852) < 1.5e-3
    p.close()
