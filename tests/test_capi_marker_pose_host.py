"""Host entries of the single-marker pose fit through librsba.so (no GPU): rsba_marker_pose_from_corners against the numpy restatement
(tests/marker_pose_ref.py) on the synthetic set, rsba_problem_initial_time_poses against the time rows the reference committed for
hongo, and every refusal of the three new entries that is decided before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import marker_pose_ref as mp
import oracle_lib as ol
from realsensecalibration_amd import capi
from test_marker_pose_ref_cpu import hongo_time_rows

NAMES = ("rsba_marker_pose_from_corners", "rsba_marker_poses_from_corners", "rsba_problem_initial_time_poses")
HONGO = os.path.join(ol.GOLDEN, "hongo", "correspondence.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


def _hongo_problem():
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    return capi.Problem.correspondence(HONGO, capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr), intr


def test_the_entries_are_declared_and_exported():
    hdr = open(os.path.join(ol.ROOT, "include", "rsba.h")).read()
    lib = capi.load()
    for name in NAMES:
        assert name + "(" in hdr and name in capi.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("config", sorted(mp.DIST3))
def test_host_fit_against_the_reference(config):
    """1e-6 per pose (BASELINE's parameter bar) on noisy corners, every case checked to be unambiguous by the reference itself."""
    n = 60
    corners, cam, intr, dist, _ = mp.batch(config, n)
    want, want_rms = mp.reference(config, n)
    worst = worst_rms = 0.0
    for i in range(n):
        pose, rms, status = capi.marker_pose_from_corners(corners[i], intr[cam[i]], None if dist is None else dist[cam[i]], mp.SIDE)
        assert status == 0, (i, status)
        worst, worst_rms = max(worst, mp.pose_distance(pose, want[i])), max(worst_rms, abs(rms - want_rms[i]))
    print("%s: largest pose difference %.3g, largest rms difference %.3g px" % (config, worst, worst_rms))
    assert worst < 1e-6 and worst_rms < 1e-6, (worst, worst_rms)


@pytest.mark.parametrize("config", sorted(mp.DIST3))
def test_host_fit_recovers_exact_poses(config):
    """Noise-free corners: the pose that made them, at the 1e-8 tests/test_initial_guess.py uses for exact data."""
    corners, cam, intr, dist, truth = mp.batch(config, 30, noise=0.0)
    for i in range(30):
        pose, rms, status = capi.marker_pose_from_corners(corners[i], intr[cam[i]], None if dist is None else dist[cam[i]], mp.SIDE)
        assert status == 0 and rms < 1e-8 and mp.pose_distance(pose, truth[i]) < 1e-8, (i, status, rms)


def test_zero_coefficients_are_the_pinhole_fit():
    corners, cam, intr, _, _ = mp.batch("pinhole", 5)
    for i in range(5):
        a = capi.marker_pose_from_corners(corners[i], intr[cam[i]], None, mp.SIDE)
        b = capi.marker_pose_from_corners(corners[i], intr[cam[i]], np.zeros(5), mp.SIDE)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_initial_time_poses_reproduces_the_committed_time_rows():
    """THE pin: from the corners alone, the six time rows the reference's OpenCV wrote into hongo's correspondence.txt, to their
    printed digits (2e-5).  Then the camera rows EPnP gives from those time rows: recorded, no bar (EPnP's sensitivity to a 5e-6 change
    of its object points is unmeasured)."""
    p, intr = _hongo_problem()
    committed = p.params.copy()
    Cn, T = p.num_cameras, p.num_times
    p.params[6 * Cn:6 * (Cn + T)] = 0.0
    assert p.initial_time_poses() == 0
    ours = p.params.copy()
    assert np.array_equal(ours[:6 * Cn], committed[:6 * Cn]) and np.array_equal(ours[6 * (Cn + T):], committed[6 * (Cn + T):])
    dev = np.abs(ours[6 * Cn:6 * (Cn + T)] - committed[6 * Cn:6 * (Cn + T)]).max()
    print("largest deviation from the committed time rows: %.3g" % dev)
    assert dev < 2e-5, dev
    # the same rows from the single entry and the pose algebra, and from the reference
    rows, _, _ = hongo_time_rows(lambda i, corners, k: capi.marker_pose_from_corners(corners, k, None, ol.MARKER_SIDE_MAIN)[0])
    assert np.abs(rows.reshape(-1) - ours[6 * Cn:6 * (Cn + T)]).max() < 1e-12
    rows_ref, _, _ = hongo_time_rows(lambda i, corners, k: mp.fit(corners, k, None, ol.MARKER_SIDE_MAIN)[0])
    assert np.abs(rows_ref.reshape(-1) - ours[6 * Cn:6 * (Cn + T)]).max() < 1e-6
    p.params[:6 * Cn] = 0.0
    p.initial_camera_poses()
    cam_dev = np.abs(p.params[:6 * Cn] - committed[:6 * Cn]).reshape(Cn, 6).max(1)
    print("camera rows from these time rows, deviation from the committed ones per camera:", cam_dev)
    assert np.all(np.isfinite(p.params))
    p.close()


def test_a_time_camera_0_did_not_see_keeps_its_bits():
    ref = ol.read_correspondence(HONGO)
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    c = ref["c"].copy()
    c[(ref["t"] == 2) & (ref["c"] == 0)] = 1
    params = ref["params"].copy()
    Cn, T = ref["C"], ref["T"]
    params[6 * Cn:6 * (Cn + T)] = np.arange(6 * T) + 0.25
    p = capi.Problem.marker_chain(dict(ref, c=c, params=params, intr=intr, marker_side=ol.MARKER_SIDE_MAIN))
    assert p.initial_time_poses() == 1
    got = p.params[6 * Cn:6 * (Cn + T)].reshape(T, 6)
    assert np.array_equal(got[2], np.arange(12, 18) + 0.25)
    want = ref["params"][6 * Cn:6 * (Cn + T)].reshape(T, 6)
    for t in (0, 1, 3, 4, 5):
        assert np.abs(got[t] - want[t]).max() < 2e-5
    # a degenerate detection at a time counts as missing too: time 0's first detection collapsed to a point
    obs = ref["obs"].reshape(-1, 8).copy()
    first = [i for i in range(ref["N"]) if ref["t"][i] == 0 and ref["c"][i] == 0][0]
    obs[first] = np.tile(obs[first, :2], 4)
    q = capi.Problem.marker_chain(dict(ref, obs=obs.reshape(-1), params=params, intr=intr, marker_side=ol.MARKER_SIDE_MAIN))
    assert q.initial_time_poses() == 1 and np.array_equal(q.params[6 * Cn:6 * Cn + 6], np.arange(6) + 0.25)
    # the count is optional
    assert capi.load().rsba_problem_initial_time_poses(q.h, None) == capi.OK
    p.close()
    q.close()


def test_initial_time_poses_honours_the_problems_distortion():
    """Corners made with camera 0's coefficients give the true base pose back only when the problem carries them."""
    b = mp.batch("distorted", 12, noise=0.0)
    corners, truth = b[0][0::3], b[4][0::3]      # camera 0's detections
    T = len(corners)
    intr, dist = mp.INTRINSICS3[:1], mp.DIST3["distorted"][:1]
    prob = dict(T=T, C=1, M=1, N=T, t=np.arange(T, dtype=np.int32), c=np.zeros(T, np.int32), m=np.zeros(T, np.int32), obs=corners.reshape(-1),
                params=np.zeros(6 * (1 + T + 1)), intr=intr, marker_side=mp.SIDE)
    with_dist, without = capi.Problem.marker_chain(dict(prob, dist=dist)), capi.Problem.marker_chain(prob)
    assert with_dist.initial_time_poses() == 0 and without.initial_time_poses() == 0
    for t in range(T):
        assert mp.pose_distance(with_dist.params[6 + 6 * t:12 + 6 * t], truth[t]) < 1e-8
    assert max(mp.pose_distance(without.params[6 + 6 * t:12 + 6 * t], truth[t]) for t in range(T)) > 1e-4
    with_dist.close()
    without.close()


def test_the_point_model_is_refused():
    from realsensecalibration_amd import synthetic
    p = capi.Problem.points(synthetic.make_problem(2, 20, 2, seed=1))
    with pytest.raises(capi.RsbaError) as e:
        p.initial_time_poses()
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert capi.load().rsba_problem_initial_time_poses(None, None) == capi.ERR_ARG
    p.close()


def _single(corners, k, dist, side, pose=True):
    out = np.full(6, 7.0)
    code = capi.load().rsba_marker_pose_from_corners(None if corners is None else capi._vp(corners), None if k is None else capi._vp(k),
                                                     None if dist is None else capi._vp(dist), C.c_double(side), capi._vp(out) if pose else None,
                                                     None, None)
    return code, out


def test_refusals_of_the_single_fit():
    corners, cam, intr, dist, _ = mp.batch("distorted", 1)
    c, k, d = corners[0], intr[0].copy(), dist[0].copy()
    assert _single(c, k, d, mp.SIDE)[0] == capi.OK and _single(c, k, None, mp.SIDE)[0] == capi.OK      # rms and status are optional
    for args in ((None, k, d, mp.SIDE), (c, None, d, mp.SIDE), (c, k, d, 0.0), (c, k, d, -0.05), (c, k, d, float("nan")), (c, k, d, float("inf"))):
        code, out = _single(*args)
        assert code == capi.ERR_ARG and np.all(out == 7.0), args
    assert _single(c, k, d, mp.SIDE, pose=False)[0] == capi.ERR_ARG
    for arr in (c, k, d):
        for bad in (float("nan"), float("inf")):
            keep = arr[1]
            arr[1] = bad
            code, out = _single(c, k, d, mp.SIDE)
            assert code == capi.ERR_ARG and np.all(out == 7.0)
            arr[1] = keep
    # degenerate detections: RSBA_ERR_UNSUPPORTED as coplanar EPnP, pose zeros, rms -1, status 2
    far = c.copy()
    far[:2] = 5000.0      # no fixed point of the undistortion at that radius
    for bad, dd in (([100.0, 100.0] * 4, None), ([100.0, 100, 200, 100, 300, 100, 200, 200], None), ([100.0, 100, 200, 100, 200, 200, 300, 300], None), (far, d)):
        pose, rms, status = np.full(6, 7.0), C.c_double(7.0), C.c_int32(7)
        bad = np.array(bad, float)
        code = capi.load().rsba_marker_pose_from_corners(capi._vp(bad), capi._vp(k), None if dd is None else capi._vp(dd), C.c_double(mp.SIDE),
                                                         capi._vp(pose), C.byref(rms), C.byref(status))
        assert code == capi.ERR_UNSUPPORTED and not pose.any() and rms.value == -1.0 and status.value == 2, bad
        with pytest.raises(capi.RsbaError) as e:
            capi.marker_pose_from_corners(bad, k, dd, mp.SIDE)
        assert e.value.code == capi.ERR_UNSUPPORTED


def _batch_call(n, corners, cam, nc, intr, dist, side, poses=True):
    lib = capi.load()
    out, rms, status = np.full((max(n, 1), 6), 7.0), np.full(max(n, 1), 7.0), np.full(max(n, 1), 7, np.int32)
    v = lambda a: None if a is None else capi._vp(a)  # noqa: E731
    code = lib.rsba_marker_poses_from_corners(n, v(corners), v(cam), nc, v(intr), v(dist), C.c_double(side), -1, capi._vp(out) if poses else None,
                                              capi._vp(rms), capi._vp(status))
    return code, bool(np.all(out == 7.0) and np.all(rms == 7.0) and np.all(status == 7))


def test_refusals_of_the_batch_are_decided_before_any_device_work():
    corners, cam, intr, dist, _ = mp.batch("mixed", 5)
    n = 5
    bad_cam_hi, bad_cam_lo = cam.copy(), cam.copy()
    bad_cam_hi[3], bad_cam_lo[0] = 3, -1
    nan_corners, inf_intr, nan_dist = corners.copy(), intr.copy(), dist.copy()
    nan_corners[4, 7], inf_intr[2, 0], nan_dist[1, 4] = float("nan"), float("inf"), float("nan")
    cases = [(-1, corners, cam, 3, intr, dist, mp.SIDE), (n, None, cam, 3, intr, dist, mp.SIDE), (n, corners, cam, 3, None, dist, mp.SIDE),
             (n, corners, cam, 0, intr, dist, mp.SIDE), (n, corners, bad_cam_hi, 3, intr, dist, mp.SIDE), (n, corners, bad_cam_lo, 3, intr, dist, mp.SIDE),
             (n, corners, cam, 2, intr, dist, mp.SIDE), (n, nan_corners, cam, 3, intr, dist, mp.SIDE), (n, corners, cam, 3, inf_intr, dist, mp.SIDE),
             (n, corners, cam, 3, intr, nan_dist, mp.SIDE), (n, corners, cam, 3, intr, dist, 0.0), (n, corners, cam, 3, intr, dist, -1.0),
             (n, corners, cam, 3, intr, dist, float("nan"))]
    for k, args in enumerate(cases):
        code, untouched = _batch_call(*args)
        assert code == capi.ERR_ARG and untouched, (k, code)
    assert _batch_call(n, corners, cam, 3, intr, dist, mp.SIDE, poses=False)[0] == capi.ERR_ARG


def test_the_batch_has_no_cpu_path():
    corners, cam, intr, dist, _ = mp.batch("mixed", 5)
    if capi.load().rsba_device_count() == 0:
        code, untouched = _batch_call(5, corners, cam, 3, intr, dist, mp.SIDE)
        assert code == capi.ERR_NO_DEVICE and untouched
        with pytest.raises(capi.RsbaError) as e:
            capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
        assert e.value.code == capi.ERR_NO_DEVICE
    else:
        assert _batch_call(5, corners, cam, 3, intr, dist, mp.SIDE)[0] == capi.OK
