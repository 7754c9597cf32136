"""Both poses of a planar marker on the host (no GPU): tests/marker_pose_both_driver.cpp, a stand-alone program built with
-fsanitize=address,undefined as tests/test_marker_pose_host.py builds its driver, runs FitMarkerPoseBoth, MirrorMarkerPose and the block
resection with both solutions among its candidates; this file holds what it prints against the numpy restatement
(tests/marker_pose_both_ref.py), and the refusals of the new C entries that are decided before any device work.

The sets: the ambiguous one (small, nearly frontal markers: the restatement checks that it IS ambiguous), the first 60 detections of the
three configurations of tests/marker_pose_ref.py, a degenerate quadrilateral and a close-up whose second start slides back.  The crafted
block: tests/marker_pose_both_ref.crafted_rig.  Measured figures: profiles/marker_pose_both_accuracy.txt."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import marker_pose_both_ref as mb
import marker_pose_ref as mp
from realsensecalibration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "marker_pose_both_driver.cpp")] + [os.path.join(CSRC, f) for f in ("ba_problem.cpp", "rsba_capi.cpp", "ba_initial_guess.cpp", "ba_schur_plan.cpp")]
BAR = 1e-6
NAMES = ("rsba_marker_pose_from_corners_both", "rsba_marker_poses_from_corners_both", "rsba_problem_start_rig2", "rsba_problem_start_scene2")

DEGENERATE = np.array([100.0, 100, 200, 100, 300, 100, 200, 200])     # three corners on a line
# a 5 cm marker 12 cm from the camera, tilted 30 degrees: perspective leaves one minimum, the fit from the mirrored start ends at solution 0
CLOSE_UP_POSE = np.concatenate([mp.rvec_from_matrix(mp._rodrigues(np.array([np.radians(30.0), 0.0, 0.0])) @ np.diag([1.0, -1.0, -1.0])), [0.01, -0.005, 0.12]])


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("marker_pose_both") / "marker_pose_both_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + SOURCES + ["-o", exe])
    return exe


def run_driver(exe, args=()):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "marker pose both driver: ok" in r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()]


def cases():
    """[(name, corners 8, intrinsics 4, dist 5 or None)]: the ambiguous set, 60 of each configuration, the two crafted inputs."""
    out = []
    corners, _ = mb.ambiguous_set()
    out += [("ambiguous", c, mb.AMBIGUOUS_INTR, None) for c in corners]
    for config in sorted(mp.DIST3):
        corners, cam, intr, dist, _ = mp.batch(config, 60)
        out += [(config, corners[i], intr[cam[i]], None if dist is None else dist[cam[i]]) for i in range(60)]
    out.append(("degenerate", DEGENERATE, mb.AMBIGUOUS_INTR, None))
    out.append(("close-up", mp.project(CLOSE_UP_POSE, mp.SIDE, mb.AMBIGUOUS_INTR, None)[0].reshape(-1), mb.AMBIGUOUS_INTR, None))
    return out


@pytest.fixture(scope="module")
def fitted(driver, tmp_path_factory):
    path = tmp_path_factory.mktemp("both_cases") / "cases.txt"
    cs = cases()
    with open(path, "w") as f:
        for _, c8, k4, k5 in cs:
            row = list(k4) + [0 if k5 is None else 1] + list(np.zeros(5) if k5 is None else k5) + [mp.SIDE] + list(c8)
            f.write(" ".join(str(v) if isinstance(v, int) else repr(float(v)) for v in row) + "\n")
    lines = run_driver(driver, ["fit", str(path)])
    assert len(lines) == len(cs)
    return cs, lines


_REF = {}


def restated(k, case):
    if k not in _REF:
        _REF[k] = mb.fit_both(case[1], case[2], case[3], mp.SIDE)
    return _REF[k]


def test_the_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rsba.h")).read()
    lib = capi.load()
    for name in NAMES:
        assert name + "(" in hdr and name in capi.EXPORTS and hasattr(lib, name), name
    assert "RSBA_START_BOTH_SOLUTIONS 1" in hdr and "RSBA_MARKER_POSE_SAME 3" in hdr


def test_the_ambiguous_set_is_ambiguous():
    poses, rms, status, nearer = mb.ambiguous_reference()      # (asserts its own counts)
    lower = int(((status[:, 1] <= 1) & (rms[:, 1] < rms[:, 0])).sum())
    print("ambiguous set: %d of %d without a distinct second solution, solution 1 nearer the truth in %d, of lower RMS in %d" % (
        (status[:, 1] > 1).sum(), len(status), nearer.sum(), lower))


def test_the_builtin_checks_of_the_driver(driver):
    assert run_driver(driver) == []


def test_solution_0_is_the_single_fit_bit_for_bit(fitted):
    cs, lines = fitted
    for (name, c8, k4, k5), line in zip(cs, lines):
        if name == "degenerate":
            with pytest.raises(capi.RsbaError) as e:
                capi.marker_pose_from_corners(c8, k4, k5, mp.SIDE)
            assert e.value.code == capi.ERR_UNSUPPORTED and line["status"] == [2, 2]
            continue
        pose, rms, status = capi.marker_pose_from_corners(c8, k4, k5, mp.SIDE)
        assert np.array_equal(pose, np.array(line["poses"][:6])) and rms == line["rms"][0] and status == line["status"][0], name
        # the library's both-solutions entry: the sanitised build's bits (one source, two compilations: values, not a bar)
        both = capi.marker_pose_from_corners_both(c8, k4, k5, mp.SIDE)
        assert np.array_equal(both[0][0], pose) and both[1][0] == rms and list(both[2]) == line["status"], name
        assert np.abs(both[0].reshape(-1) - np.array(line["poses"])).max() < 1e-12


def test_solution_1_against_the_restatement(fitted):
    cs, lines = fitted
    worst, worst_rms, count, by_status = 0.0, 0.0, 0, {}
    for k, (case, line) in enumerate(zip(cs, lines)):
        want_poses, want_rms, want_status = restated(k, case)
        assert line["status"] == [int(s) for s in want_status], (case[0], k, line["status"], want_status)
        by_status[line["status"][1]] = by_status.get(line["status"][1], 0) + 1
        if line["status"][1] == 0 and want_status[1] == 0:
            worst = max(worst, mp.pose_distance(line["poses"][6:], want_poses[1]))
            worst_rms = max(worst_rms, abs(line["rms"][1] - want_rms[1]))
            count += 1
    print("ACCURACY solution 1, host vs restatement: largest pose difference %.3g, largest rms difference %.3g px over %d detections; statuses %s" % (
        worst, worst_rms, count, by_status))
    assert count >= 200 and worst < BAR and worst_rms < BAR


def test_statuses_2_and_3_arise(fitted):
    cs, lines = fitted
    by_name = {c[0]: ln for c, ln in zip(cs, lines)}
    assert by_name["degenerate"]["status"] == [2, 2] and not np.any(by_name["degenerate"]["poses"]) and by_name["degenerate"]["rms"] == [-1.0, -1.0]
    close = by_name["close-up"]
    assert close["status"] == [0, mb.STATUS_SAME] and not np.any(close["poses"][6:]) and close["rms"][1] == -1.0
    assert mp.pose_distance(close["poses"][:6], CLOSE_UP_POSE) < 1e-8 and close["rms"][0] < 1e-8
    # the restatement's fit from the mirrored start does end at solution 0 there: the status is the contract's, not an accident
    start, _ = mb.mirror(close["poses"][:6])
    assert mp.pose_distance(start, close["poses"][:6]) > 0.1
    assert mp.pose_distance(mp.fit(cs[-1][1], cs[-1][2], None, mp.SIDE, start=start)[0], close["poses"][:6]) < mb.SAME_BELOW


def test_the_mirror_is_a_proper_involution(fitted):
    cs, lines = fitted
    worst_twice = worst_det = worst_formula = 0.0
    for case, line in zip(cs, lines):
        if line["status"][0] > 1:
            continue
        worst_det = max(worst_det, abs(line["det"] - 1.0))
        worst_twice = max(worst_twice, max(v for v in line["twice"] if v >= 0.0))
        want, Rm = mb.mirror(line["poses"][:6])
        worst_formula = max(worst_formula, np.abs(mp._rodrigues(np.array(line["mirror0"][:3])) - Rm).max(), np.abs(np.array(line["mirror0"][3:]) - want[3:]).max())
        # the tilt changes sign: the marker's normal is reflected about the line of sight
        R0, v = mp._rodrigues(np.array(line["poses"][:3])), want[3:] / np.linalg.norm(want[3:])
        n0, n1 = R0[:, 2], Rm[:, 2]
        assert abs(n0 @ v - n1 @ v) < 1e-12 and np.abs((n0 - (n0 @ v) * v) + (n1 - (n1 @ v) * v)).max() < 1e-12
    print("mirror: |det - 1| %.3g, mirror of mirror %.3g, against numpy's formula %.3g" % (worst_det, worst_twice, worst_formula))
    assert worst_det < 1e-12 and worst_twice < 1e-12 and worst_formula < 1e-12


def test_each_converged_solution_is_a_stationary_point(fitted):
    """The loop stops when the damped step d = -(A + lambda diag A)^-1 g has max |d| < 1e-12 (1 + max |p|), A = J'J, g = J'r.  Then
    g = -(A + lambda diag A) d, and since |A_ij| <= sqrt(A_ii A_jj) <= max diag A, every row of A + lambda diag A sums to at most
    (6 + lambda) max diag A in absolute value:
        max |g| <= (6 + lambda) max diag(A) 1e-12 (1 + max |p|).
    lambda starts at 1e-3, falls by 10 on acceptance and rises by 10 on rejection; near a minimum the last steps are rejected by rounding
    (the cost cannot fall further) until the step is small, so lambda at the stop is whatever those rejections left.  The bound asserted is
        max |g| < 1e-6 max diag(A) (1 + max |p|),
    the stopping rule's 1e-12 with lambda up to 1e6 - 6 (fewer than nine rejections in a row from lambda = 1e-3).  g and A here come from the
    restatement's complex-step Jacobian at the product's pose."""
    cs, lines = fitted
    worst = 0.0
    checked = 0
    for (name, c8, k4, k5), line in zip(cs, lines):
        for s in range(2):
            if line["status"][s] != 0:
                continue
            p = np.array(line["poses"][6 * s:6 * s + 6])
            c = np.asarray(c8, float).reshape(4, 2)
            r, _ = mp._residuals(p, c, mp.SIDE, np.asarray(k4, float), k5)
            J = np.zeros((8, 6))
            for k in range(6):
                pc = p.astype(complex)
                pc[k] += 1e-30j
                J[:, k] = mp._residuals(pc, c, mp.SIDE, np.asarray(k4, float), k5)[0].imag / 1e-30
            g, A = J.T @ r, J.T @ J
            ratio = np.abs(g).max() / (np.diag(A).max() * (1.0 + np.abs(p).max()))
            worst = max(worst, ratio)
            checked += 1
            assert ratio < 1e-6, (name, s, ratio)
    print("stationarity: largest max|g| / (max diag(J'J) (1 + max|p|)) = %.3g over %d converged solutions (bar 1e-6)" % (worst, checked))
    assert checked >= 400


def test_the_crafted_block_needs_the_second_solutions(driver, tmp_path):
    """Time 0 of the crafted rig has two detections, from cameras 0 and 1, and the own fit of both is the mirror image.  Without the flag
    both candidates are mirrored and the block ends in the mirrored minimum; with it the block ends where the fit from the truth ends."""
    prob, known, pb = mb.crafted_rig()
    truth = np.asarray(prob["truth"], float).reshape(-1, 6)
    rows = [i for i in range(prob["N"]) if prob["t"][i] == mb.CRAFTED_TIME]
    assert len(rows) == 2 and sorted(int(prob["c"][i]) for i in rows) == [0, 1]
    path = tmp_path / "start.txt"
    mb.write_start_file(path, prob, 1, known, 1, [(pb, truth[pb])])
    (line,) = run_driver(driver, ["start", str(path)])
    nb = prob["C"] + prob["T"] + prob["M"]
    single, both = (np.array(line[k]["blocks"]).reshape(nb, 6) for k in ("single", "both"))
    from_truth = np.array(line["refits"])
    own, own2 = np.array(line["own_pose"]).reshape(-1, 6), np.array(line["own_pose2"]).reshape(-1, 6)
    # the precondition, by the host entry: solution 0 of BOTH detections is the mirror image, solution 1 the pose
    for i in rows:
        t = mb.own_truth(prob, i)
        far, near = mp.pose_distance(own[i], t), mp.pose_distance(own2[i], t)
        print("crafted detection %d (camera %d, marker %d): solution 0 is %.3f from the truth, solution 1 %.3f" % (i, prob["c"][i], prob["m"][i], far, near))
        assert line["own_status2"][i] == 0 and far > 0.1 and near < 0.5 * far
    cost_single, cost_both = line["single"]["start_cost"][pb], line["both"]["start_cost"][pb]
    d_single, d_both = mp.pose_distance(single[pb], from_truth), mp.pose_distance(both[pb], from_truth)
    print("ACCURACY crafted block: chosen start's cost %.6g without, %.6g with both solutions; end vs the minimiser from the truth: %.3g without (rms %.4f px), "
          "%.3g with (rms %.4f px; from the truth %.4f px)" % (cost_single, cost_both, d_single, line["single"]["rms"][pb], d_both, line["both"]["rms"][pb],
                                                             line["refit_rms"][0]))
    assert line["refit_status"] == [0] and line["both"]["status"][pb] == 0
    assert 0.0 <= cost_both <= cost_single
    assert d_both < BAR and abs(line["both"]["rms"][pb] - line["refit_rms"][0]) < BAR
    # the unflagged fit ends elsewhere: in the mirrored minimum, at four times the RMS
    assert d_single > 0.1 and line["single"]["rms"][pb] > 2.0 * line["both"]["rms"][pb]
    # every block's chosen start costs no more with the flag (the driver asserts it block by block while the runs hold the same blocks)
    for b in range(prob["C"], prob["C"] + prob["T"]):
        assert line["both"]["start_cost"][b] <= line["single"]["start_cost"][b], b
    # the other times have twelve detections: the flag changes nothing there beyond the minimiser's own repeatability
    others = [b for b in range(prob["C"], prob["C"] + prob["T"]) if b != pb]
    assert max(mp.pose_distance(single[b], both[b]) for b in others) < BAR


# ---------------------------------------------------------------------------------------------- refusals decided before any device work
def _batch_both(n, corners, cam, nc, intr, dist, side, poses=True):
    lib = capi.load()
    m = max(n, 1)
    out, rms, status = np.full((m, 12), 7.0), np.full((m, 2), 7.0), np.full((m, 2), 7, np.int32)
    v = lambda a: None if a is None else capi._vp(a)  # noqa: E731
    code = lib.rsba_marker_poses_from_corners_both(n, v(corners), v(cam), nc, v(intr), v(dist), C.c_double(side), -1, capi._vp(out) if poses else None,
                                                   capi._vp(rms), capi._vp(status))
    return code, bool(np.all(out == 7.0) and np.all(rms == 7.0) and np.all(status == 7))


def test_refusals_of_the_batch_are_decided_before_any_device_work():
    corners, cam, intr, dist, _ = mp.batch("mixed", 5)
    n = 5
    bad_cam_hi, bad_cam_lo = cam.copy(), cam.copy()
    bad_cam_hi[3], bad_cam_lo[0] = 3, -1
    nan_corners, inf_intr, nan_dist = corners.copy(), intr.copy(), dist.copy()
    nan_corners[4, 7], inf_intr[2, 0], nan_dist[1, 4] = float("nan"), float("inf"), float("nan")
    refused = [(-1, corners, cam, 3, intr, dist, mp.SIDE), (n, None, cam, 3, intr, dist, mp.SIDE), (n, corners, cam, 3, None, dist, mp.SIDE),
               (n, corners, cam, 0, intr, dist, mp.SIDE), (n, corners, bad_cam_hi, 3, intr, dist, mp.SIDE), (n, corners, bad_cam_lo, 3, intr, dist, mp.SIDE),
               (n, corners, cam, 2, intr, dist, mp.SIDE), (n, nan_corners, cam, 3, intr, dist, mp.SIDE), (n, corners, cam, 3, inf_intr, dist, mp.SIDE),
               (n, corners, cam, 3, intr, nan_dist, mp.SIDE), (n, corners, cam, 3, intr, dist, 0.0), (n, corners, cam, 3, intr, dist, -1.0),
               (n, corners, cam, 3, intr, dist, float("nan"))]
    for k, args in enumerate(refused):
        code, untouched = _batch_both(*args)
        assert code == capi.ERR_ARG and untouched, (k, code)
    assert _batch_both(n, corners, cam, 3, intr, dist, mp.SIDE, poses=False)[0] == capi.ERR_ARG
    if capi.load().rsba_device_count() == 0:      # the batch has no CPU path
        code, untouched = _batch_both(n, corners, cam, 3, intr, dist, mp.SIDE)
        assert code == capi.ERR_NO_DEVICE and untouched
        with pytest.raises(capi.RsbaError) as e:
            capi.marker_poses_from_corners_both(corners, cam, intr, dist, mp.SIDE)
        assert e.value.code == capi.ERR_NO_DEVICE


def test_refusals_of_the_single_entry():
    corners, cam, intr, dist, _ = mp.batch("distorted", 1)
    c, k, d = corners[0], intr[0].copy(), dist[0].copy()
    lib = capi.load()

    def call(c, k, d, side, poses=True):
        out = np.full(12, 7.0)
        v = lambda a: None if a is None else capi._vp(a)  # noqa: E731
        return lib.rsba_marker_pose_from_corners_both(v(c), v(k), v(d), C.c_double(side), capi._vp(out) if poses else None, None, None), out

    assert call(c, k, d, mp.SIDE)[0] == capi.OK and call(c, k, None, mp.SIDE)[0] == capi.OK
    for args in ((None, k, d, mp.SIDE), (c, None, d, mp.SIDE), (c, k, d, 0.0), (c, k, d, -0.05), (c, k, d, float("nan")), (c, k, d, float("inf"))):
        code, out = call(*args)
        assert code == capi.ERR_ARG and np.all(out == 7.0), args
    assert call(c, k, d, mp.SIDE, poses=False)[0] == capi.ERR_ARG
    for arr in (c, k, d):
        for bad in (float("nan"), float("inf")):
            keep = arr[1]
            arr[1] = bad
            code, out = call(c, k, d, mp.SIDE)
            assert code == capi.ERR_ARG and np.all(out == 7.0)
            arr[1] = keep
    with pytest.raises(capi.RsbaError) as e:
        capi.marker_pose_from_corners_both(DEGENERATE, k, None, mp.SIDE)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_refusals_of_the_flagged_starts():
    from realsensecalibration_amd import synthetic as syn
    lib = capi.load()
    prob, _, _ = mb.crafted_rig()
    p = capi.Problem.marker_chain(prob)
    before = p.params.copy()
    nb = p.num_cameras + p.num_times + p.num_markers
    status, rms, mt = np.full(nb, 7, np.int32), np.full(nb, 7.0), C.c_int32(7)
    # an unknown flag bit, before any device work: the same answer with and without a device
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
        assert lib.rsba_problem_start_rig2(p.h, None, 1, -1, flags, C.byref(mt), None, capi._vp(status), capi._vp(rms)) == capi.ERR_ARG, flags
        assert lib.rsba_problem_start_scene2(p.h, None, 1, -1, flags, C.byref(mt), None, None, capi._vp(status), capi._vp(rms)) == capi.ERR_ARG, flags
    for flags in (0, capi.START_BOTH_SOLUTIONS):
        for sweeps, device in ((-1, -1), (0, -2)):
            assert lib.rsba_problem_start_rig2(p.h, None, sweeps, device, flags, C.byref(mt), None, capi._vp(status), capi._vp(rms)) == capi.ERR_ARG
            assert lib.rsba_problem_start_scene2(p.h, None, sweeps, device, flags, C.byref(mt), None, None, capi._vp(status), capi._vp(rms)) == capi.ERR_ARG
        assert lib.rsba_problem_start_rig2(None, None, 0, -1, flags, None, None, None, None) == capi.ERR_ARG
        assert lib.rsba_problem_start_scene2(None, None, 0, -1, flags, None, None, None, None, None) == capi.ERR_ARG
    assert np.array_equal(p.params, before) and np.all(status == 7) and np.all(rms == 7.0) and mt.value == 7
    p.close()
    # the point model
    pts = capi.Problem.points(syn.make_problem(2, 20, 2, seed=1))
    for flags in (0, capi.START_BOTH_SOLUTIONS):
        assert lib.rsba_problem_start_rig2(pts.h, None, 1, -1, flags, None, None, None, None) == capi.ERR_UNSUPPORTED
        assert lib.rsba_problem_start_scene2(pts.h, None, 1, -1, flags, None, None, None, None, None) == capi.ERR_UNSUPPORTED
    assert lib.rsba_problem_start_rig2(pts.h, None, 1, -1, 2, None, None, None, None) == capi.ERR_ARG      # the flag check comes first
    for both in (False, True):
        with pytest.raises(capi.RsbaError) as e:
            pts.start_rig(both_solutions=both)
        assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.RsbaError) as e:
            pts.start_scene(both_solutions=both)
        assert e.value.code == capi.ERR_UNSUPPORTED
    pts.close()
