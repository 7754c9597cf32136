"""Both poses of a planar marker on the GPU: rsba_marker_poses_from_corners_both (k_marker_pose, then k_marker_pose_mirror) against the
single-solution batch (bit for bit) and the host entry (1e-6, the project's pose bar); rsba_problem_start_rig2 / _scene2 with flags 0
against the entries without flags (bit for bit), and with RSBA_START_BOTH_SOLUTIONS against the serial host path of
tests/marker_pose_both_driver.cpp and the minimiser reached from the truth.  tests/test_marker_pose_both_host.py runs the same sets and the
same crafted block on the CPU first.  Measured figures: profiles/marker_pose_both_accuracy.txt."""
import json
import os
import subprocess

import numpy as np
import pytest

import marker_pose_both_ref as mb
import marker_pose_ref as mp
import oracle_lib as ol
import rig_start_ref as rs
import scene_start_ref as ss
from realsensecalibration_amd import capi, synthetic as syn

pytestmark = pytest.mark.gpu
BAR = 1e-6
CONFIGS = sorted(mp.DIST3) + ["ambiguous"]
_BATCH = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/marker_pose_both_driver.cpp without the C entries (three headers, one source) under AddressSanitizer and UBSan."""
    exe = str(tmp_path_factory.mktemp("marker_pose_both_gpu") / "marker_pose_both_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-DRSBA_DRIVER_HEADERS_ONLY", "-I", rs.CSRC,
                           os.path.join(rs.ROOT, "tests", "marker_pose_both_driver.cpp"), "-o", exe])
    return exe


def host_start(exe, path, prob, model, known, sweeps, refits=()):
    mb.write_start_file(path, prob, model, known, sweeps, refits)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "start", str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "marker pose both driver: ok" in r.stderr, r.stdout[-1000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    return json.loads(r.stdout)


def batch(config):
    """(corners, camera index or None, intrinsics, dist or None): 257 detections of a configuration (255, 256 and 257 are the lane edges of
    a 256-lane workgroup), or the 60 ambiguous ones."""
    if config == "ambiguous":
        return mb.ambiguous_set()[0], None, mb.AMBIGUOUS_INTR.reshape(1, 4).copy(), None
    corners, cam, intr, dist, _ = mp.batch(config, 257)
    return corners, cam, intr, dist


def device_both(config):
    if config not in _BATCH:
        corners, cam, intr, dist = batch(config)
        _BATCH[config] = capi.marker_poses_from_corners_both(corners, cam, intr, dist, mp.SIDE)
    return _BATCH[config]


@pytest.mark.parametrize("config", CONFIGS)
def test_solution_0_is_the_single_batch_bit_for_bit(config):
    corners, cam, intr, dist = batch(config)
    poses, rms, status = device_both(config)
    p0, e0, s0 = capi.marker_poses_from_corners(corners, cam, intr, dist, mp.SIDE)
    assert np.array_equal(poses[:, 0], p0) and np.array_equal(rms[:, 0], e0) and np.array_equal(status[:, 0], s0)
    assert np.all(s0 <= 1)


@pytest.mark.parametrize("config", CONFIGS)
def test_solution_1_against_the_host_entry(config):
    corners, cam, intr, dist = batch(config)
    poses, rms, status = device_both(config)
    worst = worst_rms = 0.0
    count = 0
    for i in range(len(corners)):
        c = 0 if cam is None else cam[i]
        hp, he, hs = capi.marker_pose_from_corners_both(corners[i], intr[c], None if dist is None else dist[c], mp.SIDE)
        assert list(hs) == list(status[i]), (i, hs, status[i])
        assert np.array_equal(hp[0], poses[i, 0]) or mp.pose_distance(hp[0], poses[i, 0]) < BAR
        if hs[1] <= 1:
            worst, worst_rms = max(worst, mp.pose_distance(hp[1], poses[i, 1])), max(worst_rms, abs(he[1] - rms[i, 1]))
            count += 1
        else:
            assert not poses[i, 1].any() and rms[i, 1] == -1.0
    print("ACCURACY solution 1 %s: device vs host, largest pose difference %.3g, largest rms difference %.3g px over %d of %d detections; statuses %s" % (
        config, worst, worst_rms, count, len(corners), np.bincount(status[:, 1], minlength=4).tolist()))
    assert count >= 0.9 * len(corners) and worst < BAR and worst_rms < BAR
    if config == "ambiguous":
        # the set's point: in at least 10 of 60 the device's solution 1, not its solution 0, is the one nearer the truth
        truth = mb.ambiguous_set()[1]
        nearer = sum(1 for i in range(len(corners)) if status[i, 1] <= 1 and mp.pose_distance(poses[i, 1], truth[i]) < mp.pose_distance(poses[i, 0], truth[i]))
        print("ACCURACY ambiguous set on the device: solution 1 is the nearer to the truth in %d of %d" % (nearer, len(corners)))
        assert nearer >= 10


@pytest.mark.parametrize("config", ["mixed", "ambiguous"])
def test_place_and_repetition_of_the_batch(config):
    corners, cam, intr, dist = batch(config)
    a = device_both(config)
    b = capi.marker_poses_from_corners_both(corners, cam, intr, dist, mp.SIDE)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    perm = np.random.default_rng(5).permutation(len(corners))
    c = capi.marker_poses_from_corners_both(corners[perm], None if cam is None else cam[perm], intr, dist, mp.SIDE)
    assert all(np.array_equal(x[perm], y) for x, y in zip(a, c))
    # the lane edges: the first 255 and 256 detections alone
    for n in (255, 256):
        if n < len(corners):
            d = capi.marker_poses_from_corners_both(corners[:n], None if cam is None else cam[:n], intr, dist, mp.SIDE)
            assert all(np.array_equal(x[:n], y) for x, y in zip(a, d))


def test_an_empty_batch_and_a_degenerate_detection():
    corners, cam, intr, dist = batch("distorted")
    lib = capi.load()
    poses, rms, status = np.full((1, 12), 7.0), np.full(2, 7.0), np.full(2, 7, np.int32)
    assert lib.rsba_marker_poses_from_corners_both(0, None, None, 3, capi._vp(intr), capi._vp(dist), capi.C.c_double(mp.SIDE), -1, None, None, None) == capi.OK
    assert lib.rsba_marker_poses_from_corners_both(0, capi._vp(corners), capi._vp(cam), 3, capi._vp(intr), capi._vp(dist), capi.C.c_double(mp.SIDE), -1,
                                                   capi._vp(poses), capi._vp(rms), capi._vp(status)) == capi.OK
    assert np.all(poses == 7.0) and np.all(rms == 7.0) and np.all(status == 7)
    n = 9
    bad = corners[:n].copy()
    bad[4] = np.tile(bad[4, :2], 4)      # collapsed to a point
    clean = capi.marker_poses_from_corners_both(corners[:n], cam[:n], intr, dist, mp.SIDE)
    got = capi.marker_poses_from_corners_both(bad, cam[:n], intr, dist, mp.SIDE)
    assert list(got[2][4]) == [2, 2] and not got[0][4].any() and list(got[1][4]) == [-1.0, -1.0]
    keep = np.arange(n) != 4
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(clean, got))
    # rms and status are optional
    only = np.zeros((n, 12))
    assert lib.rsba_marker_poses_from_corners_both(n, capi._vp(corners[:n].copy()), capi._vp(cam[:n].copy()), 3, capi._vp(intr), capi._vp(dist),
                                                   capi.C.c_double(mp.SIDE), -1, capi._vp(only), None, None) == capi.OK
    assert np.array_equal(only.reshape(n, 2, 6), clean[0])


# ------------------------------------------------------------------------------------------------------------ the starts with flags
def rig2(prob, flags, known=None, sweeps=1, zero=(), model=1):
    """rsba_problem_start_rig2 -> (blocks, (missing times, cameras), status, rms)"""
    p = capi.Problem.marker_chain(prob, model)
    for b in zero:
        p.params[6 * b:6 * b + 6] = 0.0
    nb = p.num_cameras + p.num_times
    k = None if known is None else np.ascontiguousarray(known, np.uint8)
    mt, mc = capi.C.c_int32(0), capi.C.c_int32(0)
    status, rms = np.zeros(nb, np.int32), np.zeros(nb)
    code = capi.load().rsba_problem_start_rig2(p.h, None if k is None else capi._vp(k), sweeps, -1, flags, capi.C.byref(mt), capi.C.byref(mc), capi._vp(status),
                                               capi._vp(rms))
    assert code == capi.OK, code
    out = p.params.copy().reshape(-1, 6)
    p.close()
    return out, (mt.value, mc.value), status, rms


def scene2(prob, flags, known=None, sweeps=1, zero=(), model=1):
    p = capi.Problem.marker_chain(prob, model)
    for b in zero:
        p.params[6 * b:6 * b + 6] = 0.0
    nb = p.num_cameras + p.num_times + p.num_markers
    k = None if known is None else np.ascontiguousarray(known, np.uint8)
    mt, mc, mm = capi.C.c_int32(0), capi.C.c_int32(0), capi.C.c_int32(0)
    status, rms = np.zeros(nb, np.int32), np.zeros(nb)
    code = capi.load().rsba_problem_start_scene2(p.h, None if k is None else capi._vp(k), sweeps, -1, flags, capi.C.byref(mt), capi.C.byref(mc), capi.C.byref(mm),
                                                 capi._vp(status), capi._vp(rms))
    assert code == capi.OK, code
    out = p.params.copy().reshape(-1, 6)
    p.close()
    return out, (mt.value, mc.value, mm.value), status, rms


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_flags_0_is_start_rig_and_start_scene_bit_for_bit_on_the_small_rig():
    prob = rs.small_problem()
    C, T, M = prob["C"], prob["T"], prob["M"]
    p = capi.Problem.marker_chain(prob)
    p.params[:6 * (C + T)] = 0.0
    mt, mc, status, rms = p.start_rig(None, 1)
    old = (p.params.copy().reshape(-1, 6), (mt, mc), status, rms)
    p.close()
    assert set(status[1:]) <= {0, 1}
    assert same_bits(rig2(prob, 0, None, 1, zero=range(C + T)), old)
    q = capi.Problem.marker_chain(ss.unknown_board(prob))
    mt, mc, mm, status, rms = q.start_scene(None, 1)
    old = (q.params.copy().reshape(-1, 6), (mt, mc, mm), status, rms)
    q.close()
    assert set(np.delete(status, [0, C + T])) <= {0, 1}
    assert same_bits(scene2(ss.unknown_board(prob), 0, None, 1), old)


def hongo(known_markers=4):
    p = capi.Problem.correspondence(os.path.join(ol.GOLDEN, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN,
                                    ol.read_intrinsics(ol.SERIALS_MAIN))
    Cn, T, M = p.num_cameras, p.num_times, p.num_markers
    p.params[:6 * (Cn + T)] = 0.0
    p.params[6 * (Cn + T + known_markers):] = 0.0
    return p, np.array([0] * (Cn + T) + [1] * known_markers + [0] * (M - known_markers), np.uint8)


def test_flags_0_is_start_scene_bit_for_bit_on_hongo():
    """Markers 0-3 keep the committed geometry and are flagged (test_gpu_scene_start's case); start_rig with the whole board given."""
    lib = capi.load()
    p, known = hongo()
    mt, mc, mm, status, rms = p.start_scene(known)
    old = p.params.copy()
    p.close()
    q, _ = hongo()
    nb = len(known)
    status2, rms2 = np.zeros(nb, np.int32), np.zeros(nb)
    m2 = [capi.C.c_int32(7) for _ in range(3)]
    assert lib.rsba_problem_start_scene2(q.h, capi._vp(known), 1, -1, 0, capi.C.byref(m2[0]), capi.C.byref(m2[1]), capi.C.byref(m2[2]), capi._vp(status2),
                                         capi._vp(rms2)) == capi.OK
    assert np.array_equal(q.params, old) and np.array_equal(status, status2) and np.array_equal(rms, rms2) and [v.value for v in m2] == [mt, mc, mm]
    assert set(status[1:len(known) - 11]) <= {0, 1}
    q.close()
    a, _ = hongo(11)
    mt, mc, status, rms = a.start_rig()
    b, _ = hongo(11)
    nb = a.num_cameras + a.num_times
    status2, rms2 = np.zeros(nb, np.int32), np.zeros(nb)
    assert lib.rsba_problem_start_rig2(b.h, None, 1, -1, 0, capi.C.byref(m2[0]), capi.C.byref(m2[1]), capi._vp(status2), capi._vp(rms2)) == capi.OK
    assert np.array_equal(a.params, b.params) and np.array_equal(status, status2) and np.array_equal(rms, rms2) and [m2[0].value, m2[1].value] == [mt, mc]
    a.close()
    b.close()


def test_the_crafted_block_on_the_device(driver, tmp_path):
    """The two-detection time of marker_pose_both_ref.crafted_rig inside its 3 x 4 x 4 rig (38 detections): with the flag the block is the
    serial host path's and the minimiser reached from the truth; without it the block ends in the mirrored minimum."""
    prob, known, pb = mb.crafted_rig()
    C, T, M = prob["C"], prob["T"], prob["M"]
    assert prob["N"] == 38
    truth = np.asarray(prob["truth"], float).reshape(-1, 6)
    host = host_start(driver, tmp_path / "crafted.txt", prob, 1, known, 1, [(pb, truth[pb])])
    host_both = np.array(host["both"]["blocks"]).reshape(-1, 6)
    from_truth = np.array(host["refits"])
    times = list(range(C, C + T))
    for name, got in (("start_rig2", rig2(prob, capi.START_BOTH_SOLUTIONS, known[:C + T], 1)), ("start_scene2", scene2(prob, capi.START_BOTH_SOLUTIONS, known, 1))):
        blocks, missing, status, rms = got
        to_host = max(mp.pose_distance(blocks[b], host_both[b]) for b in times)
        d = mp.pose_distance(blocks[pb], from_truth)
        print("ACCURACY crafted block, %s with both solutions: device vs serial host %.3g (all times), vs the minimiser from the truth %.3g, rms %.4f px" % (
            name, to_host, d, rms[pb]))
        assert set(missing) == {0} and list(status[C:C + T]) == host["both"]["status"][C:C + T] and status[pb] == 0
        assert to_host < BAR and np.abs(rms[C:C + T] - np.array(host["both"]["rms"])[C:C + T]).max() < BAR
        assert d < BAR
        assert np.array_equal(blocks[:C], truth[:C]) and np.array_equal(blocks[C + T:], truth[C + T:])     # the given blocks keep their bits
    # through the Python flag
    p = capi.Problem.marker_chain(prob)
    p.start_rig(known[:C + T], 1, both_solutions=True)
    assert mp.pose_distance(p.params[6 * pb:6 * pb + 6], from_truth) < BAR
    p.close()
    # without the flag: the mirrored minimum, as on the host
    blocks, _, status, rms = rig2(prob, 0, known[:C + T], 1)
    host_single = np.array(host["single"]["blocks"]).reshape(-1, 6)
    d = mp.pose_distance(blocks[pb], from_truth)
    print("ACCURACY crafted block without the flag: %.3g from the minimiser from the truth, rms %.4f px" % (d, rms[pb]))
    assert d > 0.1 and mp.pose_distance(blocks[pb], host_single[pb]) < BAR


def noise_free_rig():
    prob = syn.make_marker_chain(3, 4, 4, seed=60, keep=1.0, noise_px=0.0)
    C, T = prob["C"], prob["T"]
    blocks = np.asarray(prob["truth"], float).reshape(-1, 6).copy()
    blocks[:C + T] = 0.0                 # the board is the truth: the true candidate costs zero with and without the flag
    return dict(prob, params=blocks.ravel())


def test_the_flag_changes_nothing_where_the_true_candidate_costs_zero():
    prob = noise_free_rig()
    C, T = prob["C"], prob["T"]
    truth = np.asarray(prob["truth"], float).reshape(-1, 6)
    for name, run, known in (("start_rig2", rig2, None), ("start_scene2", scene2, [0] * (C + T) + [1] * prob["M"])):
        without, with_flag = run(prob, 0, known, 1), run(prob, capi.START_BOTH_SOLUTIONS, known, 1)
        gap = max(mp.pose_distance(a, b) for a, b in zip(without[0], with_flag[0]))
        to_truth = max(mp.pose_distance(a, b) for a, b in zip(with_flag[0], truth))
        print("ACCURACY noise-free 3 x 4 x 4, %s: flagged vs unflagged %.3g, flagged vs the truth %.3g" % (name, gap, to_truth))
        assert np.array_equal(without[2], with_flag[2]) and set(with_flag[2][1:C + T]) <= {0, 1}
        assert gap < BAR and to_truth < BAR
    # the board unknown too: the first round's candidates still include the truth at cost zero
    a, b = scene2(ss.unknown_board(prob), 0, None, 1), scene2(ss.unknown_board(prob), capi.START_BOTH_SOLUTIONS, None, 1)
    gap = max(mp.pose_distance(x, y) for x, y in zip(a[0], b[0]))
    print("ACCURACY noise-free 3 x 4 x 4, board unknown: flagged vs unflagged %.3g" % gap)
    assert np.array_equal(a[2], b[2]) and gap < BAR


def test_place_and_repetition_with_the_flag():
    """test_gpu_rig_start's: one time's detections alone (T = 1) and as time 37 of 65 give the same bits for that block; two calls give
    the same bits everywhere."""
    full = syn.make_marker_chain(3, 65, 4, seed=63)
    C, T = full["C"], full["T"]
    known = [1] * C + [0] * T
    flag = capi.START_BOTH_SOLUTIONS
    a = rig2(full, flag, known, 1, zero=range(C, C + T))
    b = rig2(full, flag, known, 1, zero=range(C, C + T))
    assert same_bits(a, b)
    rows = np.asarray(full["t"]) == 37
    assert rows.sum() >= 2
    alone = rs.keep_rows(full, rows)
    alone["t"] = np.zeros(alone["N"], np.int32)
    alone["T"] = 1
    blocks = np.asarray(full["params"], float).reshape(-1, 6)
    alone["params"] = np.concatenate([blocks[:C], np.zeros((1, 6)), blocks[C + T:]]).ravel()
    c = rig2(alone, flag, [1] * C + [0], 1)
    assert c[2][C] in (0, 1) and c[2][C] == a[2][C + 37]
    assert np.array_equal(c[0][C], a[0][C + 37]) and c[3][C] == a[3][C + 37]
    # the scene start with the flag, twice
    small = ss.unknown_board(rs.small_problem())
    assert same_bits(scene2(small, flag, None, 1), scene2(small, flag, None, 1))
