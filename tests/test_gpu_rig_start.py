"""rsba_problem_start_rig on the GPU: k_block_resection (csrc/ba_resection.hpp) launched from the plan of csrc/ba_rig_start_plan.hpp.
Problems come from synthetic.make_marker_chain with rows dropped to shape the co-visibility graph.  A resected block is held to the
minimiser of the same cost with every other block constant — oracle.solve_marker_chain_constant started from the truth, with tolerances
under which only a step below 1e-11 (1 + |x|) ends it; with lens coefficients, which that oracle does not take,
marker_distortion_ref's numpy restatement of the same minimisation — at 1e-6 per component, BASELINE's parameter bar, the bar of the
marker-pose tests.  The serial host fit is tests/rig_start_plan_driver.cpp's.

The resection's loop is FitMarkerPose's with one more test, that a step realise a quarter of the decrease its damped model predicts
(ba_marker_pose.hpp, MarkerPoseMinimise<true>): without it time 2 of the 3 x 4 x 4 problem — cameras and markers at the generator's start
values, 9.2 px RMS at the minimum — crept at the edge of stability and ended at the iteration cap 1.6e-4 from the oracle's minimiser.
The measured figures are in profiles/rig_start_accuracy.txt."""
import numpy as np
import pytest

import marker_distortion_ref as mdr
import marker_pose_ref as mp
import oracle_lib as ol
import rig_start_ref as rs
from realsensecalibration_amd import capi, synthetic as syn

pytestmark = pytest.mark.gpu
BAR = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return rs.build_driver(tmp_path_factory.mktemp("rig_start_gpu"))


def start(prob, model, known=None, sweeps=0, zero=()):
    """-> (blocks (C + T + M) x 6 after the call, missing times, missing cameras, status, rms); the blocks of `zero` are zeroed first."""
    p = capi.Problem.marker_chain(prob, model)
    for b in zero:
        p.params[6 * b:6 * b + 6] = 0.0
    mt, mc, status, rms = p.start_rig(known, sweeps)
    out = p.params.copy().reshape(-1, 6)
    p.close()
    return out, mt, mc, status, rms


def zero_rotation_problem():
    """3 x 4 x 4 without noise whose time 1 has a rotation of exactly zero: with cameras and markers at the truth the minimiser IS the
    truth, and the fit ends inside AngleAxisRotatePoint's first-order branch."""
    base = syn.make_marker_chain(3, 4, 4, seed=61, keep=1.0)
    C = base["C"]
    truth = np.asarray(base["truth"], float).copy()
    truth[6 * (C + 1):6 * (C + 1) + 3] = 0.0
    prob = mdr.redetect(dict(base, truth=truth), np.zeros((C, 5)), 0.0, 0)
    prob.pop("dist")
    prob["params"] = truth.copy()
    return prob


TIME_CASES = {"chain": (1, "pinhole"), "test2": (2, "pinhole"), "distorted": (1, "distorted"), "zero_rotation": (1, "zero")}


@pytest.mark.parametrize("name", sorted(TIME_CASES))
def test_time_resection_against_the_oracle_and_the_host(driver, tmp_path, name):
    model, config = TIME_CASES[name]
    dist = mp.DIST3.get(config)
    prob = zero_rotation_problem() if config == "zero" else rs.small_problem(dist)
    C, T = prob["C"], prob["T"]
    known = [1] * C + [0] * T
    times = range(C, C + T)
    got, mt, mc, status, rms = start(prob, model, known, 0, zero=times)
    want = rs.oracle_minimiser(prob, model - 1, times, dist)
    zeroed = dict(prob, params=np.asarray(prob["params"], float).copy())
    zeroed["params"][6 * C:6 * (C + T)] = 0.0
    host, host_rms, host_status, _ = rs.host_start(driver, tmp_path / "times.txt", zeroed, model, known, 0)
    to_oracle, to_host = np.abs(got[C:C + T] - want[C:C + T]).max(1), np.abs(got[C:C + T] - host[C:]).max(1)
    print("ACCURACY times %s: device vs oracle %s | device vs host %s | status %s | rms %s" % (
        name, " ".join("%.3g" % v for v in to_oracle), " ".join("%.3g" % v for v in to_host), list(status[C:]), " ".join("%.4f" % v for v in rms[C:])))
    assert (mt, mc) == (0, 0) and list(status[:C]) == [4] * C and set(status[C:]) <= {0, 1}
    assert np.array_equal(got[:C], np.asarray(prob["params"]).reshape(-1, 6)[:C]) and np.array_equal(got[C + T:], np.asarray(prob["params"]).reshape(-1, 6)[C + T:])
    assert np.all(rms[:C] == -1.0) and np.all(rms[C:] > 0.0 if config != "zero" else rms[C:] >= 0.0)
    if config == "zero":
        assert np.abs(got[C + 1, :3]).max() < 1.4e-8   # theta^2 <= DBL_EPSILON: the first-order branch
    assert to_host.max() < BAR and np.abs(rms[C:] - host_rms[C:]).max() < BAR and list(host_status) == list(status)
    assert to_oracle.max() < BAR


@pytest.mark.parametrize("model,config", [(1, "pinhole"), (2, "pinhole"), (1, "distorted")])
def test_camera_resection_against_the_oracle(model, config):
    """Times given, cameras 1 and above zeroed; camera 2 keeps the detections of ONE shot only: one board in one shot, the kind of
    input the coplanar EPnP entry refuses (the generator's board is a few millimetres off its plane, so that entry is not asked here)."""
    dist = mp.DIST3[config]
    full = rs.small_problem(dist)
    prob = rs.keep_rows(full, (np.asarray(full["c"]) != 2) | (np.asarray(full["t"]) == 1))
    C, T = prob["C"], prob["T"]
    assert set(np.asarray(prob["t"])[np.asarray(prob["c"]) == 2]) == {1}
    known = [0] * C + [1] * T
    got, mt, mc, status, rms = start(prob, model, known, 0, zero=range(1, C))
    want = rs.oracle_minimiser(prob, model - 1, range(1, C), dist)
    diff = np.abs(got[1:C] - want[1:C]).max(1)
    print("ACCURACY cameras model %d %s: device vs oracle %s | status %s | rms %s" % (model, config, " ".join("%.3g" % v for v in diff), list(status[:C]),
                                                                                  " ".join("%.4f" % v for v in rms[:C])))
    assert (mt, mc) == (0, 0) and status[0] == 4 and set(status[1:C]) <= {0, 1} and list(status[C:]) == [4] * T
    assert np.array_equal(got[C:], np.asarray(prob["params"]).reshape(-1, 6)[C:]) and not got[0].any()
    assert diff.max() < BAR


_EDGE = {}


def edge_problem():
    """9 x 24 x 16 with every marker in view kept: a time has up to 144 detections, a camera up to 384."""
    if "p" not in _EDGE:
        _EDGE["p"] = syn.make_marker_chain(9, 24, 16, seed=62, keep=1.0)
    return _EDGE["p"]


def test_lane_edges_of_a_time():
    """Single times with exactly 1, 2, 63, 64, 65 and 129 detections (the second trip of a wavefront's stride loop), all cameras given."""
    full = edge_problem()
    C, T = full["C"], full["T"]
    t_all = np.asarray(full["t"])
    rich = sorted(range(T), key=lambda t: -(t_all == t).sum())[:6]
    counts = dict(zip(rich, [129, 65, 64, 63, 2, 1]))
    assert all((t_all == t).sum() >= n for t, n in counts.items()), [(t_all == t).sum() for t in range(T)]
    mask = np.zeros(full["N"], bool)
    for t, n in counts.items():
        mask[np.flatnonzero(t_all == t)[:n]] = True
    prob = rs.keep_rows(full, mask)
    known = [1] * C + [0] * T
    blocks = [C + t for t in counts]
    got, mt, mc, status, rms = start(prob, 1, known, 0, zero=range(C, C + T))
    want = rs.oracle_minimiser(prob, 0, blocks)
    diff = np.abs(got[blocks] - want[blocks]).max(1)
    print("ACCURACY lane edges, times with %s detections: device vs oracle %s | status %s" % (list(counts.values()), " ".join("%.3g" % v for v in diff), list(status[blocks])))
    assert mt == T - 6 and mc == 0 and set(status[blocks]) <= {0, 1}
    others = [C + t for t in range(T) if t not in counts]
    assert set(status[others]) == {3} and not got[others].any() and np.all(rms[others] == -1.0)
    assert diff.max() < BAR


@pytest.mark.parametrize("n", [255, 256, 257])
def test_lane_edges_of_a_camera(n):
    """One camera with n detections (a workgroup's 256 lanes: one short, exact, one into the second trip), the times given."""
    full = edge_problem()
    C, T = full["C"], full["T"]
    c_all = np.asarray(full["c"])
    cam = next(c for c in range(1, C) if (c_all == c).sum() >= 257)
    mask = c_all != cam
    mask[np.flatnonzero(c_all == cam)[:n]] = True
    prob = rs.keep_rows(full, mask)
    known = [1] * C + [1] * T
    known[cam] = 0
    got, mt, mc, status, rms = start(prob, 1, known, 0, zero=[cam])
    want = rs.oracle_minimiser(prob, 0, [cam])
    diff = np.abs(got[cam] - want[cam]).max()
    print("ACCURACY lane edges, a camera with %d detections: device vs oracle %.3g | status %d | rms %.4f" % (n, diff, status[cam], rms[cam]))
    assert (mt, mc) == (0, 0) and status[cam] in (0, 1) and diff < BAR


def test_place_and_repetition():
    """One time's detections alone (T = 1) and as time 37 of 65 give the same bits for that block; two calls give the same bits everywhere."""
    full = syn.make_marker_chain(3, 65, 4, seed=63)
    C, T = full["C"], full["T"]
    known = [1] * C + [0] * T
    a = start(full, 1, known, 1, zero=range(C, C + T))
    b = start(full, 1, known, 1, zero=range(C, C + T))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[1:3] == b[1:3]
    rows = np.asarray(full["t"]) == 37
    assert rows.sum() >= 2
    alone = rs.keep_rows(full, rows)
    alone["t"] = np.zeros(alone["N"], np.int32)
    alone["T"] = 1
    blocks = np.asarray(full["params"], float).reshape(-1, 6)
    alone["params"] = np.concatenate([blocks[:C], np.zeros((1, 6)), blocks[C + T:]]).ravel()
    c = start(alone, 1, [1] * C + [0], 1)
    assert c[3][C] in (0, 1) and c[3][C] == a[3][C + 37]
    assert np.array_equal(c[0][C], a[0][C + 37]) and c[4][C] == a[4][C + 37]


def propagation_problem(extra_camera=False):
    """4 x 12 x 6: camera 0 sees times 0-5, camera 1 all, camera 2 times 6-11, camera 3 times 4-7.  extra_camera: a camera 4 that sees
    only a time 12 nobody else sees."""
    C, T = (5, 13) if extra_camera else (4, 12)
    full = syn.make_marker_chain(C, T, 6, seed=64)
    c, t = np.asarray(full["c"]), np.asarray(full["t"])
    keep = ((c == 0) & (t <= 5)) | ((c == 1) & (t <= 11)) | ((c == 2) & (t >= 6) & (t <= 11)) | ((c == 3) & (t >= 4) & (t <= 7)) | ((c == 4) & (t == 12))
    return rs.keep_rows(full, keep)


def test_propagation_starts_what_camera_zero_does_not_see():
    prob = propagation_problem()
    C, T = prob["C"], prob["T"]
    p = capi.Problem.marker_chain(prob)
    p.params[:6 * (C + T)] = 0.0
    assert p.initial_time_poses() == 6                      # the parent's start: times 6-11 stay as they are
    p.params[:6 * (C + T)] = 0.0
    mt, mc, status, rms = p.start_rig()
    print("PROPAGATION status %s rms %s" % (list(status), " ".join("%.3f" % v for v in rms)))
    assert (mt, mc) == (0, 0) and status[0] == 4 and set(status[1:]) <= {0, 1}
    opts = capi.default_options()
    s = p.solve(opts)
    p.close()
    q = capi.Problem.marker_chain(dict(prob, params=np.asarray(prob["truth"], float).copy()))
    s_truth = q.solve(opts)
    q.close()
    print("PROPAGATION final cost %.12g in %d iterations; from the truth %.12g in %d" % (s.final_cost, s.num_iterations, s_truth.final_cost, s_truth.num_iterations))
    assert s.termination_type == capi.CONVERGENCE and s_truth.termination_type == capi.CONVERGENCE
    assert abs(s.final_cost - s_truth.final_cost) <= 10.0 * opts.function_tolerance * s_truth.final_cost


def test_a_camera_without_a_shared_shot_is_unreached():
    prob = propagation_problem(extra_camera=True)
    C, T = prob["C"], prob["T"]
    assert (np.asarray(prob["c"]) == 4).sum() > 0
    before = np.asarray(prob["params"], float).reshape(-1, 6)
    got, mt, mc, status, rms = start(prob, 1)
    assert (mt, mc) == (1, 1) and status[4] == 3 and status[C + 12] == 3 and rms[4] == -1.0
    assert np.array_equal(got[4], before[4]) and np.array_equal(got[C + 12], before[C + 12])
    assert set(status[1:4]) <= {0, 1} and set(status[C:C + 12]) <= {0, 1}


def test_hongo_from_the_corners():
    import os
    hongo = os.path.join(ol.GOLDEN, "hongo", "correspondence.txt")
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    p = capi.Problem.correspondence(hongo, capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    Cn, T = p.num_cameras, p.num_times
    p.params[:6 * (Cn + T)] = 0.0
    mt, mc, status, rms = p.start_rig()
    assert (mt, mc) == (0, 0) and set(status[1:]) <= {0, 1}
    s = p.solve()
    print("HONGO start status %s rms %s; final cost %.9f, %d iterations" % (list(status), " ".join("%.3f" % v for v in rms), s.final_cost, s.num_iterations))
    assert s.termination_type == capi.CONVERGENCE and abs(s.final_cost - 143.629388852) < 1.5e-3
    p.close()


AMBIGUOUS_SEED = 9   # searched on the CPU with rsba_marker_pose_from_corners over seeds 0-59: the small marker's own fit ends 0.658 rad
                     # from the truth with an RMS of 0.034 px, below the second marker's 0.068 px — it is the FIRST candidate


def ambiguous_problem():
    """One time seen by the base camera: marker 0 small, far and nearly frontal (10 pixels at 3 m, tilted 0.32 rad), marker 1 2.2 m nearer
    and turned."""
    import marker_loss_ref as ref
    time = np.array([0.25, -0.2, 0.02, 0.05, -0.04, 3.0])
    m1 = np.array([0.6, 0.3, 0.0, 0.2, 0.1, -2.2])
    truth = np.concatenate([np.zeros(6), time, np.zeros(6), m1])
    prob = dict(C=1, T=1, M=2, N=2, t=np.zeros(2, np.int32), c=np.zeros(2, np.int32), m=np.array([0, 1], np.int32), obs=np.zeros((2, 8)),
                params=truth.copy(), truth=truth, intr=np.array([[615.0, 615.0, 320.0, 240.0]]), marker_side=0.05)
    proj = ref.MarkerChain(prob).residuals(truth.reshape(-1, 6))
    prob["obs"] = proj + np.random.default_rng([AMBIGUOUS_SEED, 0xA3B]).normal(0, 0.3, proj.shape)
    return prob


def test_a_second_detection_resolves_the_first_candidates_ambiguity():
    prob = ambiguous_problem()
    own, own_rms, _ = capi.marker_pose_from_corners(prob["obs"][0], prob["intr"][0], None, prob["marker_side"])
    second_rms = capi.marker_pose_from_corners(prob["obs"][1], prob["intr"][0], None, prob["marker_side"])[1]
    Ra, Rb = mp._rodrigues(own[:3]), mp._rodrigues(prob["truth"][6:9])
    angle = float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))
    assert angle > 0.1 and own_rms < second_rms, (angle, own_rms, second_rms)   # the precondition: the first candidate sits in the wrong basin
    got, mt, mc, status, rms = start(prob, 1, None, 0, zero=[1])
    want = rs.oracle_minimiser(prob, 0, [1])
    print("AMBIGUOUS own fit %.3f rad from the truth; resected time vs oracle %.3g, status %d, rms %.4f" % (angle, np.abs(got[1] - want[1]).max(), status[1], rms[1]))
    assert (mt, mc) == (0, 0) and status[1] in (0, 1)
    assert np.abs(got[1] - want[1]).max() < BAR


def test_refusals():
    lib = capi.load()
    pts = capi.Problem.points(syn.make_problem(4, 50, 3, seed=1))
    with pytest.raises(capi.RsbaError) as e:
        pts.start_rig()
    assert e.value.code == capi.ERR_UNSUPPORTED
    pts.close()
    prob = rs.small_problem()
    C, T = prob["C"], prob["T"]
    p = capi.Problem.marker_chain(prob)
    before = p.params.copy()
    status, rms, mt = np.full(C + T, 7, np.int32), np.full(C + T, 7.0), capi.C.c_int32(7)
    for sweeps, device in ((-1, -1), (0, 1 << 20), (0, -2)):
        assert lib.rsba_problem_start_rig(p.h, None, sweeps, device, capi.C.byref(mt), None, capi._vp(status), capi._vp(rms)) == capi.ERR_ARG
    assert lib.rsba_problem_start_rig(None, None, 0, -1, None, None, None, None) == capi.ERR_ARG
    assert np.array_equal(p.params, before) and np.all(status == 7) and np.all(rms == 7.0) and mt.value == 7
    p.close()
    # a time whose detections are all collapsed to a point
    known = [1] * C + [0] * T
    clean = start(prob, 1, known, 0, zero=range(C, C + T))
    bad = dict(prob, obs=np.asarray(prob["obs"], float).copy())
    rows = np.asarray(prob["t"]) == 2
    bad["obs"][rows] = np.tile(bad["obs"][rows][:, :2], 4)
    got, mt, mc, status, rms = start(bad, 1, known, 0, zero=range(C, C + T))
    assert (mt, mc) == (1, 0) and status[C + 2] == 2 and rms[C + 2] == -1.0 and not got[C + 2].any()
    keep = np.arange(C + T) != C + 2
    assert np.array_equal(got[:C + T][keep], clean[0][:C + T][keep]) and np.array_equal(status[keep], clean[3][keep]) and np.array_equal(rms[keep], clean[4][keep])
