"""rsba_problem_start_scene on the GPU: the whole-rig start with the marker blocks fitted too — k_block_resection's marker instance
(csrc/ba_resection.hpp, RESECT_MARKER), and its time and camera instances behind k_scene_mask_index, launched from the plan of
csrc/ba_scene_start_plan.hpp.  A resected marker is held to the minimiser of
the same cost with every other block constant (rig_start_ref.oracle_minimiser: the oracle started from the truth, only a step below
1e-11 (1 + |x|) ends it; with lens coefficients marker_distortion_ref's restatement) at 1e-6 per component, BASELINE's parameter bar, and to
the serial host fit of tests/scene_start_driver.cpp.  With the board unknown the start is judged by where rsba_solve ends from it: the cost
of the solve from the truth, at the bar of test_gpu_rig_start's propagation test.  tests/test_scene_start_plan_host.py runs the same
shapes serially on the CPU first.  The measured figures are in profiles/scene_start_accuracy.txt."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import rig_start_ref as rs
import scene_start_ref as ss
from realsensecalibration_amd import capi, synthetic as syn

pytestmark = pytest.mark.gpu
BAR = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ss.build_driver(tmp_path_factory.mktemp("scene_start_gpu"))


def scene(prob, model=1, known=None, sweeps=0, zero=()):
    """-> (blocks (C + T + M) x 6 after the call, (missing times, cameras, markers), status, rms); the blocks of `zero` are zeroed first."""
    p = capi.Problem.marker_chain(prob, model)
    for b in zero:
        p.params[6 * b:6 * b + 6] = 0.0
    mt, mc, mm, status, rms = p.start_scene(known, sweeps)
    out = p.params.copy().reshape(-1, 6)
    p.close()
    return out, (mt, mc, mm), status, rms


@pytest.mark.parametrize("name", sorted(ss.MARKER_CASES))
def test_marker_resection_against_the_oracle_and_the_host(driver, tmp_path, name):
    model, dist, prob, zeroed, known, free = ss.marker_case(name)
    nb = prob["C"] + prob["T"] + prob["M"]
    given = [b for b in range(nb) if b not in free]
    got, missing, status, rms = scene(prob, model, known, 0, zero=free)
    want = rs.oracle_minimiser(prob, model - 1, free, dist)
    host, host_rms, host_status, _ = ss.host_start(driver, tmp_path / "markers.txt", zeroed, model, known, 0)
    to_oracle, to_host = np.abs(got[free] - want[free]).max(1), np.abs(got[free] - host[free]).max(1)
    print("ACCURACY markers %s: device vs oracle %s | device vs host %s | status %s | rms %s" % (
        name, " ".join("%.3g" % v for v in to_oracle), " ".join("%.3g" % v for v in to_host), [int(v) for v in status[free]], " ".join("%.4f" % v for v in rms[free])))
    assert missing == (0, 0, 0) and list(status[given]) == [4] * len(given) and set(status[free]) <= {0, 1}
    assert np.array_equal(got[given], np.asarray(prob["params"], float).reshape(-1, 6)[given])   # every given block keeps its bits
    assert np.all(rms[given] == -1.0) and np.all(rms[free] > 0.0)
    assert to_host.max() < BAR and np.abs(rms - host_rms).max() < BAR and list(host_status) == list(status)
    assert to_oracle.max() < BAR


_EDGE = {}


def edge_problem():
    """9 x 40 x 4 with every marker in view kept: a marker is named by up to 360 detections."""
    if "p" not in _EDGE:
        _EDGE["p"] = syn.make_marker_chain(9, 40, 4, seed=62, keep=1.0)
    return _EDGE["p"]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_lane_edges_of_a_marker(n):
    """One marker with n detections (a workgroup's 256 lanes: one short, exact, one into the second trip of the stride loop), everything
    else given."""
    full = edge_problem()
    C, T, M = full["C"], full["T"], full["M"]
    m_all = np.asarray(full["m"])
    counts = [(m_all == m).sum() for m in range(M)]
    assert max(counts[1:]) >= 257, counts
    marker = next(m for m in range(1, M) if counts[m] >= 257)
    mask = m_all != marker
    mask[np.flatnonzero(m_all == marker)[:n]] = True
    prob = rs.keep_rows(full, mask)
    assert (np.asarray(prob["m"]) == marker).sum() == n
    block = C + T + marker
    known = [1] * (C + T + M)
    known[block] = 0
    got, missing, status, rms = scene(prob, 1, known, 0, zero=[block])
    want = rs.oracle_minimiser(prob, 0, [block])
    diff = np.abs(got[block] - want[block]).max()
    print("ACCURACY lane edges, a marker with %d detections: device vs oracle %.3g | status %d | rms %.4f" % (n, diff, status[block], rms[block]))
    assert missing == (0, 0, 0) and status[block] in (0, 1) and diff < BAR
    others = np.arange(C + T + M) != block
    assert np.array_equal(got[others], np.asarray(prob["params"], float).reshape(-1, 6)[others]) and set(status[others]) == {4}


def propagation_problem():
    """test_gpu_rig_start's: 4 x 12 x 6, camera 0 sees times 0-5, camera 1 all, camera 2 times 6-11, camera 3 times 4-7."""
    full = syn.make_marker_chain(4, 12, 6, seed=64)
    c, t = np.asarray(full["c"]), np.asarray(full["t"])
    keep = ((c == 0) & (t <= 5)) | ((c == 1) & (t <= 11)) | ((c == 2) & (t >= 6) & (t <= 11)) | ((c == 3) & (t >= 4) & (t <= 7))
    return rs.keep_rows(full, keep)


@pytest.mark.parametrize("which", ["propagation", "small"])
@pytest.mark.parametrize("sweeps", [0, 1])
def test_all_markers_flagged_equals_start_rig_bit_for_bit(which, sweeps):
    prob = propagation_problem() if which == "propagation" else rs.small_problem()
    C, T, M = prob["C"], prob["T"], prob["M"]
    p = capi.Problem.marker_chain(prob)
    p.params[:6 * (C + T)] = 0.0
    mt, mc, status, rms = p.start_rig(None, sweeps)
    rig = p.params.copy()
    p.close()
    got, missing, s_status, s_rms = scene(prob, 1, [0] * (C + T) + [1] * M, sweeps, zero=range(C + T))
    assert set(status[1:]) <= {0, 1} and rig[6:6 * (C + T)].reshape(-1, 6).any(1).all()          # start_rig fitted every block
    assert np.array_equal(got.ravel(), rig)
    assert np.array_equal(s_status[:C + T], status) and np.array_equal(s_rms[:C + T], rms) and missing == (mt, mc, 0)
    assert list(s_status[C + T:]) == [4] * M and np.all(s_rms[C + T:] == -1.0)


def test_place_and_repetition():
    """Two calls give the same bits everywhere; marker 3's detections alone (M = 2: the base marker and it) and the same marker as marker
    3 of 4 give the same bits for that block."""
    prob = rs.small_problem()
    C, T, M = prob["C"], prob["T"], prob["M"]
    a = scene(ss.unknown_board(prob), 1, None, 1)
    b = scene(ss.unknown_board(prob), 1, None, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[1] == b[1] == (0, 0, 0)
    known = [1] * (C + T) + [0] * M
    full = scene(prob, 1, known, 0, zero=range(C + T + 1, C + T + M))
    rows = np.asarray(prob["m"]) == 3
    assert rows.sum() >= 2
    alone = rs.keep_rows(prob, rows)
    alone["m"] = np.ones(alone["N"], np.int32)
    alone["M"] = 2
    blocks = np.asarray(prob["params"], float).reshape(-1, 6)
    alone["params"] = np.concatenate([blocks[:C + T + 1], np.zeros((1, 6))]).ravel()
    c = scene(alone, 1, [1] * (C + T) + [0, 0], 0)
    assert c[2][C + T + 1] in (0, 1) and c[2][C + T + 1] == full[2][C + T + 3]
    assert np.array_equal(c[0][C + T + 1], full[0][C + T + 3]) and c[3][C + T + 1] == full[3][C + T + 3]


@pytest.mark.parametrize("shape", [(3, 4, 4, 60, 1.0), (3, 6, 6, 7, 0.6)])
def test_board_unknown_end_to_end(shape):
    """Nothing flagged, every camera, time and non-base marker block zeroed: start_scene, then solve() with default options, against the
    solve from the truth (14.375649 and 19.22661 on these shapes)."""
    C, T, M, seed, keep = shape
    prob = syn.make_marker_chain(C, T, M, seed=seed, keep=keep)
    p = capi.Problem.marker_chain(ss.unknown_board(prob))
    assert not p.params.any()
    mt, mc, mm, status, rms = p.start_scene(refine_sweeps=1)
    print("ACCURACY board unknown %s: status %s rms %s" % (shape, [int(v) for v in status], " ".join("%.3f" % v for v in rms)))
    assert (mt, mc, mm) == (0, 0, 0) and status[0] == 4 and status[C + T] == 4 and set(np.delete(status, [0, C + T])) <= {0, 1}
    opts = capi.default_options()
    s = p.solve(opts)
    p.close()
    q = capi.Problem.marker_chain(dict(prob, params=np.asarray(prob["truth"], float).copy()))
    s_truth = q.solve(opts)
    q.close()
    print("ACCURACY board unknown %s: final cost %.12g in %d iterations; from the truth %.12g in %d" % (shape, s.final_cost, s.num_iterations, s_truth.final_cost, s_truth.num_iterations))
    assert s.termination_type == capi.CONVERGENCE and s_truth.termination_type == capi.CONVERGENCE
    assert abs(s.final_cost - s_truth.final_cost) <= 10.0 * opts.function_tolerance * s_truth.final_cost


def hongo():
    return capi.Problem.correspondence(os.path.join(ol.GOLDEN, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN,
                                       ol.read_intrinsics(ol.SERIALS_MAIN))


def test_hongo_with_part_of_its_board():
    """Markers 0-3 keep the committed geometry and are flagged; markers 4-10, all cameras and all times are zeroed."""
    p = hongo()
    Cn, T, M = p.num_cameras, p.num_times, p.num_markers
    assert M == 11
    p.params[:6 * (Cn + T)] = 0.0
    p.params[6 * (Cn + T + 4):] = 0.0
    known = [0] * (Cn + T) + [1] * 4 + [0] * (M - 4)
    mt, mc, mm, status, rms = p.start_scene(known)
    free = [b for b in range(1, Cn + T + M) if not Cn + T <= b < Cn + T + 4]
    assert (mt, mc, mm) == (0, 0, 0) and set(status[free]) <= {0, 1} and status[0] == 4 and list(status[Cn + T:Cn + T + 4]) == [4] * 4
    s = p.solve()
    print("ACCURACY hongo, markers 0-3 given: start status %s rms %s; final cost %.9f, %d iterations" % (
        [int(v) for v in status], " ".join("%.3f" % v for v in rms), s.final_cost, s.num_iterations))
    assert s.termination_type == capi.CONVERGENCE and abs(s.final_cost - 143.629388852) < 1.5e-3
    p.close()


def test_hongo_with_nothing_flagged_has_no_first_round():
    """Camera 0 never sees marker 0 in the committed file: no launch, every block unreached, all bits untouched."""
    p = hongo()
    Cn, T, M = p.num_cameras, p.num_times, p.num_markers
    before = p.params.copy()
    mt, mc, mm, status, rms = p.start_scene()
    want = np.full(Cn + T + M, 3)
    want[0] = want[Cn + T] = 4
    assert (mt, mc, mm) == (6, 3, 10) and np.array_equal(status, want) and np.all(rms == -1.0)
    assert np.array_equal(p.params, before)
    p.close()


def test_refusals():
    lib = capi.load()
    pts = capi.Problem.points(syn.make_problem(4, 50, 3, seed=1))
    with pytest.raises(capi.RsbaError) as e:
        pts.start_scene()
    assert e.value.code == capi.ERR_UNSUPPORTED
    pts.close()
    prob = rs.small_problem()
    nb = prob["C"] + prob["T"] + prob["M"]
    p = capi.Problem.marker_chain(prob)
    before = p.params.copy()
    status, rms = np.full(nb, 7, np.int32), np.full(nb, 7.0)
    mt, mc, mm = capi.C.c_int32(7), capi.C.c_int32(7), capi.C.c_int32(7)
    for sweeps, device in ((-1, -1), (0, 1 << 20), (0, -2)):
        assert lib.rsba_problem_start_scene(p.h, None, sweeps, device, capi.C.byref(mt), capi.C.byref(mc), capi.C.byref(mm), capi._vp(status),
                                            capi._vp(rms)) == capi.ERR_ARG
    assert lib.rsba_problem_start_scene(None, None, 0, -1, None, None, None, None, None) == capi.ERR_ARG
    assert np.array_equal(p.params, before) and np.all(status == 7) and np.all(rms == 7.0) and (mt.value, mc.value, mm.value) == (7, 7, 7)
    p.close()
