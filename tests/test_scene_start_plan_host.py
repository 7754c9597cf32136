"""The host units of the scene start under AddressSanitizer and UBSan: tests/scene_start_driver.cpp, a stand-alone program, is compiled
with -fsanitize=address,undefined and run as a child process.
  * the planner (csrc/ba_scene_start_plan.hpp) on crafted graphs: the driver checks the lists' invariants, the launches' blocks, grids and
    byte counts, the buffers and — with every marker flagged — the equality with PlanRigStart itself, and prints what it planned; that is
    held against tests/scene_start_ref.py, a restatement of the three-kind rule written from the rule, against the rounds each graph was
    crafted to need, and on rig_start_ref's graphs with the board given against rig_start_ref.plan;
  * the marker fit (csrc/ba_resection.hpp, RESECT_MARKER) run serially on the 3 x 4 x 4 problem, cameras and times given, markers 1-3
    zeroed: it must land on the oracle's minimiser with every other block constant at 1e-6 per component (BASELINE's parameter bar);
  * the whole start with the board unknown, serially, then the oracle's solve: the shapes the GPU test relies on reach the cost of the
    solve from the truth.
Nothing loaded into Python is sanitised.

MEASURED (host): markers 1-3 against the oracle 3.6e-9 to 9.2e-8 in 15 to 18 steps (both wirings), 5.2e-11 to 1.0e-8 in 16 to 22 (distorted).
Board unknown: 14.3756485 against 14.375649 from the truth (3 x 4 x 4), 19.2266108 against 19.2266176 (3 x 6 x 6, keep 0.6); hongo with
markers 0-3 given: 143.629399127."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import rig_start_ref as rs
import scene_start_ref as ss
from realsensecalibration_amd import synthetic as syn


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ss.build_driver(tmp_path_factory.mktemp("scene_start"))


def test_the_restatement_on_the_crafted_graphs():
    """The rule in Python against the launch sequences stated in words (no compiled code involved)."""
    for name, (C, T, M, cam, tim, mar, known, sweeps, base, (kinds, un_t, un_c, un_m)) in ss.graphs().items():
        got = ss.plan(C, T, M, cam, tim, mar, known, sweeps, base)
        assert [l[0] for l in got["launches"][:got["num_rounds"]]] == kinds, name
        assert (got["unreachable_times"], got["unreachable_cameras"], got["unreachable_markers"]) == (un_t, un_c, un_m), name
        assert len(got["launches"]) == got["num_rounds"] + sweeps * len(set(kinds)), name


def test_planned_rounds_are_the_rule(driver, tmp_path):
    graphs = ss.graphs()
    path = tmp_path / "graphs.txt"
    ss.write_plan_cases(path, [g[:9] for g in graphs.values()])
    lines = ss.run_driver(driver, ["plan", str(path)])
    assert len(lines) == len(graphs)
    for (name, (C, T, M, cam, tim, mar, known, sweeps, base, (kinds, un_t, un_c, un_m))), line in zip(graphs.items(), lines):
        want = ss.plan(C, T, M, cam, tim, mar, known, sweeps, base)
        got = [(l["which"], l["sweep"], l["blocks"]) for l in line["launches"]]
        assert got == want["launches"], (name, got, want["launches"])
        assert line["num_rounds"] == want["num_rounds"] == len(kinds), name
        assert [l["which"] for l in line["launches"][:len(kinds)]] == kinds, name
        assert line["unreachable_times"] == want["unreachable_times"] == un_t, name
        assert line["unreachable_cameras"] == want["unreachable_cameras"] == un_c, name
        assert line["unreachable_markers"] == want["unreachable_markers"] == un_m, name
        for l in line["launches"]:
            assert l["grid"] == ((len(l["blocks"]) + 3) // 4 if l["which"] == ss.TIME else len(l["blocks"])), name
        assert (line["time_ptr"], line["time_obs"]) == rs.csr(T, tim), name
        assert (line["camera_ptr"], line["camera_obs"]) == rs.csr(C, cam), name
        assert (line["marker_ptr"], line["marker_obs"]) == rs.csr(M, mar), name


def test_the_board_given_plans_what_the_rig_start_plans(driver, tmp_path):
    graphs = ss.rig_graphs_with_the_board_given()
    path = tmp_path / "rig_graphs.txt"
    ss.write_plan_cases(path, [(C, T, M, cam, tim, mar, known, sweeps, True) for C, T, M, cam, tim, mar, known, sweeps, _ in graphs.values()])
    lines = ss.run_driver(driver, ["plan", str(path)])
    assert len(lines) == len(graphs) == len(rs.graphs())
    for (name, (C, T, M, cam, tim, mar, known, sweeps, rig_known)), line in zip(graphs.items(), lines):
        want = rs.plan(C, T, cam, tim, rig_known, sweeps)
        got = [(l["which"], l["sweep"], l["blocks"]) for l in line["launches"]]
        assert got == want["launches"] == ss.plan(C, T, M, cam, tim, mar, known, sweeps)["launches"], name
        assert line["num_rounds"] == want["num_rounds"], name
        assert (line["unreachable_times"], line["unreachable_cameras"], line["unreachable_markers"]) == (want["unreachable_times"], want["unreachable_cameras"], []), name


def test_empty_problems_and_refused_arguments(driver):
    assert ss.run_driver(driver) == []


@pytest.mark.parametrize("name", sorted(ss.MARKER_CASES))
def test_serial_marker_fit_lands_on_the_oracles_minimiser(driver, tmp_path, name):
    model, dist, prob, zeroed, known, free = ss.marker_case(name)
    C, T, M = prob["C"], prob["T"], prob["M"]
    blocks, rms, status, iters = ss.host_start(driver, tmp_path / "markers.txt", zeroed, model, known, 0)
    want = rs.oracle_minimiser(prob, model - 1, free, dist)
    diff = np.abs(blocks[free] - want[free]).max(1)
    print("HOST markers %s: difference per marker %s, iterations %s, status %s, rms %s"
          % (name, " ".join("%.3g" % v for v in diff), iters[free], status[free], " ".join("%.4f" % v for v in rms[free])))
    assert list(status) == [4] * (C + T + 1) + [0] * (M - 1)
    assert diff.max() < 1e-6
    given = [b for b in range(C + T + M) if b not in free]
    assert np.array_equal(blocks[given], np.asarray(prob["params"]).reshape(-1, 6)[given]) and np.all(rms[given] == -1) and np.all(rms[free] > 0)


def solve_from(prob, params):
    """The oracle's solve of the chain model with default options from params -> (final cost, iterations)."""
    o = ol.load()
    _, s, _ = o.solve_marker_chain(dict(prob, params=np.asarray(params, float).ravel().copy()), 0, prob["marker_side"], np.asarray(prob["intr"], float).ravel())
    return s.final_cost, s.num_iterations


@pytest.mark.parametrize("shape", [(3, 4, 4, 60, 1.0), (3, 6, 6, 7, 0.6)])
def test_board_unknown_on_the_host_reaches_the_truths_cost(driver, tmp_path, shape):
    """The shapes of the GPU end-to-end test: nothing flagged, every block zeroed, the start run serially with one sweep, then the
    oracle's solve; the bar is that test's, 10 x function_tolerance x cost."""
    C, T, M, seed, keep = shape
    prob = syn.make_marker_chain(C, T, M, seed=seed, keep=keep)
    blocks, rms, status, _ = ss.host_start(driver, tmp_path / "scene.txt", ss.unknown_board(prob), 1, None, 1)
    assert status[0] == 4 and status[C + T] == 4 and set(np.delete(status, [0, C + T])) <= {0, 1}, list(status)
    cost, its = solve_from(prob, blocks)
    truth_cost, truth_its = solve_from(prob, prob["truth"])
    print("HOST board unknown %s: final cost %.9g in %d iterations; from the truth %.9g in %d" % (shape, cost, its, truth_cost, truth_its))
    assert abs(cost - truth_cost) <= 10.0 * ol.load().options().function_tolerance * truth_cost


def hongo_problem():
    """The committed hongo file as the generator's dictionaries carry a problem."""
    prob = ol.read_correspondence(os.path.join(ol.GOLDEN, "hongo", "correspondence.txt"))
    return dict(prob, obs=prob["obs"].reshape(-1, 8), intr=ol.read_intrinsics(ol.SERIALS_MAIN), marker_side=ol.MARKER_SIDE_MAIN)


def test_hongo_with_part_of_its_board_on_the_host(driver, tmp_path):
    """Markers 0-3 of the committed geometry flagged, everything else zeroed: the serial start, then the oracle's solve, against the bar of
    test_hongo_from_the_corners."""
    prob = hongo_problem()
    C, T, M = prob["C"], prob["T"], prob["M"]
    known = [0] * (C + T) + [1] * 4 + [0] * (M - 4)
    start = dict(prob, params=prob["params"].copy())
    start["params"][:6 * (C + T)] = 0.0
    start["params"][6 * (C + T + 4):] = 0.0
    blocks, rms, status, _ = ss.host_start(driver, tmp_path / "hongo.txt", start, 1, known, 1)
    free = [b for b in range(1, C + T + M) if not (C + T <= b < C + T + 4)]
    assert set(status[free]) <= {0, 1}, list(status)
    cost, its = solve_from(prob, blocks)
    print("HOST hongo, markers 0-3 given: start status %s; final cost %.9f in %d iterations" % (list(status), cost, its))
    assert abs(cost - 143.629388852) < 1.5e-3
