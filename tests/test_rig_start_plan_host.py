"""The host units of the whole-rig start under AddressSanitizer and UBSan: tests/rig_start_plan_driver.cpp, a stand-alone program, is
compiled with -fsanitize=address,undefined and run as a child process.
  * the planner (csrc/ba_rig_start_plan.hpp) on crafted co-visibility graphs: the driver checks the lists' invariants, the launches' blocks,
    grids and byte counts and the buffers itself and prints what it planned; that is held against tests/rig_start_ref.py, a restatement of
    the rounds written from the rule, and against the rounds each graph was crafted to need;
  * the fit (csrc/ba_resection.hpp): the RSBA_HD accumulation and the shared Levenberg-Marquardt step run serially, summing in observation
    order, on a 3-camera, 4-time, 4-marker problem, both wirings and a distorted lens, and must land on the oracle's minimiser with every
    other block constant at 1e-6 per component (BASELINE's parameter bar) — the result tests/test_gpu_rig_start.py holds the kernel to.
Nothing loaded into Python is sanitised.

MEASURED: 2.1e-8 to 1.6e-7 from the oracle for the times (55 to 202 steps), 4e-13 to 5e-11 for the cameras (7 to 17 steps)."""
import numpy as np
import pytest

import marker_pose_ref as mp
import rig_start_ref as rs


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return rs.build_driver(tmp_path_factory.mktemp("rig_start"))


def test_planned_rounds_are_the_rule(driver, tmp_path):
    graphs = rs.graphs()
    path = tmp_path / "graphs.txt"
    with open(path, "w") as f:
        for C, T, M, cam, tim, known, sweeps, _ in graphs.values():
            f.write("%d %d %d %d %d %d\n" % (C, T, M, len(cam), sweeps, 0 if known is None else 1))
            if known is not None:
                f.write(" ".join(str(v) for v in known) + "\n")
            f.write("".join("%d %d\n" % (c, t) for c, t in zip(cam, tim)))
    lines = rs.run_driver(driver, ["plan", str(path)])
    assert len(lines) == len(graphs)
    for (name, (C, T, M, cam, tim, known, sweeps, (kinds, un_t, un_c))), line in zip(graphs.items(), lines):
        want = rs.plan(C, T, cam, tim, known, sweeps)
        got = [(l["which"], l["sweep"], l["blocks"]) for l in line["launches"]]
        assert got == want["launches"], (name, got, want["launches"])
        assert line["num_rounds"] == want["num_rounds"] == len(kinds), name
        assert [l["which"] for l in line["launches"][:len(kinds)]] == kinds, name
        assert line["unreachable_times"] == want["unreachable_times"] == un_t, name
        assert line["unreachable_cameras"] == want["unreachable_cameras"] == un_c, name
        for l in line["launches"]:
            assert l["grid"] == ((len(l["blocks"]) + 3) // 4 if l["which"] == rs.TIME else len(l["blocks"])), name
        assert (line["time_ptr"], line["time_obs"]) == rs.csr(T, tim), name
        assert (line["camera_ptr"], line["camera_obs"]) == rs.csr(C, cam), name


def test_empty_problems_and_refused_arguments(driver):
    assert rs.run_driver(driver) == []


@pytest.mark.parametrize("model,config", [(1, "pinhole"), (2, "pinhole"), (1, "distorted")])
def test_serial_fit_lands_on_the_oracles_minimiser(driver, tmp_path, model, config):
    dist = mp.DIST3[config]
    prob = rs.small_problem(dist)
    C, T = prob["C"], prob["T"]
    # times from known cameras
    p1 = dict(prob, params=np.asarray(prob["params"], float).copy())
    p1["params"][6 * C:6 * (C + T)] = 0.0
    known = [1] * C + [0] * T
    blocks, rms, status, iters = rs.host_start(driver, tmp_path / "times.txt", p1, model, known, 0)
    want = rs.oracle_minimiser(prob, model - 1, range(C, C + T), dist)
    print("HOST times model %d %s: difference per time %s, iterations %s, status %s"
          % (model, config, " ".join("%.3g" % v for v in np.abs(blocks[C:] - want[C:C + T]).max(1)), iters[C:], status[C:]))
    assert list(status) == [4] * C + [0] * T
    assert np.abs(blocks[C:] - want[C:C + T]).max() < 1e-6
    assert np.array_equal(blocks[:C], np.asarray(prob["params"]).reshape(-1, 6)[:C]) and np.all(rms[:C] == -1) and np.all(rms[C:] > 0)
    # cameras from known times
    p2 = dict(prob, params=np.asarray(prob["params"], float).copy())
    p2["params"][6:6 * C] = 0.0
    known = [0] * C + [1] * T
    blocks, rms, status, iters = rs.host_start(driver, tmp_path / "cameras.txt", p2, model, known, 0)
    want = rs.oracle_minimiser(prob, model - 1, range(1, C), dist)
    print("HOST cameras model %d %s: difference per camera %s, iterations %s, status %s"
          % (model, config, " ".join("%.3g" % v for v in np.abs(blocks[1:C] - want[1:C]).max(1)), iters[1:C], status[1:C]))
    assert list(status) == [4] + [0] * (C - 1) + [4] * T
    assert np.abs(blocks[1:C] - want[1:C]).max() < 1e-6
