"""The whole-rig start at the scale the project measures: rsba_problem_start_rig on the 8 x 5000 x 16 synthetic marker-chain problem
(synthetic.make_marker_chain(8, 5000, 16, seed=11), as tools/marker_chain_scale.py) with its camera and time blocks zeroed, and, beside it,
the two-step start it replaces (rsba_problem_initial_time_poses + rsba_problem_initial_camera_poses, host code) on the same problem, where
camera 0 sees every shot — the only shape that start can handle.  A second rig in which camera 0 sees a quarter of the shots shows the
propagation at work.  Recorded, no bar: profiles/rig_start_scale.jsonl.

The kernel time of each round and sweep is taken by HIP events between the launches (the library records them under RSBA_RUNPROF=1 and prints
the intervals, the iteration-count histogram and the number of fits that ended at the cap to stderr, which is read back here); the whole
call, with its planning, allocation and copies, by the wall clock after one warm-up call.

    python tools/rig_start_scale.py [--out profiles/rig_start_scale.jsonl] [--repeat 3] [--sweeps 1]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from realsensecalibration_amd import capi, synthetic  # noqa: E402


def block_errors(params, prob):
    """Largest deviation of the camera / time blocks from the truth (as the six numbers; the generator's rotations are far from pi)."""
    C, T = prob["C"], prob["T"]
    d = np.abs(np.asarray(params).reshape(-1, 6)[:C + T] - np.asarray(prob["truth"]).reshape(-1, 6)[:C + T]).max(1)
    return float(d[:C].max()), float(np.median(d[C:])), float(d[C:].max())


def measure_start(prob, sweeps, repeat):
    C, T = prob["C"], prob["T"]
    p = capi.Problem.marker_chain(prob)
    start = p.params.copy()
    start[:6 * (C + T)] = 0.0
    p.params[:] = start
    p.start_rig(None, sweeps)                                # warm-up
    os.environ["RSBA_RUNPROF"] = "1"
    sys.stderr.flush()
    log, saved = tempfile.TemporaryFile(), os.dup(2)
    os.dup2(log.fileno(), 2)                                 # the library's stderr lines of the timed calls
    wall = []
    for _ in range(repeat):
        p.params[:] = start
        t0 = time.perf_counter()
        mt, mc, status, rms = p.start_rig(None, sweeps)
        wall.append(round(1e3 * (time.perf_counter() - t0), 3))
    os.dup2(saved, 2)
    os.close(saved)
    del os.environ["RSBA_RUNPROF"]
    log.seek(0)
    text = log.read().decode()
    own = [float(x) for x in re.findall(r"start_rig k_marker_pose: \d+ detections, ([0-9.]+) ms", text)]
    launches = re.findall(r"start_rig launch (\d+): (\w+) (\w+) (\d+), (\d+) blocks, (\d+) detections, ([0-9.]+) ms", text)
    per = len(launches) // repeat
    rows = []
    for k in range(per):
        reps = [float(launches[r * per + k][6]) for r in range(repeat)]
        _, which, kind, number, blocks, dets, _ = launches[k]
        rows.append(dict(launch=k, blocks_of=which, kind=kind, number=int(number), blocks=int(blocks), detections=int(dets), event_ms_repetitions=reps, event_ms_min=min(reps)))
    hist = re.findall(r"start_rig iterations by 25:([ 0-9]+); at the cap: (\d+)", text)[-1]
    cam_err, time_med, time_max = block_errors(p.params, prob)
    s = p.solve()
    out = dict(shape=[C, T, prob["M"]], detections=prob["N"], refine_sweeps=sweeps, missing_times=mt, missing_cameras=mc,
               status_counts=[int((status == k).sum()) for k in range(5)], own_fit_event_ms_min=min(own), launches=rows,
               kernels_event_ms_min_total=round(min(own) + sum(r["event_ms_min"] for r in rows), 4), call_wall_ms_repetitions=wall, call_wall_ms_min=min(wall),
               iterations_histogram_by_25=[int(v) for v in hist[0].split()], blocks_at_the_cap=int(hist[1]),
               block_rms_median_px=round(float(np.median(rms[rms >= 0])), 4), camera_error_max=cam_err, time_error_median=time_med, time_error_max=time_max,
               solve_after=dict(termination=int(s.termination_type), iterations=int(s.num_iterations), final_cost=float(s.final_cost)))
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=1)
    a = ap.parse_args()
    prob = synthetic.make_marker_chain(8, 5000, 16, seed=11)
    lines = [dict(line="start_rig_camera0_sees_everything", **measure_start(prob, a.sweeps, a.repeat))]
    lines.append(dict(line="start_rig_rounds_only", **measure_start(prob, 0, a.repeat)))
    # the two-step host start on the same problem
    C, T = prob["C"], prob["T"]
    p = capi.Problem.marker_chain(prob)
    p.params[:6 * (C + T)] = 0.0
    t0 = time.perf_counter()
    missing = p.initial_time_poses()
    t1 = time.perf_counter()
    p.initial_camera_poses()
    t2 = time.perf_counter()
    cam_err, time_med, time_max = block_errors(p.params, prob)
    s = p.solve()
    lines.append(dict(line="two_step_host_start", shape=[C, T, prob["M"]], missing_times=missing, initial_time_poses_ms=round(1e3 * (t1 - t0), 2),
                      initial_camera_poses_ms=round(1e3 * (t2 - t1), 2), camera_error_max=cam_err, time_error_median=time_med, time_error_max=time_max,
                      solve_after=dict(termination=int(s.termination_type), iterations=int(s.num_iterations), final_cost=float(s.final_cost))))
    p.close()
    # camera 0 sees the first quarter of the shots only: the two-step start leaves the rest, the propagation reaches them through camera 1
    import rig_start_ref as rs
    part = rs.keep_rows(prob, (np.asarray(prob["c"]) != 0) | (np.asarray(prob["t"]) < T // 4))
    lines.append(dict(line="start_rig_camera0_sees_a_quarter", **measure_start(part, a.sweeps, a.repeat)))
    q = capi.Problem.marker_chain(part)
    lines.append(dict(line="two_step_host_start_camera0_sees_a_quarter", missing_times=q.initial_time_poses()))
    q.close()
    text = "\n".join(json.dumps(x) for x in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
