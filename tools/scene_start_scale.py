"""The scene start at the scale the project measures: rsba_problem_start_scene on the 8 x 5000 x 16 synthetic marker-chain problem
(synthetic.make_marker_chain(8, 5000, 16, seed=11), as tools/rig_start_scale.py) with the board unknown — every camera, time and non-base
marker block zeroed, nothing flagged — and, beside it, rsba_problem_start_rig on the same problem with the board given.  Each launch's
time, and where rsba_solve ends from each start.  Recorded, no bar: profiles/scene_start_scale.jsonl.

The kernel time of each round and sweep is taken by HIP events between the launches (the library records them under RSBA_RUNPROF=1 and
prints the intervals to stderr, which is read back here); the whole call, with its planning, allocation and copies, by the wall clock after
one warm-up call.

    python tools/scene_start_scale.py [--out profiles/scene_start_scale.jsonl] [--repeat 3] [--sweeps 1]
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
from realsensecalibration_amd import capi, synthetic  # noqa: E402


def measure(prob, entry, sweeps, repeat):
    """entry: "start_scene" (board unknown) or "start_rig" (board given)."""
    C, T, M = prob["C"], prob["T"], prob["M"]
    p = capi.Problem.marker_chain(prob)
    start = p.params.copy()
    start[:6 * (C + T)] = 0.0
    if entry == "start_scene":
        start[6 * (C + T + 1):] = 0.0
    call = (lambda: p.start_scene(None, sweeps)) if entry == "start_scene" else (lambda: p.start_rig(None, sweeps))
    p.params[:] = start
    call()                                                   # warm-up
    os.environ["RSBA_RUNPROF"] = "1"
    sys.stderr.flush()
    log, saved = tempfile.TemporaryFile(), os.dup(2)
    os.dup2(log.fileno(), 2)                                 # the library's stderr lines of the timed calls
    wall = []
    for _ in range(repeat):
        p.params[:] = start
        t0 = time.perf_counter()
        result = call()
        wall.append(round(1e3 * (time.perf_counter() - t0), 3))
    os.dup2(saved, 2)
    os.close(saved)
    del os.environ["RSBA_RUNPROF"]
    log.seek(0)
    text = log.read().decode()
    status, rms = result[-2], result[-1]
    own = [float(x) for x in re.findall(entry + r" k_marker_pose: \d+ detections, ([0-9.]+) ms", text)]
    launches = re.findall(entry + r" launch (\d+): (\w+) (\w+) (\d+), (\d+) blocks, (\d+) detections, ([0-9.]+) ms", text)
    per = len(launches) // repeat
    rows = []
    for k in range(per):
        reps = [float(launches[r * per + k][6]) for r in range(repeat)]
        _, which, kind, number, blocks, dets, _ = launches[k]
        rows.append(dict(launch=k, blocks_of=which, kind=kind, number=int(number), blocks=int(blocks), detections=int(dets), event_ms_repetitions=reps, event_ms_min=min(reps)))
    hist = re.findall(entry + r" iterations by 25:([ 0-9]+); at the cap: (\d+)", text)[-1]
    d = np.abs(p.params.reshape(-1, 6) - np.asarray(prob["truth"]).reshape(-1, 6)).max(1)
    s = p.solve()
    out = dict(entry=entry, board="unknown" if entry == "start_scene" else "given", shape=[C, T, M], detections=prob["N"], refine_sweeps=sweeps,
               missing=[int(v) for v in result[:-2]], status_counts=[int((status == k).sum()) for k in range(5)], own_fit_event_ms_min=min(own), launches=rows,
               kernels_event_ms_min_total=round(min(own) + sum(r["event_ms_min"] for r in rows), 4), call_wall_ms_repetitions=wall, call_wall_ms_min=min(wall),
               iterations_histogram_by_25=[int(v) for v in hist[0].split()], blocks_at_the_cap=int(hist[1]),
               block_rms_median_px=round(float(np.median(rms[rms >= 0])), 4), camera_error_max=float(d[:C].max()), time_error_median=float(np.median(d[C:C + T])),
               time_error_max=float(d[C:C + T].max()), marker_error_max=float(d[C + T:].max()),
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
    lines = [dict(line="start_scene_board_unknown", **measure(prob, "start_scene", a.sweeps, a.repeat)),
             dict(line="start_rig_board_given", **measure(prob, "start_rig", a.sweeps, a.repeat))]
    q = capi.Problem.marker_chain(dict(prob, params=np.asarray(prob["truth"], float).copy()))
    s = q.solve()
    q.close()
    lines.append(dict(line="solve_from_the_truth", termination=int(s.termination_type), iterations=int(s.num_iterations), final_cost=float(s.final_cost)))
    text = "\n".join(json.dumps(x) for x in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
