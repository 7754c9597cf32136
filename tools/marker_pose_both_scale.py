"""Both poses of a planar marker at the scale the project measures, and what the flagged starts buy.  Recorded, no bar:
profiles/marker_pose_both_scale.jsonl (the text of profiles/marker_pose_both_accuracy.txt quotes it).

  kernels    k_marker_pose and k_marker_pose_mirror on the detections of synthetic.make_marker_chain(8, 5000, 16, seed=11) in one call of
             rsba_marker_poses_from_corners_both; the statuses of solution 1 and the lanes at the iteration cap
  starts     rsba_problem_start_scene2 on that problem with the board unknown, without and with RSBA_START_BOTH_SOLUTIONS, launch by launch,
             and where rsba_solve ends from each
  small      a rig of small markers (5 cm at 1.2-2.4 m: 15-25 pixels), board given and board unknown: the blocks that start mirrored (more
             than 0.1 from the truth as rotation matrix) without and with the flag, and where rsba_solve ends from each start
  recorded   make_marker_chain(4, 8, 9, seed=3, keep=0.5) with nothing flagged, the mirrored-board failure recorded with the scene start

Kernel times are HIP-event intervals the library prints under RSBA_RUNPROF=1 (read back from stderr here), the minimum of the repetitions.

    python tools/marker_pose_both_scale.py [--out profiles/marker_pose_both_scale.jsonl] [--repeat 3] [--skip-large]
"""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from realsensecalibration_amd import capi, synthetic  # noqa: E402


def profiled(call, repeat):
    """-> (the last call's result, the library's stderr lines of `repeat` calls after one warm-up call)"""
    call()
    os.environ["RSBA_RUNPROF"] = "1"
    sys.stderr.flush()
    log, saved = tempfile.TemporaryFile(), os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        for _ in range(repeat):
            result = call()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        del os.environ["RSBA_RUNPROF"]
    log.seek(0)
    return result, log.read().decode()


def rotation_error(a, b):
    import marker_pose_ref as mp
    return np.array([np.abs(mp._rodrigues(x[:3]) - mp._rodrigues(y[:3])).max() for x, y in zip(a, b)])


def kernels(prob, repeat):
    dist = prob.get("dist")
    (poses, rms, status), text = profiled(lambda: capi.marker_poses_from_corners_both(prob["obs"], prob["c"], prob["intr"], dist, prob["marker_side"]), repeat)
    first = [float(x) for x in re.findall(r"k_marker_pose: \d+ detections, ([0-9.]+) ms", text)]
    second = [float(x) for x in re.findall(r"k_marker_pose_mirror: \d+ detections, ([0-9.]+) ms", text)]
    lower = (status[:, 1] <= 1) & (rms[:, 1] < rms[:, 0])
    return dict(line="kernels", detections=int(prob["N"]), k_marker_pose_event_ms=first, k_marker_pose_mirror_event_ms=second,
                k_marker_pose_event_ms_min=min(first), k_marker_pose_mirror_event_ms_min=min(second), ratio_of_minima=round(min(second) / min(first), 3),
                solution_0_status_counts=np.bincount(status[:, 0], minlength=3).tolist(), solution_1_status_counts=np.bincount(status[:, 1], minlength=4).tolist(),
                lanes_at_the_iteration_cap=[int((status[:, 0] == 1).sum()), int((status[:, 1] == 1).sum())], solution_1_of_lower_rms=int(lower.sum()))


def start(prob, board_known, both, sweeps, repeat=0):
    """One start and the solve after it -> dict; repeat > 0: with the launches' event times."""
    C, T, M = prob["C"], prob["T"], prob["M"]
    p = capi.Problem.marker_chain(prob)
    begin = p.params.copy()
    begin[:6 * (C + T)] = 0.0
    if board_known:
        begin[6 * (C + T):] = np.asarray(prob["truth"], float)[6 * (C + T):]
    else:
        begin[6 * (C + T + 1):] = 0.0

    def call():
        p.params[:] = begin
        return p.start_rig(None, sweeps, both_solutions=both) if board_known else p.start_scene(None, sweeps, both_solutions=both)

    out = dict(board="given" if board_known else "unknown", both_solutions=bool(both), shape=[C, T, M], detections=int(prob["N"]), refine_sweeps=sweeps)
    if repeat:
        result, text = profiled(call, repeat)
        name = "start_rig" if board_known else "start_scene"
        own = [float(x) for x in re.findall(name + r" k_marker_pose: \d+ detections, ([0-9.]+) ms", text)]
        mirror = [float(x) for x in re.findall(name + r" k_marker_pose_mirror: \d+ detections, ([0-9.]+) ms", text)]
        launches = re.findall(name + r" launch (\d+): (\w+) (\w+) (\d+), (\d+) blocks, (\d+) detections, ([0-9.]+) ms", text)
        per = len(launches) // repeat
        rows = [dict(launch=k, blocks_of=launches[k][1], kind=launches[k][2], blocks=int(launches[k][4]), detections=int(launches[k][5]),
                     event_ms_min=min(float(launches[r * per + k][6]) for r in range(repeat))) for k in range(per)]
        out.update(own_fit_event_ms_min=min(own), mirror_event_ms_min=min(mirror) if mirror else None, launches=rows,
                   kernels_event_ms_min_total=round(min(own) + (min(mirror) if mirror else 0.0) + sum(r["event_ms_min"] for r in rows), 4))
    else:
        result = call()
    status = result[-2]
    blocks, truth = p.params.reshape(-1, 6).copy(), np.asarray(prob["truth"], float).reshape(-1, 6)
    fitted = np.flatnonzero(status <= 1)
    err = rotation_error(blocks[fitted], truth[fitted])
    mirrored = fitted[err > 0.1]
    s = p.solve()
    out.update(missing=[int(v) for v in result[:-2]], status_counts=[int((status == k).sum()) for k in range(5)],
               blocks_more_than_0p1_from_the_truth=dict(cameras=int((mirrored < C).sum()), times=int(((mirrored >= C) & (mirrored < C + T)).sum()),
                                                        markers=int((mirrored >= C + T).sum())),
               solve_after=dict(termination=int(s.termination_type), iterations=int(s.num_iterations), final_cost=float(s.final_cost)))
    p.close()
    return out


def from_truth(prob):
    q = capi.Problem.marker_chain(dict(prob, params=np.asarray(prob["truth"], float).copy()))
    s = q.solve()
    q.close()
    return dict(termination=int(s.termination_type), iterations=int(s.num_iterations), final_cost=float(s.final_cost))


def ambiguous():
    import marker_pose_both_ref as mb
    import marker_pose_ref as mp
    corners, truth = mb.ambiguous_set()
    poses, rms, status = capi.marker_poses_from_corners_both(corners, None, mb.AMBIGUOUS_INTR.reshape(1, 4), None, mp.SIDE)
    have = status[:, 1] <= 1
    nearer = sum(1 for i in range(len(corners)) if have[i] and mp.pose_distance(poses[i, 1], truth[i]) < mp.pose_distance(poses[i, 0], truth[i]))
    return dict(line="ambiguous_set", detections=len(corners), with_a_second_solution=int(have.sum()), solution_1_nearer_the_truth=int(nearer),
                solution_1_of_lower_rms=int((have & (rms[:, 1] < rms[:, 0])).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    lines = [ambiguous()]
    if not a.skip_large:
        big = synthetic.make_marker_chain(8, 5000, 16, seed=11)
        lines.append(kernels(big, a.repeat))
        for both in (False, True):
            lines.append(dict(line="start_scene2_8x5000x16", **start(big, False, both, 1, a.repeat)))
        lines.append(dict(line="solve_from_the_truth_8x5000x16", **from_truth(big)))
    small = synthetic.make_marker_chain(4, 24, 9, seed=5, keep=0.7, marker_side=0.05)
    for known in (True, False):
        for both in (False, True):
            lines.append(dict(line="small_markers_4x24x9", marker_side=0.05, **start(small, known, both, 1)))
    lines.append(dict(line="solve_from_the_truth_small_markers_4x24x9", **from_truth(small)))
    rec = synthetic.make_marker_chain(4, 8, 9, seed=3, keep=0.5)
    for both in (False, True):
        lines.append(dict(line="recorded_failure_4x8x9_seed3_keep0p5", **start(rec, False, both, 1)))
    lines.append(dict(line="solve_from_the_truth_4x8x9_seed3_keep0p5", **from_truth(rec)))
    text = "\n".join(json.dumps(x) for x in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
