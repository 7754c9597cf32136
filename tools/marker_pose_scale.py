"""Single-marker pose fits at the scale the project measures: the detections of the 8 x 5000 x 16 synthetic marker-chain problem
(synthetic.make_marker_chain(8, 5000, 16, seed=11), as tools/marker_chain_scale.py) through rsba_marker_poses_from_corners on the GPU and
through a single-thread host loop of rsba_marker_pose_from_corners.  Recorded, no bar: profiles/marker_pose_scale.jsonl.

The GPU figures are taken after one warm-up call: HIP events around the kernel launch (the library records them under RSBA_RUNPROF=1 and
prints the interval to stderr, which is read back here), and HIP events on the null stream around the whole call — the entry owns its
buffers, so that interval also holds the allocation and the copies of 64 B in and 60 B out per detection.  The host loop is timed through
ctypes on the first --host-sample detections and scaled (the Python call overhead is measured on a refused call and subtracted).

    python tools/marker_pose_scale.py [--out profiles/marker_pose_scale.jsonl] [--repeat 5] [--host-sample 20000]
"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=20000)
    a = ap.parse_args()
    import torch
    prob = synthetic.make_marker_chain(8, 5000, 16, seed=11)
    corners, cam, intr, side = np.ascontiguousarray(prob["obs"]), prob["c"], prob["intr"], prob["marker_side"]
    n = len(corners)
    poses, rms, status = capi.marker_poses_from_corners(corners, cam, intr, None, side)      # warm-up
    ms, wall = [], []
    os.environ["RSBA_RUNPROF"] = "1"
    sys.stderr.flush()
    log, saved = tempfile.TemporaryFile(), os.dup(2)
    os.dup2(log.fileno(), 2)        # the library's stderr lines of the timed calls
    for _ in range(a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        capi.marker_poses_from_corners(corners, cam, intr, None, side)
        e1.record()
        e1.synchronize()
        wall.append(round(1e3 * (time.perf_counter() - t0), 3))
        ms.append(round(e0.elapsed_time(e1), 3))
    os.dup2(saved, 2)
    os.close(saved)
    del os.environ["RSBA_RUNPROF"]
    log.seek(0)
    launch = [round(float(x), 4) for x in re.findall(r"k_marker_pose: \d+ detections, ([0-9.]+) ms", log.read().decode())]
    assert len(launch) == a.repeat, launch
    lines = [dict(line="gpu_batch", detections=n, launch_event_ms_repetitions=launch, launch_event_ms_min=min(launch), status_counts=[int((status == k).sum()) for k in range(3)], rms_median_px=round(float(np.median(rms[status < 2])), 4),
                  call_event_ms_repetitions=ms, call_event_ms_min=min(ms), call_wall_ms_repetitions=wall,
                  note="launch: HIP events around the one launch of k_marker_pose; call: around the entry, with its allocation and copies in and out")]
    lib, m = capi.load(), min(a.host_sample, n)
    out, e, st = np.zeros(6), C.c_double(), C.c_int32()
    t0 = time.perf_counter()
    for i in range(m):
        lib.rsba_marker_pose_from_corners(None, None, None, C.c_double(side), None, None, None)
    overhead = time.perf_counter() - t0
    host = np.zeros((m, 6))
    t0 = time.perf_counter()
    for i in range(m):
        lib.rsba_marker_pose_from_corners(corners[i].ctypes.data, intr[cam[i]].ctypes.data, None, C.c_double(side), out.ctypes.data, C.byref(e), C.byref(st))
        host[i] = out
    loop = time.perf_counter() - t0
    per = max(loop - overhead, 0.0) / m
    diff = float(np.abs(host - poses[:m])[status[:m] < 2].max())
    lines.append(dict(line="host_single_thread", detections_timed=m, us_per_detection=round(1e6 * per, 3), ms_scaled_to_all=round(1e3 * per * n, 1),
                      loop_seconds=round(loop, 3), call_overhead_seconds=round(overhead, 3), largest_difference_to_gpu=diff,
                      note="ctypes loop over rsba_marker_pose_from_corners, call overhead of a refused call subtracted (array indexing of the loop is not)"))
    text = "\n".join(json.dumps(x) for x in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
