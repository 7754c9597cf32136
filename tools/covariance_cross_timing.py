"""Time the general covariance queries (rsba_solver_covariance_blocks, rsba_solver_time_covariances) with HIP events
(torch.cuda.Event on the solver's stream), each beside rsba_solver_covariance_compute of the same solver.

  python tools/covariance_cross_timing.py [--reps 5]

  marker chain 8 x 5000 x 16, time-eliminating path:  time_covariances() (formed once per compute: every repetition computes first,
                                                      the compute timed on its own) and 10 000 (time, marker) pairs
  point model cfg3 (camera 0 and point 0 constant):   10 000 (camera, point) pairs

The covariance is taken at the uploaded start (no solve first).  One untimed round precedes the timed ones.  The calls are
synchronous (they return after the blocks have been read back), so an event pair around a call spans its uploads, kernels and the
copy back.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from realsensecalibration_amd import capi, synthetic  # noqa: E402


def timed(stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def marker_chain(reps):
    prob = synthetic.make_marker_chain(8, 5000, 16, seed=1)
    pr = capi.Problem.marker_chain(prob)
    stream = torch.cuda.Stream()
    s = capi.Solver(pr, capi.default_options(schur_impl=2, stream=stream.cuda_stream))
    assert s.eliminates_times() == 1
    rng = np.random.default_rng(3)
    pairs = [(s.time_offset(int(t)), s.marker_offset(int(m))) for t, m in zip(rng.integers(0, 5000, 10_000), rng.integers(1, 16, 10_000))]
    out = {"shape": "marker_chain_8x5000x16", "N": prob["N"], "compute_ms": [], "time_covariances_ms": [], "blocks_10000_time_marker_ms": []}
    for r in range(reps + 1):
        ms = (timed(stream, s.covariance_compute), timed(stream, s.time_covariances), timed(stream, lambda: s.covariance_blocks(pairs)))
        if r > 0:   # (round 0: warm-up)
            for k, v in zip(("compute_ms", "time_covariances_ms", "blocks_10000_time_marker_ms"), ms):
                out[k].append(v)
    s.close()
    pr.close()
    return out


def points(reps):
    prob = synthetic.make_config("cfg3")
    pr = capi.Problem.points(prob)
    pr.set_camera_constant(0)
    pr.set_point_constant(0)
    stream = torch.cuda.Stream()
    s = capi.Solver(pr, capi.default_options(huber_delta=prob.get("huber_delta", 0.0), stream=stream.cuda_stream))
    rng = np.random.default_rng(4)
    pairs = [(s.camera_offset(int(c)), s.point_offset(int(j))) for c, j in zip(rng.integers(1, prob["C"], 10_000), rng.integers(1, prob["P"], 10_000))]
    out = {"shape": "cfg3", "C": prob["C"], "P": prob["P"], "N": prob["N"], "compute_ms": [], "blocks_10000_camera_point_ms": []}
    for r in range(reps + 1):
        ms = (timed(stream, s.covariance_compute), timed(stream, lambda: s.covariance_blocks(pairs)))
        if r > 0:
            out["compute_ms"].append(ms[0])
            out["blocks_10000_camera_point_ms"].append(ms[1])
    s.close()
    pr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    capi.load()
    for fn in (marker_chain, points):
        res = fn(a.reps)
        res.update({k.replace("_ms", "_min_ms"): min(v) for k, v in res.items() if k.endswith("_ms")})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
