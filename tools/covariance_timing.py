"""Time rsba_solver_covariance_compute with HIP events (torch.cuda.Event on the solver's stream).

  python tools/covariance_timing.py [--reps 3]

Shapes: cfg3 (64 cameras x 100k points x 2M observations, camera 0 and point 0 constant) and one rank's shard of cfg5 (256 cameras,
the first 62 500 of its 500k points, Huber 1.0, camera 0 and point 0 constant).  The covariance is taken at the uploaded start (no
solve first); one untimed call precedes the timed ones.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from realsensecalibration_amd import capi, synthetic  # noqa: E402


def time_shape(name, prob, reps):
    pr = capi.Problem.points(prob)
    pr.set_camera_constant(0)
    pr.set_point_constant(0)
    stream = torch.cuda.Stream()
    o = capi.default_options(huber_delta=prob.get("huber_delta", 0.0), stream=stream.cuda_stream)
    s = capi.Solver(pr, o)
    s.covariance_compute()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        s.covariance_compute()   # (synchronous: it returns after the result flag has been read back)
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    s.close()
    return {"shape": name, "C": prob["C"], "P": prob["P"], "N": prob["N"], "covariance_ms": ms, "min_ms": min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    capi.load()
    print(json.dumps(time_shape("cfg3", synthetic.make_config("cfg3"), a.reps)), flush=True)
    print(json.dumps(time_shape("cfg5_shard", synthetic.make_config("cfg5", point_range=(0, 62_500)), a.reps)), flush=True)


if __name__ == "__main__":
    main()
