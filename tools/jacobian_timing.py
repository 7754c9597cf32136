"""Time rsba_solver_evaluate_jacobian with HIP events (torch.cuda.Event on the solver's stream).

  python tools/jacobian_timing.py [--reps 5]

Shapes: cfg3 (64 cameras x 100k points x 2M observations, camera 0 and point 0 constant) and one rank's shard of cfg5 (256 cameras,
the first 62 500 of its 500k points, Huber 1.0, camera 0 and point 0 constant), at the uploaded start; one untimed call precedes the
timed ones.  A call is [pose constants | the Jacobian kernel | the device-to-host copy of the values] on one stream, and the entry
point has no device-pointer output, so the two parts are told apart like this:
  call_ms     events around the whole call (kernels + copy into pageable host memory; the call returns after the copy)
  copy_ms     events around a copy of as many bytes from a device buffer into pageable host memory, on the same stream
  kernel      the kernels' own time is the kernel trace's: run this script under `rocprofv3 --kernel-trace --stats -- python ...`
              in a run of its own and read k_eval_jacobian_points there.  call_ms - copy_ms is NOT it: Solver.evaluate_jacobian
              allocates its result for every call, so the call's copy also pays the first touch of those pages
and the kernel is a pure store stream, so it is set against bytes_written / 6.3 TB/s (the streaming rate the part reaches).
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from realsensecalibration_amd import capi, synthetic  # noqa: E402

STREAM_TBS = 6.3


def _timed(stream, fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def time_shape(name, prob, reps):
    pr = capi.Problem.points(prob)
    pr.set_camera_constant(0)
    pr.set_point_constant(0)
    stream = torch.cuda.Stream()
    o = capi.default_options(huber_delta=prob.get("huber_delta", 0.0), stream=stream.cuda_stream)
    s = capi.Solver(pr, o)
    (rows, cols), indptr, _ = s.jacobian_structure()
    nnz = int(indptr[-1])
    s.evaluate_jacobian()
    call = _timed(stream, s.evaluate_jacobian, reps)   # (synchronous: it returns after the values have been copied back)
    dev = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    host = torch.from_numpy(np.zeros(nnz))   # pageable, as the caller's array is

    def copy():
        with torch.cuda.stream(stream):
            host.copy_(dev)
    copy()
    cp = _timed(stream, copy, reps)
    s.close()
    pr.close()
    floor_ms = 8.0 * nnz / (STREAM_TBS * 1e12) * 1e3
    return {"shape": name, "C": prob["C"], "P": prob["P"], "N": prob["N"], "rows": rows, "cols": cols, "nnz": nnz, "bytes_written": 8 * nnz,
            "call_ms": call, "copy_ms": cp, "min_call_ms": min(call), "min_copy_ms": min(cp),
            "bytes_over_%.1f_TBs_ms" % STREAM_TBS: floor_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    capi.load()
    print(json.dumps(time_shape("cfg3", synthetic.make_config("cfg3"), a.reps)), flush=True)
    print(json.dumps(time_shape("cfg5_shard", synthetic.make_config("cfg5", point_range=(0, 62_500)), a.reps)), flush=True)


if __name__ == "__main__":
    main()
