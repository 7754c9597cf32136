"""The cost of staying on the dense path with free intrinsics (rsba_problem_set_intrinsics_free): per-iteration time of the dense
marker-chain solve on one rig with and without them, and of the time-eliminating path such a solver gives up (DESIGN §8,
profiles/marker_intrinsics_scale.jsonl), and of the eliminating path with free intrinsics (schur_impl = 3,
profiles/marker_intrinsics_elim_scale.jsonl).

    python tools/marker_intrinsics_scale.py [reps=3] [shape=4,200,16] [mask=0x3f] [dense=1] [out=PATH]

Four configurations of one problem (synthetic.make_marker_chain(shape, seed=11), intrinsics displaced as the tests displace them), in
one process, the repetitions alternating between them:
    dense, intrinsics fixed    schur_impl 0: the parent's kernels
    dense, intrinsics free     `mask` on every camera: the k_marker_intr_* kernels, 6 more columns per camera
    eliminating, fixed         schur_impl 2: what a solver without free intrinsics may take instead
    eliminating, free          schur_impl 3 with `mask`: the time blocks eliminated, the intrinsics blocks in the reduced system
dense=0 skips the two dense configurations (a shape whose dense system is refused with free intrinsics, or too large without).
Per repetition a fresh solver: one warm-up run, then one run timed by the host clock (rsba_summary's minimizer_seconds: every step ends
in a stream synchronise) and one profiled run (profile_kernels = 1: the solver's own HIP event pairs around every kernel).  One line
per configuration: ms_per_iteration = minimizer time / (iterations + 1), kernel_ms_per_step = the events' total over the steps
launched; of both the minimum over the repetitions, and every repetition's value.  Recorded, no bar.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import marker_intrinsics_ref as iref  # noqa: E402
from realsensecalibration_amd import capi, synthetic  # noqa: E402

KW = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
REPS = int(KW.get("reps", 3))
C_, T_, M_ = (int(v) for v in KW.get("shape", "4,200,16").split(","))
MASK = int(KW.get("mask", "0x3f"), 0)
CONFIGS = [("dense, intrinsics fixed", 0, 0), ("dense, intrinsics free (mask 0x%02x on every camera)" % MASK, 0, MASK), ("eliminating, intrinsics fixed", 2, 0),
           ("eliminating, intrinsics free (mask 0x%02x on every camera)" % MASK, 3, MASK)]
if int(KW.get("dense", 1)) == 0:
    CONFIGS = [c for c in CONFIGS if c[1] != 0]

base = synthetic.make_marker_chain(C_, T_, M_, seed=11)
prob = dict(base, intr=iref.displaced_intrinsics(base["intr"]))


def one(schur_impl, mask):
    p = capi.Problem.marker_chain(prob)
    try:
        for k in range(C_ if mask else 0):
            p.set_intrinsics_free(k, mask)
        out = {}
        for mode in (0, 1):
            s = capi.Solver(p, capi.default_options(profile_kernels=mode, schur_impl=schur_impl))
            try:
                s.run()
                if mode == 1:
                    s.configure_run(50, 1)   # (drops the warm-up's statistics)
                sm = s.run()
                if mode == 0:
                    out.update(eliminates_times=s.eliminates_times(), iterations=sm.num_iterations, final_cost=sm.final_cost,
                               ms_per_iteration=1e3 * sm.minimizer_seconds / (sm.num_iterations + 1))
                else:
                    st = s.kernel_stats(64)
                    steps = max(n for k, (n, _) in st.items() if k in ("k_marker_system", "k_marker_intr_system", "k_marker_reduce"))
                    out.update(kernel_ms_per_step=sum(ms for _, ms in st.values()) / steps,
                               kernels_us={k: round(1e3 * ms / n, 1) for k, (n, ms) in st.items()})
            finally:
                s.close()
        return out
    finally:
        p.close()


results = {name: [] for name, _, _ in CONFIGS}
for rep in range(REPS):
    for name, impl, mask in (CONFIGS if rep % 2 == 0 else CONFIGS[::-1]):
        results[name].append(one(impl, mask))
        print("repetition %d  %-60s %.3f ms per iteration" % (rep + 1, name, results[name][-1]["ms_per_iteration"]), file=sys.stderr)
lines = []
for name, impl, mask in CONFIGS:
    r = results[name]
    ms, kms = [round(v["ms_per_iteration"], 4) for v in r], [round(v["kernel_ms_per_step"], 4) for v in r]
    used = np.unique(prob["t"]).size + (C_ - 1) + (M_ - 1)
    lines.append(json.dumps({"line": name, "cameras": C_, "times": T_, "markers": M_, "residual_blocks": int(prob["N"]),
                             "columns": 6 * used + (6 * C_ if mask else 0), "schur_impl": impl, "eliminates_times": r[0]["eliminates_times"],
                             "ms_per_iteration_min": min(ms), "ms_per_iteration_repetitions": ms,
                             "kernel_ms_per_step_min": min(kms), "kernel_ms_per_step_repetitions": kms,
                             "iterations": r[0]["iterations"], "final_cost": r[0]["final_cost"], "kernels_us": r[0]["kernels_us"]}))
text = "\n".join(lines) + "\n"
if "out" in KW:
    open(KW["out"], "w").write(text)
sys.stdout.write(text)
