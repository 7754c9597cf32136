"""Marker-chain model at scale on the GPU: per-kernel times of the time-elimination path.

    python tools/marker_chain_scale.py [C T M [huber|cauchy a]] [const=SET] [schur_impl=K] [dump=PATH] [weights=FRAC] [dist=SEED] [subset=FRAC] [priors=SIGMA]
        default 8 5000 16, no loss; SET: markers | cameras:K (cameras 1..K) | times:K (every T/K-th time) | rig (every camera
        and marker: only the times are free), joined by '+' (e.g. cameras:2+times:100); dump=PATH writes the final parameters
        and the iteration log (.npz) of the last unprofiled run; weights=FRAC: observation weights on the problem (ceres::ScaledLoss),
        that fraction of the residual blocks (seeded) at weight 0 and the rest at 1 — 0 asks for all ones; dist=SEED: lens distortion,
        tests/marker_distortion_ref.py's coefficients(C, SEED) on the problem and its detections redetected through them;
        subset=FRAC: constant components (ceres::SubsetParameterization) — that fraction of the camera, time and marker blocks
        (seeded) each get a random mask of one to five components; priors=SIGMA: a Gaussian prior (ceres::NormalPrior) with
        A = diag(1 / SIGMA) around the start values on every free camera and marker block
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from realsensecalibration_amd import capi, synthetic  # noqa: E402

KW = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
ARGS = [a for a in sys.argv[1:] if "=" not in a]
C_, T_, M_ = (int(v) for v in ARGS[0:3]) if len(ARGS) >= 3 else (8, 5000, 16)
LOSS, LOSS_A = (ARGS[3], float(ARGS[4])) if len(ARGS) >= 5 else ("none", 0.0)


def constant_blocks(spec):
    out = set()
    for part in filter(None, spec.split("+")):
        kind, _, k = part.partition(":")
        if kind == "markers":
            out |= {C_ + T_ + m for m in range(1, M_)}
        elif kind == "cameras":
            out |= set(range(1, int(k) + 1))
        elif kind == "times":
            out |= {C_ + t for t in range(0, T_, max(1, T_ // int(k)))}
        elif kind == "rig":
            out |= set(range(1, C_)) | {C_ + T_ + m for m in range(1, M_)}
        else:
            raise SystemExit("unknown constant set %r" % part)
    return sorted(out)


CONST = constant_blocks(KW.get("const", ""))
LOSS_KW = {} if LOSS == "none" else {"huber_delta": LOSS_A, "loss_type": 1 if LOSS == "cauchy" else 0}
t0 = time.time()
prob = synthetic.make_marker_chain(C_, T_, M_, seed=11)
gen = time.time() - t0
DIST = int(KW["dist"]) if "dist" in KW else None
if DIST is not None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import marker_distortion_ref as dref  # noqa: E402
    prob = dref.redetect(prob, dref.coefficients(C_, DIST), 0.3, DIST)
p = capi.Problem.marker_chain(prob)
for b in CONST:
    p.set_parameter_block_constant(6 * b)
WEIGHTS = float(KW["weights"]) if "weights" in KW else None
if WEIGHTS is not None:
    p.set_observation_weights(np.where(np.random.default_rng(12).random(prob["N"]) < WEIGHTS, 0.0, 1.0))
SUBSET = float(KW["subset"]) if "subset" in KW else None
NSUB = 0
if SUBSET:
    rng = np.random.default_rng(13)
    for b in np.flatnonzero(rng.random(C_ + T_ + M_) < SUBSET):
        p.set_parameter_subset_constant(6 * int(b), int(rng.integers(1, 63)))
        NSUB += 1
NPRIOR = 0
if "priors" in KW:
    start = np.asarray(prob["params"], float).reshape(-1, 6)
    for b in [c for c in range(1, C_)] + [C_ + T_ + m for m in range(1, M_)]:
        if b not in CONST:
            p.set_block_prior(6 * b, np.eye(6) / float(KW["priors"]), start[b])
            NPRIOR += 1
out = {}
for mode in (0, 1):
    s = capi.Solver(p, capi.default_options(profile_kernels=mode, schur_impl=int(KW.get("schur_impl", 1)), **LOSS_KW))
    s.run()            # warm-up: code objects, allocations
    for _ in range(int(os.environ.get("MC_RUNS", "3")) - 1):   # (the kernel statistics include the warm-up's first launches: amortised)
        s.run()
    sm = s.run()
    if mode == 0:
        out["constant_blocks"] = len(CONST)
        out["zero_weight_fraction"] = WEIGHTS
        out["distortion_seed"] = DIST
        out["subset_blocks"] = NSUB
        out["prior_blocks"] = NPRIOR
        out["eliminates_times"] = s.eliminates_times()
        if "dump" in KW:
            s.download()
            np.savez(KW["dump"], params=p.params.copy(), iterations=s.iterations())
        out.update({"cameras": C_, "times": T_, "markers": M_, "residual_blocks": int(prob["N"]), "generate_s": round(gen, 2), "loss": LOSS, "loss_scale": LOSS_A,
                    "iterations": sm.num_iterations, "initial_cost": sm.initial_cost, "final_cost": sm.final_cost,
                    "minimizer_ms": 1e3 * sm.minimizer_seconds, "setup_seconds": sm.setup_seconds,
                    "ms_per_iteration": 1e3 * sm.minimizer_seconds / max(1, sm.num_iterations + 1)})
    else:
        out["kernels_us"] = {k: round(1e3 * ms / n, 1) for k, (n, ms) in s.kernel_stats().items()}
    s.download()
    s.close()
# roofline entry of the elimination of the time blocks: ALGORITHMIC work per LM iteration.  Per residual block (8 residuals, a camera,
# a time and a marker block of 6: J is 8 x 18) the normal-equation products J'J / J'r restricted to what the elimination needs —
# V += Jt'Jt (8 x 21 unique), g_t (8 x 6), W_c = Jt'Jc and W_m = Jt'Jm (8 x 36 each), U_cc, U_mm (8 x 21 each), U_cm (8 x 36),
# g_c, g_m (8 x 6 each): 1512 multiply-adds where all three blocks are parameters (camera 0 / marker 0 are not: those rows drop
# their terms); per time block with f touched camera / marker blocks the Schur update W'V^-1 W: (6f)^2/2 x 6 + the 6 x 6 solve.
# Bytes: a residual block's record (8 pixels + 3 indices: 76 B) once, every time block's parameters read and its step written (96 B).
t_arr, c_arr, m_arr = prob["t"], prob["c"], prob["m"]
fma = 0.0
for has_c, has_m in ((True, True), (True, False), (False, True), (False, False)):
    n = int(np.sum(((c_arr != 0) == has_c) & ((m_arr != 0) == has_m)))
    fma += n * 8 * (21 + 6 + (36 + 21 + 6 if has_c else 0) + (36 + 21 + 6 if has_m else 0) + (36 if has_c and has_m else 0))
key = t_arr.astype(np.int64) * 4096
fc = np.unique(key[c_arr != 0] + c_arr[c_arr != 0]); fm = np.unique(key[m_arr != 0] + 2048 + m_arr[m_arr != 0])
f_per_time = np.bincount((np.concatenate([fc, fm]) // 4096).astype(np.int64), minlength=T_).astype(float)
fma += float(np.sum((6 * f_per_time) ** 2 / 2 * 6 + 6 ** 3 / 3))
flops = 2.0 * fma
nbytes = 76.0 * prob["N"] + 96.0 * T_
# the elimination of the time blocks: round 6's split kernels (csrc/ba_marker_split.hpp; timed one after the other here — in a run
# that is not profiled the three product kernels share the chip on three streams), or round 4's k_time_eliminate (RSBA_MT_SPLIT=0)
SPLIT = ["k_mc_slot_products", "k_mc_time_products", "k_mc_cross", "k_mc_accumulate"]
ku = out.get("kernels_us", {})
parts = {k: ku[k] for k in SPLIT if k in ku} or ({"k_time_eliminate": ku["k_time_eliminate"]} if "k_time_eliminate" in ku else {})
if parts:
    us = sum(parts.values())
    # the split kernels form a residual block's Jacobian rows 2.7 times instead of once: NOT counted — algorithmic work only
    out["roofline"] = {"kernel": "+".join(parts), "kernels_us": parts, "avg_launch_us": round(us, 1), "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": nbytes,
                       "flops_per_residual_block": flops / prob["N"], "bytes_per_residual_block": nbytes / prob["N"],
                       "achieved_TFLOPs": flops / (us * 1e-6) / 1e12, "frac_of_fp64_peak_78.6": flops / (us * 1e-6) / 1e12 / 78.6,
                       "achieved_GBps": nbytes / (us * 1e-6) / 1e9, "frac_of_hbm_8000": nbytes / (us * 1e-6) / 1e9 / 8000.0,
                       "bound": ("fp64 VALU issue of threads that own their sums (one wavefront a SIMD at 334 registers), then two barriers a time in the accumulation" if len(parts) > 1 else
                                 "neither roof: a latency chain of five barriers per 32-block tile inside one workgroup per chunk of shots (HISTORY.md round 4)")}
err = np.abs(p.params - prob["truth"]).reshape(-1, 6)
out["max_abs_error_vs_truth"] = float(err.max())
print(json.dumps(out))
