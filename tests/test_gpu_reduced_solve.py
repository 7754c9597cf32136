"""Every factorisation of the point model's reduced camera system, checked as a linear solve.

Whole LM solves hide an inexact step (Levenberg-Marquardt corrects it), so each production path — the schedule, factorisation
and back-substitution rsba_solver_run picks for a camera count and the RSBA_* switches — is run here for one step through
rsba_points_solve_stage and held to:
  (a) the path it ran is the path the case names (the step's own path scalars), with no stall or fallback;
  (b) S and rhs equal the oracle's at the stage bars (1e-11 of max |S|, max |rhs|), S symmetric to the bit;
  (c) the solve's componentwise backward error within the bar any correct fp64 factorisation meets (tests/solve_accuracy.py);
  (d) a second call gives the same dcam, bit for bit.
Singular systems (a camera without observations, min_lm_diagonal = 0) must be reported as failed solves on every factorisation
kind, and a whole solve must end like test_invalid_steps_end_in_failure; with the default LM floor the same camera gets a zero
step.  The switches are read once per process: one child process per setting (tests/stage_worker.py)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from step_path_ref import expected_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def name(C, P=None, k=8, h=0.0, r=1e4, impl=1, const=(), drop=None, lm0=False, whole=False):
    P = P or (600 if C <= 64 else 1500)
    s = "c%d_p%d_k%d_s%d" % (C, P, k, 500 + C)
    if h:
        s += "_h%g" % h
    if r != 1e4:
        s += "_r%g" % r
    if not impl:
        s += "_i0"
    if const:
        s += "_const" + "-".join(str(c) for c in const)
    if drop is not None:
        s += "_drop%d" % drop
    if lm0:
        s += "_lm0"
    if whole:
        s += "_whole"
    return s


def rows(Cs, impls=(1,), star=()):
    """Huber 0 and 1.0 at radius 1e4; the cameras counts in `star` also at radius 2.5 and 1e12."""
    out = []
    for C in Cs:
        for impl in impls:
            for h in (0.0, 1.0):
                out.append(name(C, h=h, impl=impl))
                if C in star:
                    out += [name(C, h=h, impl=impl, r=2.5), name(C, h=h, impl=impl, r=1e12)]
    return out


def singular(C, cams, whole=True):
    """A camera without observations: exactly singular (min_lm_diagonal = 0, plus a whole solve) and at the default LM floor."""
    return [x for cam in cams for x in (name(C, drop=cam, lm0=True, whole=whole), name(C, drop=cam))]


SETTINGS = [
    # (the defaults in four children: one-workgroup and diagonal-chain paths, the tiled paths, the atomic Schur kernel and constant
    #  cameras, singular systems)
    ({}, rows([1, 2, 5, 16], impls=(1, 0)) + rows([17, 31, 32, 33, 37, 47, 48, 63, 64], star=(64,))),
    ({}, rows([65, 96, 97, 100, 128, 129, 240, 256], star=(256,))),
    ({}, rows([40, 70], impls=(0,)) + [name(40, const=(0, 35, 39)), name(40, h=1.0, const=(0, 35, 39)), name(70, const=(0, 40, 69)),
                                      name(70, h=1.0, const=(0, 40, 69))]),
    ({}, singular(20, (0, 19)) + singular(32, (0, 31)) + singular(37, (0, 34, 36)) + singular(65, (0, 64))),
    ({"RSBA_CHOL_WGS": "1"}, rows([40, 64])),
    ({"RSBA_BORDER": "0"}, rows([40, 64]) + singular(40, (0, 39))),
    ({"RSBA_CHOL_WGS": "2"}, rows([37, 64])),
    ({"RSBA_CHOL_WGS": "3"}, rows([37, 64])),
    ({"RSBA_CHOL_WGS": "6"}, rows([37, 64])),
    ({"RSBA_CHOL_WGS": "8"}, rows([37, 64])),
    ({"RSBA_PIPELINE": "0"}, rows([40, 64]) + singular(37, (0, 36))),
    ({"RSBA_TILES_SMALL": "1", "RSBA_PIPELINE": "0"}, rows([33, 64]) + singular(37, (0, 36))),
    ({"RSBA_SYS_FUSED": "0"}, rows([65, 130])),
    ({"RSBA_CHOL_TILES": "0"}, rows([65, 130]) + singular(65, (0, 64))),
    ({"RSBA_BACKSUB_MULTI": "0"}, rows([65, 130])),
    ({"RSBA_BACKSUB_MULTI": "1"}, rows([65, 130])),
    ({"RSBA_TILE_ORDER": "0"}, rows([65, 130])),
    # Schur-kernel switches: S and rhs at one size each
    ({"RSBA_SPARSE_PAIRS": "0"}, rows([130])),
    ({"RSBA_SEG_PER_CU": "1"}, rows([64])),
    ({"RSBA_SEG_PER_CU": "4"}, rows([130])),
    ({"RSBA_BALANCE": "0"}, rows([64])),
]


def _run(env, cases):
    child_env = dict(os.environ)
    child_env.update(env)
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stage_worker.py")] + cases, env=child_env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("{"):
            r = json.loads(ln)
            res[r["name"]] = r
    return res, out.stderr, time.time() - t0


def _id(i):
    env, cases = SETTINGS[i]
    return (" ".join("%s=%s" % kv for kv in env.items()) or "defaults") + " " + cases[0]


@pytest.mark.parametrize("env,cases", SETTINGS, ids=[_id(i) for i in range(len(SETTINGS))])
def test_reduced_solve_within_its_backward_error_bar(env, cases):
    import stage_worker
    res, err, secs = _run(env, cases)
    print("\n[%s] %d cases in %.1f s" % (" ".join("%s=%s" % kv for kv in env.items()) or "defaults", len(cases), secs))
    assert "stalled" not in err, err[-3000:]
    failures = []
    for nm in cases:
        r = res[nm]
        c = stage_worker.parse(nm)
        want = expected_path(env, c["C"], c["impl"])
        got = {k: r["path"][k] for k in want}
        print("  %-44s eta %.2e  kappa %8.2f  bar %.2e  S %.1e rhs %.1e  %s" % (nm, r.get("eta", float("nan")), r.get("kappa", float("nan")),
                                                                            r.get("bar", float("nan")), r["S_err"], r["rhs_err"],
                                                                            " ".join("%s=%s" % kv for kv in r["path"].items())))
        checks = [
            ("path", got == want, (got, want)),
            ("path of the second call", {k: r["path_again"][k] for k in want} == want, r["path_again"]),
            ("stalls / fallbacks", r["path"]["stalls"] == 0 and r["path"]["fallbacks"] == 0, r["path"]),
        ]
        # (one camera: every point has one view, so its 3 x 3 block has a null direction (depth) held only by the LM damping and
        #  S = U - W V^-1 W' cancels: both sides' roundings grow by kappa(V_j) ~ radius, measured 5e-10 of max |S| — the stage bars
        #  are for points with two views or more; (a), (c) and (d) still hold)
        if c["C"] > 1:
            checks += [("S vs oracle", r["S_err"] < 1e-11, r["S_err"]), ("rhs vs oracle", r["rhs_err"] < 1e-11, r["rhs_err"])]
        checks += [
            ("S symmetric", r["S_sym"] == 0.0, r["S_sym"]),
            ("S, rhs finite", r["finite"] or (c["lm0"] and not r["solve_ok"]), r["finite"]),
        ]
        if c["lm0"] and c["drop"] is not None:
            checks.append(("singular system reported", not r["solve_ok"], r["solve_ok"]))
        else:
            checks += [("solve ok", r["solve_ok"], r["solve_ok"]),
                       ("backward error", r.get("eta", np.inf) <= r.get("bar", 0.0), (r.get("eta"), r.get("bar"), r.get("kappa"))),
                       # (schur_impl 0 adds into S with atomics: its order, and so its last bits, differ from call to call)
                       ("reproducible", r["reproducible"] or c["impl"] == 0, None)]
        if c["const"]:
            checks += [("constant rows", r["const_rows_exact"], None), ("constant cameras' dcam == 0", r["const_dcam_zero"], None)]
        if c["drop"] is not None and not c["lm0"]:
            checks.append(("camera without observations: dcam == 0", r["drop_dcam_zero"], None))
        if c["whole"]:
            w = r["whole"]
            checks += [("whole solve ends in FAILURE after 5 invalid steps", (w["termination"], w["stop"], w["iterations"], w["unsuccessful"]) == (2, 6, 5, 5), w),
                       ("radii", np.allclose(w["radii"][:4], [5e3, 1250.0, 156.25, 9.765625]), w["radii"]),
                       ("parameters unchanged", w["params_unchanged"], None),
                       ("no stall in the whole solve", w["stalls"] == 0, w)]
        failures += ["%s: %s %s" % (nm, what, detail) for what, ok, detail in checks if not ok]
    assert not failures, "\n".join(failures)
