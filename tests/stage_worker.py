"""Child process of tests/test_gpu_reduced_solve.py: runs the point model's first step through rsba_points_solve_stage with
whatever RSBA_* switches the environment carries (they are read once per process) and prints, as one JSON line per run, the path
that ran, how S and rhs compare with the oracle, and the backward error of the solve (tests/solve_accuracy.py).
Test infrastructure: the oracle and the host checker are the references.

Case names: c<C>_p<P>_k<views>_s<seed>[_h<huber>][_r<radius>][_i0][_const<a>-<b>...][_drop<cam>][_lm0][_whole]
  _i0       schur_impl = 0 (the atomic Schur kernel)
  _const    constant cameras
  _drop     every observation of that camera removed (a zero column in S but for the damping)
  _lm0      min_lm_diagonal = 0 (with _drop: exactly singular)
  _whole    also a whole solve (min_lm_diagonal as above), its termination, radii, parameters and stalls
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import oracle_lib  # noqa: E402
import solve_accuracy as sa  # noqa: E402
from realsensecalibration_amd import capi, synthetic as syn  # noqa: E402

NAME = re.compile(r"c(\d+)_p(\d+)_k(\d+)_s(\d+)(?:_h([\d.]+))?(?:_r([\de.+-]+))?(_i0)?(?:_const([\d-]+))?(?:_drop(\d+))?(_lm0)?(_whole)?$")


def parse(name):
    m = NAME.match(name)
    assert m, name
    C, P, k, seed = (int(m.group(i)) for i in range(1, 5))
    return dict(C=C, P=P, k=k, seed=seed, huber=float(m.group(5) or 0.0), radius=float(m.group(6) or 1e4), impl=0 if m.group(7) else 1,
                const=[int(c) for c in m.group(8).split("-")] if m.group(8) else [], drop=int(m.group(9)) if m.group(9) else None,
                lm0=bool(m.group(10)), whole=bool(m.group(11)))


def drop_camera(prob, cam):
    keep = prob["cam_idx"] != cam
    q = dict(prob)
    q["cam_idx"] = np.ascontiguousarray(prob["cam_idx"][keep])
    q["pt_idx"] = np.ascontiguousarray(prob["pt_idx"][keep])
    q["obs"] = np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1))
    q["N"] = int(keep.sum())
    return q


def stage(prob, opts, radius, const):
    if not const:
        return capi.points_solve_stage(prob, radius, opts)
    # (constant cameras: the problem handle carries them, so the stage entry is called on a handle of our own)
    import ctypes as C
    p = capi.Problem.points(prob)
    for c in const:
        p.set_camera_constant(c)
    nc, n = 6 * prob["C"], 6 * prob["C"] + 3 * prob["P"]
    S, rhs, dcam, scale_c, delta, scal = np.zeros((nc, nc)), np.zeros(nc), np.zeros(nc), np.zeros(nc), np.zeros(n), np.zeros(17)
    try:
        capi._chk(capi.load().rsba_points_solve_stage(p.h, C.byref(opts), radius, capi._vp(S), capi._vp(rhs), capi._vp(dcam), capi._vp(scale_c),
                                                      capi._vp(delta), capi._vp(scal)), "rsba_points_solve_stage")
    finally:
        p.close()
    return dict(S=S, rhs=rhs, dcam=dcam, scale_c=scale_c, delta=delta, solve_ok=bool(scal[3]),
                path=dict(schedule="pipelined" if scal[8] else "sequential", factorisation=capi.STAGE_FACTORISATIONS[int(scal[9])],
                          workgroups=int(scal[10]), border_cols=int(scal[11]), tiles=int(scal[12]), backsub=capi.STAGE_BACKSUBS[int(scal[13])],
                          sys_fused=bool(scal[14]), stalls=int(scal[15]), fallbacks=int(scal[16])))


def run_case(oracle, name):
    c = parse(name)
    C, radius = c["C"], c["radius"]
    prob = syn.make_problem(C, c["P"], c["k"], seed=c["seed"], outlier_frac=0.05 if c["huber"] else 0.0)
    if c["drop"] is not None:
        prob = drop_camera(prob, c["drop"])
    kw = dict(schur_impl=c["impl"], huber_delta=c["huber"])
    if c["lm0"]:
        kw["min_lm_diagonal"] = 0.0
    opts = capi.default_options(**kw)
    got = stage(prob, opts, radius, c["const"])
    again = stage(prob, capi.default_options(**kw), radius, c["const"])
    free = np.ones(C, bool)
    free[c["const"]] = False
    rows = sa.free_rows(C, free)
    out = dict(name=name, path=got["path"], path_again=again["path"], solve_ok=got["solve_ok"],
               finite=bool(np.isfinite(got["dcam"]).all() and np.isfinite(got["S"]).all() and np.isfinite(got["rhs"]).all()),
               reproducible=bool(np.array_equal(got["dcam"], again["dcam"])),
               S_sym=float(np.abs(got["S"] - got["S"].T).max()))
    # S and rhs against the oracle (free cameras; a constant camera's rows are zero but for the LM floor on the diagonal)
    ref = oracle.points_linearize_and_step(prob, prob["params"], radius, oracle.options(**{k: v for k, v in kw.items() if k != "schur_impl"}))
    Sf, Sr = got["S"][np.ix_(rows, rows)], ref["S"][np.ix_(rows, rows)]
    out["S_err"] = float(np.abs(Sf - Sr).max() / np.abs(Sr).max())
    out["rhs_err"] = float(np.abs(got["rhs"][rows] - ref["rhs"][rows]).max() / np.abs(ref["rhs"][rows]).max())
    if c["const"]:
        crow = np.setdiff1d(np.arange(6 * C), rows)
        floor = np.diag(np.full(crow.size, opts.min_lm_diagonal / radius))
        out["const_rows_exact"] = bool(np.array_equal(got["S"][crow][:, crow], floor) and not got["S"][crow][:, rows].any()
                                       and not got["rhs"][crow].any())
        out["const_dcam_zero"] = bool(np.all(got["dcam"][crow] == 0.0))
    if c["drop"] is not None:
        out["drop_dcam_zero"] = bool(np.all(got["dcam"][6 * c["drop"]:6 * c["drop"] + 6] == 0.0))
    if got["solve_ok"]:
        y = -got["dcam"] / got["scale_c"]
        eta, bar, kappa = sa.check(got["S"], got["rhs"], y, rows)
        out.update(eta=eta, bar=bar, kappa=kappa)
    if c["whole"]:
        p = capi.Problem.points(prob)
        for cc in c["const"]:
            p.set_camera_constant(cc)
        sv = capi.Solver(p, capi.default_options(**kw))
        try:
            s = sv.run()
            sv.download()
            log = sv.iterations()
            info = sv.schedule_info()
        finally:
            sv.close()
        out["whole"] = dict(termination=int(s.termination_type), stop=int(s.stop_reason), iterations=int(s.num_iterations),
                            unsuccessful=int(s.num_unsuccessful_steps), radii=[float(r) for r in log[1:, 6]],
                            params_unchanged=bool(np.array_equal(p.params, prob["params"])), stalls=info["stalls"], fallbacks=info["fallbacks"])
        p.close()
    return out


def main():
    oracle = oracle_lib.load()
    for name in sys.argv[1:]:
        print(json.dumps(run_case(oracle, name)), flush=True)


if __name__ == "__main__":
    main()
