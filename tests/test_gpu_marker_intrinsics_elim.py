"""Free intrinsics on the marker chain's TIME-ELIMINATING path (schur_impl = 3: the intrinsics blocks join the reduced system), through
the C ABI, against tests/marker_intrinsics_ref.py — the numpy reference the dense path is held to.  The Schur complement is exact
algebra, so the bars are the dense test's, test_gpu_marker_intrinsics._compare: the same valid / successful sequence, iteration
count, termination and reason; every iterate's cost to 1e-9 relative; pose and intrinsics blocks to 1e-6 absolute and relative; RMS
to 1e-4 px; what is not solved for keeps its bits.

One LM step: marker_step_accuracy's componentwise backward-error bar, unmodified, on marker_subset_ref.SubsetSystem with
dense = False (the eliminating form: the intrinsics columns are in the reduced set).

Measured on an MI355X (eta / bar of test 3): see DESIGN §4 "Free intrinsics".
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import marker_intrinsics_ref as iref
import marker_loss_ref as ref
import marker_subset_ref as sref
import test_gpu_marker_intrinsics as dense
from realsensecalibration_amd import capi, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_KERNELS = {"k_mc_intr_state", "k_mc_intr_slot_products", "k_mc_intr_marker_cross", "k_mc_intr_cross_sum"}
EXTRA = {   # name -> (C, T, M, masks, constant blocks)
    "3x12x4_const1": (3, 12, 4, [0x0F, 0x3F, 0x33], (1,)),
    "4x10x24_3f": (4, 10, 24, [0x3F] * 4, ()),
    "6x8x40_mixed6": (6, 8, 40, [0x0F, 0, 0x33, 0x3F, 0x03, 0x30], ()),
}
EXTRA_FACTS = {"3x12x4_const1": (42, 15), "4x10x24_3f": (180, 6), "6x8x40_mixed6": (294, 5)}   # reduced columns, iterations of the reference
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _extra_case(name):
    C, T, M, masks, const = EXTRA[name]
    prob, truth_six, truth = iref.rig(C, T, M, masks)
    return dict(prob=prob, dist=prob["dist"], masks=list(masks), variant=0, loss="none", a=0.0, weights=None, constant_blocks=const,
                pose_masks={}, priors={}, truth_six=truth_six, truth=truth)


def _run(name, **kw):
    """(case, chain, x, summary, rows) of the reference, once per process."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _RUNS:
        if name in EXTRA:
            cs = _extra_case(name)
        else:
            cs = iref.case(name)
        if not kw and name not in EXTRA:
            _RUNS[key] = iref.reference_run(name)
        else:
            mc = iref.chain_of(cs)
            _RUNS[key] = (cs, mc) + tuple(ref.minimise(mc, **kw))
    return _RUNS[key]


def _assert_eliminating(out):
    assert out["elim"] == 1
    names = set(out["stats"])
    assert NEW_KERNELS <= names and any(k.startswith("k_mc_accumulate") for k in names), sorted(names)
    assert "k_marker_intr_system" not in names and "k_marker_system" not in names, sorted(names)


def _reduced_columns(mc):
    return 6 * int(sum(1 for b in mc.free_blocks if b < mc.C or b >= mc.C + mc.T)) + 6 * len(mc.cams)


# ------------------------------------------------------------------------------------------------ 1. whole solves
@pytest.mark.parametrize("name", list(iref.SOLVE_CASES) + list(EXTRA))
def test_solve_matches_the_reference(name):
    run = _run(name)
    if name in EXTRA:
        nred, its = EXTRA_FACTS[name]
        assert _reduced_columns(run[1]) == nred and len(run[4]) - 1 == its, (_reduced_columns(run[1]), len(run[4]) - 1)
    out = dense._solve(run[0], 3, profile=True)
    _assert_eliminating(out)
    dense._compare(name, out, run)


# ------------------------------------------------------------------------------------------------ 2. a rejected step in the middle
def test_a_rejected_step_in_the_middle():
    run = _run("3x12x4_3f", min_relative_decrease=0.5)
    cs, rows = run[0], run[4]
    assert [rw["valid"] + 2 * rw["successful"] for rw in rows] == [0, 3, 3, 3, 1, 3, 3, 3, 3, 3, 1]
    out = dense._solve(cs, 3, profile=True, min_relative_decrease=0.5)
    _assert_eliminating(out)
    dense._compare("3x12x4_3f rejected", out, run)
    # a run that ends on the rejection returns what the run before it ended at
    four = dense._solve(cs, 3, max_num_iterations=4, min_relative_decrease=0.5)
    three = dense._solve(cs, 3, max_num_iterations=3, min_relative_decrease=0.5)
    assert int(four["log"][4, 7]) == 1 and four["elim"] == 1 and three["elim"] == 1
    assert four["params"].tobytes() == three["params"].tobytes()
    assert four["intr"].tobytes() == three["intr"].tobytes() and four["dist"].tobytes() == three["dist"].tobytes()


# ------------------------------------------------------------------------------------------------ 3. one step as a linear solve
@pytest.mark.parametrize("name", ["3x12x4_3f"] + list(EXTRA))
def test_one_step_within_its_backward_error_bar(name):
    cs, mc = _run(name)[:2]
    cv = mc.compact_view()
    sysm = sref.SubsetSystem(cv, cv.x0(), 1e4, dense=False)
    out = dense._solve(cs, 3, profile=True, max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
    _assert_eliminating(out)
    log = out["log"]
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    x1 = np.concatenate([out["params"].reshape(-1, 6)[mc.free_blocks].ravel(), np.concatenate([out["intr"], out["dist"][:, :2]], axis=1)[mc.cams].ravel()])
    assert x1[mc.held].tobytes() == mc.x0()[mc.held].tobytes()      # a held component's step is an exact zero
    r = sysm.check(x1[cv.keep])
    print("\nINTRELIMSTEP %s: n %d (%d kept) m %d kappa %.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e" % (
        name, mc.n, cv.n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"]))
    assert r["eta"] <= r["bar"], r
    assert abs(log[0, 1] - sysm.cost) <= 1e-12 * sysm.cost and abs(log[0, 3] - sysm.gmax) <= 1e-11 * sysm.gmax
    nd, tol = sysm.step_norm_tolerance(x1[cv.keep])
    assert abs(log[1, 4] - nd) <= tol, (log[1, 4], nd, tol)
    mcc, mcc_tol = sysm.model_cost_change(x1[cv.keep])
    assert abs(log[1, 2] / log[1, 5] - mcc) <= mcc_tol + 2 * 2.0 ** -53 * abs(mcc), (log[1, 2] / log[1, 5], mcc, mcc_tol)


# ------------------------------------------------------------------------------------------------ 4. without free intrinsics: 2
@pytest.mark.parametrize("which", ["4x40x6", "hongo"])
def test_without_free_intrinsics_three_is_two(which):
    prob = ref.hongo() if which == "hongo" else synthetic.make_marker_chain(4, 40, 6, seed=iref.RIG_SEED)
    cs = dict(prob=prob, dist=None, masks=[0] * 4, variant=0, loss="none", a=0.0, weights=None, constant_blocks=(), pose_masks={}, priors={})
    outs = []
    for impl, touch in ((2, False), (3, False), (3, True)):
        pr = capi.Problem.marker_chain(prob)
        try:
            if touch:
                for k in range(4):
                    pr.set_intrinsics_free(k, 0x3F)
                for k in range(4):
                    pr.set_intrinsics_free(k, 0)
            s = capi.Solver(pr, dense._options(cs, impl))
            try:
                s.configure_run(50, 1)
                summ = s.run()
                s.download()
                assert s.eliminates_times() == 1
                outs.append((dense._bits(dict(summary=summ, log=s.iterations(), params=pr.params.copy(), intr=pr.intrinsics, dist=np.zeros(1))),
                             sorted(s.kernel_stats(64))))
                assert pr.distortion is None
            finally:
                s.close()
        finally:
            pr.close()
    assert outs[0] == outs[1] == outs[2]
    assert not any(k.startswith("k_mc_intr") for k in outs[0][1])


# ------------------------------------------------------------------------------------------------ 5. reproducible, resident
def test_two_runs_and_two_solvers_return_identical_bits():
    cs = iref.case("3x70x5_mixed_all")
    first = dense._solve(cs, 3)
    assert first["elim"] == 1
    pr = dense._problem(cs)
    try:
        s = capi.Solver(pr, dense._options(cs, 3))
        try:
            got = []
            for turn in range(2):
                summ = s.run()
                s.download()
                params, intr, dist = dense._state(pr)
                got.append(dense._bits(dict(summary=summ, log=s.iterations(), params=params, intr=intr, dist=dist)))
                if turn == 0:   # the same values through the solver-level setters: nothing changes
                    s.set_observation_weights(cs["weights"])
                    for b, (A, v) in cs["priors"].items():
                        s.set_block_prior(6 * b, A, v)
            assert got[0] == got[1] == dense._bits(first)
        finally:
            s.close()
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 6. switches
def _child(env, tmp_path, tag):
    f = str(tmp_path / ("%s.npz" % tag))
    child_env = dict(os.environ)
    for k in ("RSBA_MT_ACC_MFMA", "RSBA_MT_CHUNKS", "RSBA_MT_FORK", "RSBA_MT_SOLVE_LDS", "RSBA_MT_SPLIT", "RSBA_MT_SPLIT_BACKSUB", "RSBA_MT_BACKSUB_WG"):
        child_env.pop(k, None)
    child_env.update(env)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "marker_intr_elim_worker.py"), "3x12x4_3f", f], env=child_env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(f)
    t = [int(v) for v in z["summary"]]
    summ = types.SimpleNamespace(termination_type=t[0], stop_reason=t[1], num_iterations=t[2], num_successful_steps=t[3], num_unsuccessful_steps=t[4],
                                 initial_cost=float(z["costs"][0]), final_cost=float(z["costs"][1]))
    return dict(summary=summ, log=z["log"], params=z["params"], intr=z["intr"], dist=z["dist"], rms=float(z["rms"]), rms_solver=float(z["rms_solver"]),
                elim=int(z["elim"]), stats={str(k): None for k in z["kernels"]})


SWITCHES = [{"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_CHUNKS": "3"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SOLVE_LDS": "0"},
            {"RSBA_MT_SPLIT": "0", "RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=[" ".join("%s=%s" % kv for kv in e.items()) for e in SWITCHES])
def test_switch_selects_a_path_at_the_parity_bar(env, tmp_path):
    out = _child(env, tmp_path, "set")
    _assert_eliminating(out)
    dense._compare("3x12x4_3f " + " ".join(env), out, _run("3x12x4_3f"))
    if "RSBA_MT_SPLIT" in env:   # ignored on this path: the bits of the unset run
        assert dense._bits(out) == dense._bits(_child({}, tmp_path, "unset"))


# ------------------------------------------------------------------------------------------------ 7. size
def test_the_problem_the_dense_path_refuses_solves():
    prob = synthetic.make_marker_chain(2, 1400, 2, seed=3)
    cs = dict(prob=prob, dist=None, masks=[0, 0x03], variant=0, loss="none", a=0.0, weights=None, constant_blocks=(), pose_masks={}, priors={})
    fixed = dense._solve(cs, 2, masks=[0, 0])
    pr = dense._problem(cs)
    try:
        s = capi.Solver(pr, dense._options(cs, 3))
        try:
            summ = s.run()
            s.download()
            elim, rms_solver = s.eliminates_times(), float(np.sqrt(s.final_costs()[1] / (8.0 * prob["N"])))
        finally:
            s.close()
        # (reprojection_error builds a solver of its own, with the default schur_impl: the mask, which that path refuses at this size,
        #  is cleared first — the refined values stay in the problem)
        pr.set_intrinsics_free(1, 0)
        rms = pr.reprojection_error()[1]
        assert pr.intrinsics[1, :2].tobytes() != np.asarray(prob["intr"], float).reshape(-1, 4)[1, :2].tobytes()
    finally:
        pr.close()
    print("2x1400x2: cost %.9e with fx fy of camera 1 free, %.9e fixed; %d iterations" % (summ.final_cost, fixed["summary"].final_cost, summ.num_iterations))
    assert elim == 1 and summ.termination_type == 0
    assert summ.final_cost < fixed["summary"].final_cost
    assert abs(rms - rms_solver) <= 1e-9, (rms, rms_solver)


# ------------------------------------------------------------------------------------------------ 8. zero noise
def test_zero_noise_reaches_the_truth():
    cs = iref.case("3x12x4_3f", noise=0.0)
    out = dense._solve(cs, 3)
    err = np.abs(np.concatenate([out["intr"], out["dist"][:, :2]], axis=1) - cs["truth_six"])
    print("zero noise: cost %.2e, intrinsics %.2e px off the truth, k1 k2 %.2e" % (out["summary"].final_cost, err[:, :4].max(), err[:, 4:].max()))
    assert out["elim"] == 1
    assert err[:, :4].max() < 1e-4 and err[:, 4:].max() < 1e-6


# ------------------------------------------------------------------------------------------------ 9. fallback and refusals
def test_a_duplicated_detection_takes_the_dense_path():
    cs = iref.case("3x12x4_3f")
    p = cs["prob"]
    dup = dict(p, N=p["N"] + 1, t=np.append(p["t"], p["t"][0]), c=np.append(p["c"], p["c"][0]), m=np.append(p["m"], p["m"][0]),
               obs=np.concatenate([np.asarray(p["obs"]), np.asarray(p["obs"])[:1]]))
    cs = dict(cs, prob=dup)
    a, b = dense._solve(cs, 3), dense._solve(cs, 2)
    assert a["elim"] == 0 and b["elim"] == 0
    assert dense._bits(a) == dense._bits(b)


def test_queries_stay_refused_on_an_eliminating_solver():
    cs = iref.case("3x12x4_0f")
    pr = dense._problem(cs)
    try:
        s = capi.Solver(pr, dense._options(cs, 3))
        try:
            s.run()
            for call in (lambda: s.evaluate(), lambda: s.evaluate_jacobian(), lambda: s.jacobian_structure(), lambda: s.covariance_compute(),
                         lambda: s.set_parameters(pr.params.copy())):
                with pytest.raises(capi.RsbaError) as e:
                    call()
                assert e.value.code == capi.ERR_UNSUPPORTED
            s.download()     # and the solver is as it was
            assert s.eliminates_times() == 1 and len(s.iterations()) > 2
        finally:
            s.close()
    finally:
        pr.close()


def test_a_mask_on_a_camera_no_observation_names_is_refused():
    cs = iref.case("3x12x4_3f")
    prob = cs["prob"]
    keep = np.asarray(prob["c"]) != 2
    prob = dict(prob, N=int(keep.sum()), t=prob["t"][keep], c=prob["c"][keep], m=prob["m"][keep], obs=np.asarray(prob["obs"])[keep])
    pr = capi.Problem.marker_chain(prob)
    try:
        pr.set_intrinsics_free(0, 0x0F)
        pr.set_intrinsics_free(2, 0x01)
        with pytest.raises(capi.RsbaError) as e:
            capi.Solver(pr, capi.default_options(schur_impl=3))
        assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        pr.close()
