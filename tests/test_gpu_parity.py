"""Parity of the HIP path (through the C ABI) against the oracle.  Run on the GPU box: -m gpu.

Tolerances are BASELINE.json's: final poses/points within 1e-6 relative, reprojection RMS within 1e-4 px,
and — because parity of the *result* needs parity of the *trajectory* — the same iteration count, the
same accept/reject sequence and the same termination reason.
"""
import os

import numpy as np
import pytest

import oracle_lib as ol
import oracle_spread
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu
G = ol.GOLDEN
IMPLS = [0, 1]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = capi.load()
    assert lib.rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"
    return lib


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _block_rel(a, b, C):
    """max over 6-/3-blocks of |da| / max(|b|, 1e-12)."""
    worst = 0.0
    for x, y in ((a[:6 * C].reshape(-1, 6), b[:6 * C].reshape(-1, 6)), (a[6 * C:].reshape(-1, 3), b[6 * C:].reshape(-1, 3))):
        worst = max(worst, (np.abs(x - y).max(axis=1) / np.maximum(np.abs(y).max(axis=1), 1e-12)).max())
    return worst


# ------------------------------------------------------------------ stage level: one linearisation
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("C,P,k,radius", [(6, 40, 4, 1e4), (8, 300, 8, 1e4), (8, 300, 5, 2.5), (13, 700, 7, 1e2)])
def test_reduced_system_and_step_match_oracle(oracle, impl, C, P, k, radius):
    prob = syn.make_problem(C, P, k, seed=100 + C)
    ref = oracle.points_linearize_and_step(prob, prob["params"], radius)
    got = capi.points_linearize_and_step(prob, radius, capi.default_options(schur_impl=impl))
    assert got["solve_ok"] and ref["solve_ok"]
    sc = np.abs(ref["S"]).max()
    assert np.abs(got["S"] - ref["S"]).max() < 1e-11 * sc
    assert np.abs(got["S"] - got["S"].T).max() == 0.0
    assert np.abs(got["rhs"] - ref["rhs"]).max() < 1e-11 * np.abs(ref["rhs"]).max()
    assert abs(got["cost"] - ref["cost"]) < 1e-12 * ref["cost"]
    assert abs(got["gradient_max_norm"] - ref["gradient_max_norm"]) < 1e-11 * ref["gradient_max_norm"]
    assert np.abs(got["delta"] - ref["delta"]).max() < 1e-8 * np.abs(ref["delta"]).max()
    assert abs(got["model_cost_change"] - ref["model_cost_change"]) < 1e-9 * abs(ref["model_cost_change"])
    cand_cost, _ = oracle.points_cost(prob, prob["params"] + ref["delta"])
    assert abs(got["cost_candidate"] - cand_cost) < 1e-7 * cand_cost
    assert abs(got["step_norm"] - np.linalg.norm(ref["delta"])) < 1e-8 * np.linalg.norm(ref["delta"])
    assert abs(got["x_norm"] - np.linalg.norm(prob["params"])) < 1e-12 * np.linalg.norm(prob["params"])


# ------------------------------------------------------------------ whole solves
def _compare_solve(oracle, prob, impl, huber=0.0, params_bar=1e-6, iter_cost_tol=1e-7, **optkw):
    """Whole solve against the oracle.  `params_bar`: the bar on the RAW parameters, per block — BASELINE.json's 1e-6 unless
    the caller has measured that the oracle itself does not meet it on this problem (oracle_spread.bars); no alignment
    along the gauge orbit anywhere.  Returns (parameters, summary, log, raw parameter difference)."""
    o_ref = oracle.options(huber_delta=huber, **optkw)
    ref, s_ref, log_ref = oracle.solve_points(prob, o_ref)
    got, s_got, log_got = capi.solve_points(prob, capi.default_options(schur_impl=impl, huber_delta=huber, **optkw))
    assert s_got.termination_type == s_ref.termination and s_got.stop_reason == s_ref.stop_reason
    assert s_got.num_iterations == s_ref.num_iterations
    assert (s_got.num_successful_steps, s_got.num_unsuccessful_steps) == (s_ref.num_successful_steps, s_ref.num_unsuccessful_steps)
    assert np.array_equal(log_got[:, 7], log_ref[:, 7])  # same accept / reject sequence
    assert abs(s_got.initial_cost - s_ref.initial_cost) < 1e-11 * s_ref.initial_cost
    assert abs(s_got.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    # every iterate has the same cost (relative to the largest cost on the trajectory)
    assert np.abs(log_got[:, 1] - log_ref[:, 1]).max() / log_ref[:, 1].max() < iter_cost_tol
    rel = _block_rel(got, ref, prob["C"])
    assert rel < params_bar, "raw parameters differ by %.2e (bar %.1e)" % (rel, params_bar)
    c_ref, ss_ref = oracle.points_cost(prob, ref)
    c_got, ss_got = oracle.points_cost(prob, got)
    rms_ref, rms_got = np.sqrt(ss_ref / (2 * prob["N"])), np.sqrt(ss_got / (2 * prob["N"]))
    assert abs(rms_ref - rms_got) < 1e-4
    return got, s_got, log_got, rel


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("C,P,k,seed", [(4, 60, 3, 1), (8, 2000, 6, 21), (16, 3000, 9, 7), (3, 500, 3, 4)])
def test_solve_matches_oracle(oracle, impl, C, P, k, seed):
    _compare_solve(oracle, syn.make_problem(C, P, k, seed=seed), impl)


@pytest.mark.parametrize("C,P,k,huber", [(40, 2500, 30, 0.0), (40, 2500, 30, 1.5), (96, 2000, 24, 0.0), (96, 2000, 24, 1.5), (128, 1500, 14, 0.0),
                                          (200, 1200, 26, 0.0), (200, 1200, 26, 1.5)])
def test_back_substitution_record_paths(oracle, C, P, k, huber):
    """k_backsub_candidate_proj keeps a lane's first observation records in registers (ten; seven in the robust instances),
    the next ones in LDS (ten / eleven up to 64 cameras, six / seven up to 128, ten up to 256) and streams the rest.  30 views at
    40 cameras, 24 at 96 and 26 at 200 go through all three paths of all six instances — <64>, <128>, <256> with and without the
    robust loss (a template parameter); 200 cameras without a loss is k_backsub_candidate_proj<256, 10, 10, false>, which no
    BASELINE configuration reaches.  Raw parameters at 1e-6."""
    prob = syn.make_problem(C, P, k, seed=300 + C, outlier_frac=0.05 if huber else 0.0)
    _compare_solve(oracle, prob, 1, huber=huber)


@pytest.mark.parametrize("impl", IMPLS)
def test_config2_full_size(oracle, impl):
    """BASELINE.json configs[1]: 8 cams x 10k points, 80k observations."""
    prob = syn.make_config("cfg2")
    got, s, log, _ = _compare_solve(oracle, prob, impl)
    assert prob["N"] == 80_000


@pytest.mark.parametrize("impl", IMPLS)
def test_huber_and_rejected_steps(oracle, impl):
    """17 iterations, the radius grows to 4e11 with every block free (Test1_BundleAdjustment/main.cpp:76-79 fixes none): the
    suite's longest robust run.  RAW parameters at 1e-6 — three executions of the oracle end within 1e-7 of each other here
    (tests/test_oracle_self_sensitivity.py), so the bar is defined, and the HIP path measures 4e-8.  Round 2 compared this case
    modulo the gauge orbit because its back-substitution ended 1.5e-5 away: that kernel formed the candidate's residuals —
    the next iteration's g_p — from rows pre-multiplied by fx while the Schur kernel formed g_c from R and t, a mismatch of
    ~1e-13 px that the radius amplified along the orbit.  Every residual that enters a gradient now comes from ONE function
    (ProjectResidual, csrc/ba_math.hpp)."""
    prob = syn.make_problem(8, 1500, 6, seed=9, outlier_frac=0.05)
    _, s, _, rel = _compare_solve(oracle, prob, impl, huber=1.0)
    assert s.num_iterations == 17 and rel < 5e-7


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("sigma,radius0,seed,min_rejected", [(0.7, 1e4, 2, 2), (0.65, 1e6, 2, 5)])
def test_rejected_steps_follow_the_same_trajectory(oracle, impl, sigma, radius0, seed, min_rejected):
    """A far-off start: rejected steps, radius shrinkage by 2, 4, 8, ... and recovery.

    All cameras and points are free (as in Test1_BundleAdjustment/main.cpp:76-79), so the cost has a 7-dof gauge orbit, and far
    from the minimum the damped systems are ill-conditioned (cond ~1e12): on these 20-iteration trajectories with up to six
    rejections the ORACLE's own runs end ~1e-2 apart in the parameters when only its roundings change.  The bar on the raw
    parameters is therefore ten times the oracle's own spread, measured here (oracle_spread); costs, decisions, RMS as
    everywhere."""
    prob = syn.make_problem(8, 1500, 6, seed=9, outlier_frac=0.05)
    rng = np.random.default_rng(seed)
    bad = dict(prob)
    bad["params"] = prob["params"] + np.concatenate([rng.normal(0, sigma, 48), rng.normal(0, sigma, 3 * prob["P"])])
    sp = oracle_spread.spread(oracle, bad, dict(initial_trust_region_radius=radius0))
    assert sp["same_trajectory"]
    bar = oracle_spread.bars(sp, bad["N"])["raw"]
    # intermediate costs of two correct solvers agree to ~1e-5 there, not 1e-7; the decisions and the end point coincide
    got, s, log, rel = _compare_solve(oracle, bad, impl, params_bar=bar, iter_cost_tol=1e-3, initial_trust_region_radius=radius0)
    assert s.num_unsuccessful_steps >= min_rejected
    print("raw parameters %.2e, the oracle against itself %.2e" % (rel, sp["raw"]))


@pytest.mark.parametrize("impl", IMPLS)
def test_invalid_steps_end_in_failure(oracle, impl):
    """A camera without observations and min_lm_diagonal = 0 make the reduced system exactly singular: the
    Cholesky fails, every step is invalid, and after max_num_consecutive_invalid_steps (5) the solve ends in
    FAILURE with the parameters left at the starting point (Ceres: HandleInvalidStep)."""
    prob = syn.make_problem(5, 300, 3, seed=12)
    keep = prob["cam_idx"] != 4
    q = dict(prob)
    q["cam_idx"] = np.ascontiguousarray(prob["cam_idx"][keep])
    q["pt_idx"] = np.ascontiguousarray(prob["pt_idx"][keep])
    q["obs"] = np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1))
    q["N"] = int(keep.sum())
    ref, s_ref, _ = oracle.solve_points(q, oracle.options(min_lm_diagonal=0.0))
    got, s, log = capi.solve_points(q, capi.default_options(schur_impl=impl, min_lm_diagonal=0.0))
    assert (s_ref.termination, s_ref.stop_reason, s_ref.num_iterations) == (2, 6, 5)
    assert (s.termination_type, s.stop_reason, s.num_iterations, s.num_unsuccessful_steps) == (2, 6, 5, 5)
    assert np.array_equal(got, q["params"]) and np.array_equal(ref, q["params"])
    assert np.allclose(log[1:5, 6], [5e3, 1250.0, 156.25, 9.765625])  # radius / 2, / 4, / 8, / 16


@pytest.mark.parametrize("impl", IMPLS)
def test_two_cam_data_file(oracle, impl):
    """The reference's only point-model input, through the product's own loader."""
    K = ol.read_intrinsics([ol.SERIALS_TEST2[1]])[0]
    p = capi.Problem.points_file(os.path.join(G, "two_cam_data.txt"), K)
    ref_prob = ol.read_two_cam_data(os.path.join(G, "two_cam_data.txt"))
    ref_prob["intr"] = np.ascontiguousarray(np.tile(K, ref_prob["C"]))
    ref, s_ref, _ = oracle.solve_points(ref_prob)
    s = p.solve(capi.default_options(schur_impl=impl))
    assert s.num_iterations == s_ref.num_iterations and s.stop_reason == s_ref.stop_reason
    assert abs(s.final_cost - s_ref.final_cost) < 1e-6 * max(s_ref.final_cost, 1e-12) + 1e-12
    # under-determined problem (1 camera, 16 points, all free): compare the fit, and loosely the parameters
    c_got, ss_got = oracle.points_cost(ref_prob, p.params)
    assert abs(np.sqrt(ss_got / 32) - np.sqrt(2 * s_ref.final_cost / 32)) < 1e-4
    p.close()


def test_unordered_observations_and_ragged_views(oracle):
    """Observation order is the caller's; points with 1 view, and a camera with no observations."""
    prob = syn.make_problem(7, 400, 5, seed=33)
    rng = np.random.default_rng(0)
    keep = rng.random(prob["N"]) > 0.3
    keep &= prob["cam_idx"] != 6            # camera 6 sees nothing
    first = np.unique(prob["pt_idx"], return_index=True)[1]
    keep[first] = True                       # every point keeps at least one view
    keep[first[prob["cam_idx"][first] == 6]] = True
    perm = rng.permutation(int(keep.sum()))
    q = dict(prob)
    q["cam_idx"] = np.ascontiguousarray(prob["cam_idx"][keep][perm])
    q["pt_idx"] = np.ascontiguousarray(prob["pt_idx"][keep][perm])
    q["obs"] = np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep][perm].reshape(-1))
    q["N"] = int(keep.sum())
    a = oracle.points_linearize_and_step(q, q["params"], 1e4)
    b = capi.points_linearize_and_step(q, 1e4)
    assert np.abs(b["S"] - a["S"]).max() < 1e-11 * np.abs(a["S"]).max()
    assert np.abs(b["delta"] - a["delta"]).max() < 1e-8 * np.abs(a["delta"]).max()


# ------------------------------------------------------------------ marker-chain model (config 1)
def test_hongo_fixture_on_gpu_matches_committed_output(oracle, tmp_path):
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    p = capi.Problem.correspondence(os.path.join(G, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    s = p.solve()
    assert s.termination_type == capi.CONVERGENCE and s.stop_reason == 3
    assert s.num_iterations == 7 and s.num_successful_steps == 6 and s.num_unsuccessful_steps == 0
    assert abs(s.initial_cost - 138796.696054) < 1e-5 and abs(s.final_cost - 143.629388852) < 1e-7
    xml = str(tmp_path / "Camera_Transform.xml")
    p.write_outputs(xml, None, None)
    got, want = ol.read_opencv_xml(xml), ol.read_opencv_xml(os.path.join(G, "hongo", "Camera_Transform.xml"))
    for k in want:
        assert np.abs(got[k] - want[k]).max() < 1e-9, k   # reference's own Ceres output
    err, rms = p.reprojection_error()
    assert abs(rms - 0.726669955) < 1e-7
    assert np.all(p.params[:6] == 0) and np.all(p.params[60:66] == 0)  # camera 0 / marker 0 untouched
    n, counts, pts = ol.read_point3d(os.path.join(G, "hongo", "point3d.txt"))
    assert np.abs(p.point3d() - pts).max() < 6e-7
    p.close()


def test_test2_fixture_on_gpu(oracle):
    intr = ol.read_intrinsics(ol.SERIALS_TEST2)
    p = capi.Problem.correspondence(os.path.join(G, "test2", "correspondence_test.txt"), capi.MODEL_MARKER_CHAIN_TEST2, ol.MARKER_SIDE_TEST2, intr)
    s = p.solve()
    xml = ol.read_opencv_xml(os.path.join(G, "test2", "Camera_Transform.xml"))
    assert s.num_iterations == 4 and s.stop_reason == 3
    assert np.abs(p.params[6:9] - xml["R1"].ravel()).max() < 1e-9
    assert np.abs(p.params[9:12] - xml["t1"].ravel()).max() < 1e-9
    p.close()


def test_cpp_bamanager_mirror_end_to_end(tmp_path):
    """examples/main_calibration.cpp: the reference's BAManager sequence (ctor -> StartBA -> Write) through the
    C++ mirror headers, compiled with g++ against librsba.so, on the committed hongo input."""
    import subprocess
    exe = str(tmp_path / "main_calibration")
    lib = os.path.join(ol.ROOT, "realsensecalibration_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ol.ROOT, "include"), os.path.join(ol.ROOT, "examples", "main_calibration.cpp"),
                           "-L" + lib, "-lrsba", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, G, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "Termination: CONVERGENCE" in out.stdout and "Iterations: 7 (successful 6, unsuccessful 0)" in out.stdout
    got, want = ol.read_opencv_xml(str(tmp_path / "Camera_Transform.xml")), ol.read_opencv_xml(os.path.join(G, "hongo", "Camera_Transform.xml"))
    for k in want:
        assert np.abs(got[k] - want[k]).max() < 1e-9
    for i in range(4):
        assert np.abs(np.loadtxt(str(tmp_path / ("mat%d.txt" % i))) - np.loadtxt(os.path.join(G, "extrinsics", "mat%d.txt" % i))).max() < 2e-6
    rms = float(out.stdout.split("Average Reprojection Error per One Coordinate:")[1].split()[0])
    assert abs(rms - 0.726669955) < 1e-6
    # ... and the reference's own file-driven check on what was just written (6-digit text): 0.726696
    rms_files = float(out.stdout.split("From the written files:")[1].split()[1])
    assert abs(rms_files - 0.726696372) < 2e-6


def test_rccl_collective_path_single_rank(oracle):
    """RSBA_FORCE_COMM=1 builds a 1-rank RCCL communicator, so the three all-reduces of the multi-GPU path really run
    (sum of the packed reduced system, max of the gradient bound, sum of the candidate scalars).  With one rank they
    are identities: the solve must match the oracle exactly as the plain path does."""
    prob = syn.make_problem(8, 2000, 6, seed=21)
    ref, s_ref, _ = oracle.solve_points(prob)
    os.environ["RSBA_FORCE_COMM"] = "1"
    try:
        got, s, log = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_FORCE_COMM"]
    assert s.num_iterations == s_ref.num_iterations and s.stop_reason == s_ref.stop_reason
    assert _block_rel(got, ref, prob["C"]) < 1e-6
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost


def test_configure_run_changes_the_next_run_only():
    """rsba_solver_configure_run: the same solver stopped after 2 iterations, then run for 5, gives what a fresh solver
    with max_num_iterations = 5 gives, bit for bit (a run restarts from the uploaded state); bad arguments are refused."""
    prob = syn.make_problem(24, 2500, 8, seed=77)
    problem = capi.Problem.points(prob)
    fixed = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0)
    sv = capi.Solver(problem, capi.default_options(max_num_iterations=2, **fixed))
    assert sv.run().num_iterations == 2
    sv.configure_run(5, 2)
    s5 = sv.run()
    log5 = sv.iterations()
    assert "k_schur_tiles" in sv.kernel_stats()
    for bad in ((-1, 0), (3, 7)):
        with pytest.raises(capi.RsbaError):
            sv.configure_run(*bad)
    sv.close()
    fresh = capi.Solver(problem, capi.default_options(max_num_iterations=5, **fixed))
    f5 = fresh.run()
    assert s5.num_iterations == f5.num_iterations == 5 and s5.final_cost == f5.final_cost
    assert np.array_equal(log5, fresh.iterations())
    fresh.close()
    problem.close()


def test_max_solver_time_ends_the_run_like_ceres():
    """Solver::Options::max_solver_time_in_seconds (Ceres' default 1e9; the reference leaves it alone,
    Main_Calibration/bundle_adjustment_manager.cpp:90-92): TrustRegionMinimizer tests it in FRONT of the iteration limit and for
    the first time right behind iteration 0 (FinalizeIterationAndCheckIfMinimizerCanContinue), against minimiser + preprocessor
    time — a run whose budget is 0 s returns its start with NO step taken, NO_CONVERGENCE and the 'Maximum solver time reached'
    line in the report, even when the iteration limit is reached at the same moment; the default changes nothing.  (Several ranks:
    rank 0's clock decides for all, tests/test_gpu_loopback.py::test_max_solver_time_with_several_ranks_stops_every_rank_on_the_same_iteration.)"""
    prob = syn.make_problem(24, 2500, 8, seed=78)
    problem = capi.Problem.points(prob)
    fixed = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0)
    sv = capi.Solver(problem, capi.default_options(max_num_iterations=20, max_solver_time_in_seconds=0.0, **fixed))
    s = sv.run()
    assert (s.termination_type, s.stop_reason, s.num_iterations) == (capi.NO_CONVERGENCE, 8, 0)
    rep = sv.full_report()
    assert s.final_cost == s.initial_cost and "Maximum solver time reached" in rep
    # (the printed left-hand side is the value the test compares — minimiser + set-up time — and so never below the limit)
    import re
    m = re.search(r"Total solver time: ([0-9.eE+-]+) >= ([0-9.eE+-]+?)\.?[)\s]", rep + " ")
    assert m and float(m.group(1)) >= float(m.group(2)), rep
    sv.download()
    assert np.array_equal(problem.params, prob["params"]), "a zero budget must leave the start untouched"
    sv.close()
    # time is tested before the iteration count: with both exhausted the reason is the time
    sv = capi.Solver(problem, capi.default_options(max_num_iterations=0, max_solver_time_in_seconds=0.0, **fixed))
    assert sv.run().stop_reason == 8
    sv.close()
    sv = capi.Solver(problem, capi.default_options(max_num_iterations=6, **fixed))
    assert capi.default_options().max_solver_time_in_seconds == 1e9 and sv.run().num_iterations == 6
    sv.close()
    with pytest.raises(capi.RsbaError):
        capi.Solver(problem, capi.default_options(max_solver_time_in_seconds=-1.0))
    problem.close()


def test_solve_is_bitwise_reproducible():
    """The default path has no atomics: every reduction runs in a fixed order, so two solves of the same problem
    give bit-identical parameters and iteration logs (and every rank of a multi-GPU run factors identical bits)."""
    prob = syn.make_problem(16, 3000, 9, seed=7)
    a, sa, la = capi.solve_points(prob)
    b, sb, lb = capi.solve_points(prob)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and sa.final_cost == sb.final_cost


@pytest.mark.parametrize("impl", IMPLS)
def test_more_than_64_cameras_and_huber(oracle, impl):
    """C = 70: reduced system 420 x 420, larger than the LDS-panel Cholesky handles (the global-memory factorisation
    takes over), 5 camera groups (15 pair tiles + 5 self tiles), camera constants no longer LDS-staged in the
    back-substitution; with Huber loss and outliers as BASELINE.json configs[4] asks."""
    prob = syn.make_problem(70, 1500, 10, seed=5, outlier_frac=0.05)
    _compare_solve(oracle, prob, impl, huber=1.0)
    a = oracle.points_linearize_and_step(prob, prob["params"], 1e4, opts=oracle.options(huber_delta=1.0))
    b = capi.points_linearize_and_step(prob, 1e4, capi.default_options(schur_impl=impl, huber_delta=1.0))
    assert np.abs(b["S"] - a["S"]).max() < 1e-10 * np.abs(a["S"]).max()
    assert np.abs(b["delta"] - a["delta"]).max() < 1e-7 * np.abs(a["delta"]).max()


# ------------------------------------------------------------------ pipelined solve (17..64 cameras on one GPU)
@pytest.mark.parametrize("C,P,k,huber", [(17, 1200, 6, 0.0), (33, 2500, 8, 0.0), (40, 3000, 9, 0.0), (64, 4000, 12, 1.0)])
def test_pipelined_solve_matches_oracle_and_sequential_schedule(oracle, C, P, k, huber):
    """With 17..64 cameras the Cholesky of the reduced system is launched first and factors camera group g's
    columns as soon as the Schur kernel has published them (ready flags), while the later groups are still being
    eliminated.  Same kernels, same summation orders: the result must equal the oracle's within the usual tolerances
    and the sequential schedule's (RSBA_PIPELINE=0, same segment size) bit for bit.  C = 17 leaves a last group of one camera (a stage
    without any pair tile), C = 64 is the benchmark's shape, with Huber loss and outliers."""
    prob = syn.make_problem(C, P, k, seed=300 + C, outlier_frac=0.05 if huber else 0.0)
    got, s, log, _ = _compare_solve(oracle, prob, 1, huber=huber)
    os.environ["RSBA_PIPELINE"] = "0"
    os.environ["RSBA_SEG_TARGET"] = "8"   # the pipelined default (eight per CU through the whole-chunk rounding): same segments, same summation order
    try:
        seq, s_seq, log_seq = capi.solve_points(prob, capi.default_options(schur_impl=1, huber_delta=huber))
    finally:
        del os.environ["RSBA_PIPELINE"]
        del os.environ["RSBA_SEG_TARGET"]
    assert np.array_equal(got, seq) and np.array_equal(log, log_seq) and s.final_cost == s_seq.final_cost
    again, s2, log2 = capi.solve_points(prob, capi.default_options(schur_impl=1, huber_delta=huber))
    assert np.array_equal(got, again) and np.array_equal(log, log2)


def _in_the_frame_of_camera(prob, c0):
    """The same problem expressed in camera c0's (initial) orientation: points X' = R0 X, rotations R' = R R0', so
    camera c0's angle-axis vector is exactly zero — AngleAxisRotatePoint's first-order branch and its derivative
    (in the reference that is camera 0 and every marker of the test2 fixture)."""
    C = prob["C"]
    out = dict(prob)
    par = prob["params"].copy()
    cams = par[:6 * C].reshape(C, 6)
    R = syn._matrix_from_rotvec(cams[:, :3])
    R0 = R[c0]
    cams[:, :3] = syn._rotvec_from_matrix(R @ R0.T)
    cams[c0, :3] = 0.0
    par[6 * C:] = (par[6 * C:].reshape(-1, 3) @ R0.T).reshape(-1)
    out["params"] = par
    return out


@pytest.mark.parametrize("C,P,k,c0,impl", [(8, 1500, 6, 0, 0), (8, 1500, 6, 5, 1), (24, 2600, 8, 0, 1), (40, 3000, 9, 21, 1), (64, 3600, 12, 63, 1)])
def test_camera_with_zero_rotation_takes_the_small_angle_branch(oracle, C, P, k, c0, impl):
    """A camera whose angle-axis vector is exactly zero is linearised with the first-order rotation; the tiled Schur
    kernel compiles that select into a second instance of its pair tiles, taken only by the tiles that hold such a
    camera (with 24+ cameras both instances run in the same launch)."""
    prob = _in_the_frame_of_camera(syn.make_problem(C, P, k, seed=900 + C), c0)
    assert np.all(prob["params"][6 * c0:6 * c0 + 3] == 0.0)
    _compare_solve(oracle, prob, impl)


@pytest.mark.parametrize("cameras", [24, 40])   # (40: the border's workgroup, ba_cholesky_border.hpp, is the one that ends the solve)
@pytest.mark.parametrize("who", ["1", "2"])
def test_pipeline_stall_falls_back_to_sequential_schedule(oracle, capfd, who, cameras):
    """RSBA_TEST_STALL=1 makes the waiting Cholesky look for a tag nobody publishes: it must give up after its 0.5 s
    budget (never hang the queue), the step must be repeated with the sequential schedule, and the result must not
    change."""
    prob = syn.make_problem(cameras, 1500 if cameras == 24 else 3000, 7 if cameras == 24 else 9, seed=77)
    ref, s_ref, log_ref = capi.solve_points(prob)
    os.environ["RSBA_TEST_STALL"] = who   # 1: the Cholesky's wait, 2: the back-substitution's wait for the solve
    try:
        got, s, log = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_TEST_STALL"]
    assert "falling back" in capfd.readouterr().err
    assert np.array_equal(got, ref) and np.array_equal(log, log_ref) and s.num_iterations == s_ref.num_iterations


def test_double_fault_with_the_border_ends_in_the_one_workgroup_factorisation_for_good(oracle, capfd):
    """RSBA_TEST_STALL=4: the first pipelined step stalls, and its sequential repeat reports a stalled
    multi-workgroup factorisation too.  With the border (40 cameras) the Schur work list's stages are permuted (2 Bg + 1 of them),
    which the one-workgroup factorisation's gates do not describe: the solver must drop the border AND stay sequential — re-enabled,
    the pipelined schedule would factor panels whose border rows are still being accumulated, silently.  The one-workgroup kernel
    rounds differently from the diagonal-chain kernel: the bar is the oracle's, not bitwise equality."""
    prob = syn.make_problem(40, 3000, 9, seed=77)
    o_ref = oracle.options()
    ref, s_ref, log_ref = oracle.solve_points(prob, o_ref)
    os.environ["RSBA_TEST_STALL"] = "4"
    p = capi.Problem.points(prob)
    sv = capi.Solver(p, capi.default_options())
    try:
        before = sv.schedule_info()
        s = sv.run()
        sv.download()
        log = sv.iterations()
        got = p.params.copy()
        after = sv.schedule_info()
    finally:
        del os.environ["RSBA_TEST_STALL"]
        sv.close()
        p.close()
    err = capfd.readouterr().err
    assert err.count("pipelined solve stalled") == 1 and err.count("multi-workgroup Cholesky stalled") == 1, err
    assert before["schedule"] == "pipelined" and before["chol_workgroups"] == 4   # (one diagonal + two row workgroups + the border's)
    assert after["schedule"] == "sequential" and after["chol_workgroups"] == 1 and after["stalls"] == 2 and after["fallbacks"] >= 1
    assert s.num_iterations == s_ref.num_iterations and np.array_equal(log[:, 7], log_ref[:, 7])
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert _block_rel(got, ref, prob["C"]) < 1e-6


def test_file_driven_reprojection_check_matches_reference_numbers(oracle):
    """reprojection_check.cpp:5-101 from the committed files: 6-digit point3d.txt, R/t from Camera_Transform.xml,
    float32 corners.  The hongo numbers are the ones the oracle's restatement of that text path gives
    (tests/test_oracle_golden.py::test_hongo_reference_text_path_rms); test2's XML holds rvecs instead of matrices."""
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    err, rms = capi.reprojection_check_files(os.path.join(G, "hongo", "correspondence.txt"), os.path.join(G, "hongo", "point3d.txt"),
                                             os.path.join(G, "hongo", "Camera_Transform.xml"), intr)
    assert abs(err - 143.639831820) < 1e-6 and abs(rms - 0.726696372) < 1e-8
    intr2 = ol.read_intrinsics(ol.SERIALS_TEST2)
    err2, rms2 = capi.reprojection_check_files(os.path.join(G, "test2", "correspondence_test.txt"), os.path.join(G, "test2", "point3d.txt"),
                                               os.path.join(G, "test2", "Camera_Transform.xml"), intr2)
    # same computation in numpy
    prob = ol.read_correspondence(os.path.join(G, "test2", "correspondence_test.txt"))
    xml = ol.read_opencv_xml(os.path.join(G, "test2", "Camera_Transform.xml"))
    n, counts, pts = ol.read_point3d(os.path.join(G, "test2", "point3d.txt"))
    ref = 0.0
    for i in range(prob["N"]):
        c = prob["c"][i]
        R = oracle.rodrigues(xml["R%d" % c].ravel())
        t = xml["t%d" % c].ravel()
        fx, fy, px, py = intr2[c]
        for j in range(4):
            q = R @ pts[4 * i + j] + t
            u, v = fx * q[0] / q[2] + px, fy * q[1] / q[2] + py
            ou, ov = np.float32(prob["obs"][8 * i + 2 * j]), np.float32(prob["obs"][8 * i + 2 * j + 1])
            ref += ((float(ou) - u) ** 2 + (float(ov) - v) ** 2) / 2
    assert abs(err2 - ref) < 1e-9 * max(ref, 1.0) and abs(rms2 - np.sqrt(ref * 2.0 / (n * 2.0))) < 1e-10


# ------------------------------------------------------------------ edge cases of the input
def test_duplicate_observations_and_unobserved_points(oracle):
    """A camera that observes the same point twice (two residual blocks on the same parameter pair, as Ceres allows)
    cannot use one visibility bit per (camera, point): the solver must notice and take the atomic kernel, still on
    the GPU.  Points nobody observes must stay where they are."""
    prob = syn.make_problem(6, 300, 4, seed=41)
    rng = np.random.default_rng(1)
    dup = rng.choice(prob["N"], 40, replace=False)
    drop_pts = np.array([3, 77, 299])
    keep = ~np.isin(prob["pt_idx"], drop_pts)
    cam = np.concatenate([prob["cam_idx"][keep], prob["cam_idx"][dup][~np.isin(prob["pt_idx"][dup], drop_pts)]])
    pt = np.concatenate([prob["pt_idx"][keep], prob["pt_idx"][dup][~np.isin(prob["pt_idx"][dup], drop_pts)]])
    obs2 = prob["obs"].reshape(-1, 2)
    dup_obs = obs2[dup][~np.isin(prob["pt_idx"][dup], drop_pts)] + rng.normal(0, 0.3, (len(cam) - int(keep.sum()), 2))
    q = dict(prob)
    q["cam_idx"] = np.ascontiguousarray(cam.astype(np.int32)); q["pt_idx"] = np.ascontiguousarray(pt.astype(np.int32))
    q["obs"] = np.ascontiguousarray(np.concatenate([obs2[keep], dup_obs]).reshape(-1)); q["N"] = len(cam)
    got, s, log, _ = _compare_solve(oracle, q, 1)
    C = q["C"]
    for j in drop_pts:
        assert np.array_equal(got[6 * C + 3 * j: 6 * C + 3 * j + 3], q["params"][6 * C + 3 * j: 6 * C + 3 * j + 3])


def test_every_camera_sees_every_point_more_than_64_views(oracle):
    """k = C = 66 views per point: more than one 64-bit word of cameras per point, 5 camera groups, the multi-launch
    Cholesky (396 x 396)."""
    prob = syn.make_problem(66, 400, 66, seed=43)
    assert prob["N"] == 66 * 400
    _compare_solve(oracle, prob, 1)


def test_problem_without_observations(oracle):
    """No residual blocks: cost 0, gradient 0 — Ceres converges at iteration 0 on the gradient tolerance and leaves
    the parameters alone."""
    prob = syn.make_problem(3, 20, 2, seed=44)
    q = dict(prob)
    q["cam_idx"] = np.zeros(0, np.int32); q["pt_idx"] = np.zeros(0, np.int32); q["obs"] = np.zeros(0); q["N"] = 0
    got, s, log = capi.solve_points(q)
    assert s.termination_type == 0 and s.num_iterations == 0 and s.initial_cost == 0.0 and s.final_cost == 0.0
    assert np.array_equal(got, q["params"])


def test_cauchy_loss_matches_oracle(oracle):
    """ceres::CauchyLoss(a) (rho = a^2 log(1 + s / a^2), rho'' < 0: the corrector scales residual and Jacobians by
    sqrt(rho')), SURVEY 8(f) rank 4.  Outliers as in config 5; the oracle takes the Cauchy scale as a negative
    huber_delta (its own convention)."""
    prob = syn.make_problem(20, 1500, 8, seed=51, outlier_frac=0.05)
    o_ref = oracle.options(huber_delta=-2.0)
    ref, s_ref, log_ref = oracle.solve_points(prob, o_ref)
    got, s, log = capi.solve_points(prob, capi.default_options(huber_delta=2.0, loss_type=1))
    assert (s.termination_type, s.stop_reason, s.num_iterations) == (s_ref.termination, s_ref.stop_reason, s_ref.num_iterations)
    assert np.array_equal(log[:, 7], log_ref[:, 7])
    assert abs(s.initial_cost - s_ref.initial_cost) < 1e-11 * s_ref.initial_cost
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert _block_rel(got, ref, prob["C"]) < 1e-6
    # and it is a different problem from Huber with the same parameter
    _, s_h, _ = capi.solve_points(prob, capi.default_options(huber_delta=2.0))
    assert abs(s_h.final_cost - s.final_cost) > 1e-3 * s.final_cost


# ------------------------------------------------------------------ BASELINE.json configs[2] at full size
def test_config3_full_size_properties():
    """64 cameras x 100k points x 2M observations, the configuration the metric is quoted on.  The oracle needs ~1 s per
    iteration here (bench.py replays three of them in its cpu_baseline leg: `full_size_parity`), so this test checks
    what does not need it: the cost falls monotonically over accepted steps to the RMS of the synthetic noise
    (0.5 px sigma in both coordinates, 2M x 2 residuals), two solves are bit-identical, the pipelined and the sequential
    schedule agree bit for bit, and solving again from the solution stops at once (idempotence)."""
    prob = syn.make_config("cfg3")
    assert (prob["C"], prob["P"], prob["N"]) == (64, 100_000, 2_000_000)
    problem = capi.Problem.points(prob)
    sv = capi.Solver(problem, capi.default_options())
    s = sv.run()
    log = sv.iterations()
    _, sumsq = sv.final_costs()
    sv.close()
    assert s.termination_type == 0 and 2 <= s.num_iterations <= 6
    costs = log[:, 1]
    assert np.all(np.diff(costs[log[:, 7] >= 2]) < 0)                     # accepted steps only go down
    rms = np.sqrt(sumsq / (2.0 * prob["N"]))
    assert abs(rms - 0.5) < 0.03                                          # the noise floor of the generator
    sv2 = capi.Solver(problem, capi.default_options())
    s2 = sv2.run()
    log2 = sv2.iterations()
    os.environ["RSBA_PIPELINE"] = "0"
    os.environ["RSBA_SEG_TARGET"] = "8"
    try:
        sv3 = capi.Solver(problem, capi.default_options())
        s3 = sv3.run()
        log3 = sv3.iterations()
        sv3.close()
    finally:
        del os.environ["RSBA_PIPELINE"]
        del os.environ["RSBA_SEG_TARGET"]
    assert np.array_equal(log, log2) and s.final_cost == s2.final_cost
    assert np.array_equal(log, log3) and s.final_cost == s3.final_cost
    sv2.download()                                                        # the solution becomes the problem's start
    sv2.close()
    sv4 = capi.Solver(problem, capi.default_options())
    s4 = sv4.run()
    sv4.close()
    assert s4.num_iterations <= 1 and abs(s4.final_cost - s.final_cost) < 1e-6 * s.final_cost
    problem.close()


# ------------------------------------------------------------------ what the multi-GPU path relies on
@pytest.mark.parametrize("huber", [0.0, 1.0])
def test_shard_payloads_add_up_to_the_payload_of_the_whole(huber):
    """Linearity: the payload a rank contributes to the all-reduce (S | g_c | rhs correction | diag U | scalars, and
    max |g_p| for the max-reduce) is a sum over that rank's points, so the payloads of disjoint point shards, computed
    by the same HIP kernels on each shard alone, must add up to the payload of the whole problem — which is all the
    RCCL sum all-reduce assumes.  (The shards come from the generator exactly as bench.py hands them to the ranks.)"""
    C, P, k, seed = 40, 16384, 10, 61
    opts = lambda: capi.default_options(huber_delta=huber)
    whole = syn.make_problem(C, P, k, seed=seed, outlier_frac=0.05 if huber else 0.0)
    full, gmax_full = capi.points_linearize_payload(whole, 1e4, opts())
    parts, gmaxs = [], []
    for lo, hi in [(0, 4096), (4096, 12288), (12288, 16384)]:
        shard = syn.make_problem(C, P, k, seed=seed, point_range=(lo, hi), outlier_frac=0.05 if huber else 0.0)
        pay, gm = capi.points_linearize_payload(shard, 1e4, opts())
        parts.append(pay); gmaxs.append(gm)
    total = parts[0] + parts[1] + parts[2]
    n = 6 * C
    S, Sf = total[:n * n].reshape(n, n), full[:n * n].reshape(n, n)
    assert np.abs(S - Sf).max() < 1e-11 * np.abs(Sf).max()
    vec, vecf = total[n * n:n * n + 3 * n], full[n * n:n * n + 3 * n]
    assert np.abs(vec - vecf).max() < 1e-11 * np.abs(vecf).max()
    sc, scf = total[n * n + 3 * n:], full[n * n + 3 * n:]
    assert np.abs(sc - scf).max() < 1e-11 * max(np.abs(scf).max(), 1.0)
    assert max(gmaxs) == gmax_full


def test_multi_gpu_pipeline_opt_in_single_rank(oracle):
    """RSBA_PIPELINE_MG=1 (the default with a communicator since round 4): the pipelined schedule with RCCL in it — per-stage all-reduces of the row slabs of S
    on a communication stream, the Cholesky gated on the flags published after them and reading its panels from the
    reduced slabs (transposed source), the ranks agreeing on the schedule and on stalls through all-reduces.  One rank
    here (RSBA_FORCE_COMM): the collectives are identities, everything around them runs."""
    prob = syn.make_problem(40, 3000, 9, seed=340)
    ref, s_ref, log_ref = capi.solve_points(prob)
    os.environ["RSBA_FORCE_COMM"] = "1"
    os.environ["RSBA_PIPELINE_MG"] = "1"
    try:
        got, s, log = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_FORCE_COMM"]
        del os.environ["RSBA_PIPELINE_MG"]
    assert s.num_iterations == s_ref.num_iterations and s.stop_reason == s_ref.stop_reason
    assert np.array_equal(log[:, 7], log_ref[:, 7])
    assert _block_rel(got, ref, prob["C"]) < 1e-9 and abs(s.final_cost - s_ref.final_cost) < 1e-12 * s_ref.final_cost


# ------------------------------------------------------------------ marker-chain model at scale
# The time blocks are eliminated on the GPU (ba_marker_schur.hpp); the oracle solves the dense normal equations of all
# blocks.  Same LM sequence, parameters to 1e-6 relative.
def _solve_marker_chain_both(oracle, prob, schur_impl, model=capi.MODEL_MARKER_CHAIN):
    variant = 0 if model == capi.MODEL_MARKER_CHAIN else 1
    ref, s_ref, log = oracle.solve_marker_chain(prob, variant, prob["marker_side"], prob["intr"])
    p = capi.Problem.marker_chain(prob, model)
    s = p.solve(capi.default_options(schur_impl=schur_impl))
    got = p.params.copy()
    p.close()
    return ref, s_ref, got, s


@pytest.mark.parametrize("env", [{}, {"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SOLVE_LDS": "0"}],
                         ids=["default", "valu-accumulate", "one-stream", "k_time_eliminate", "panel-solver"])
@pytest.mark.parametrize("shape", [(4, 40, 6), (8, 120, 12), (3, 300, 4), (12, 40, 20)])
def test_marker_chain_time_elimination_matches_oracle(oracle, shape, env, monkeypatch):
    """The split elimination (csrc/ba_marker_split.hpp, round 6) in its variants — the chunk's sum of W'Y on the matrix cores in the
    wavefronts' registers (up to 144 reduced columns: three tiles a wavefront; up to 240: eight — the (12, 40, 20) shape, 180 columns),
    the VALU accumulation in LDS (wider systems; forced here), the three product kernels on one stream — and round 4's k_time_eliminate; the
    reduced solve with the whole triangle in LDS (up to 160 columns: 48, 108, 30 here; 180 takes the panel solver) or the panel solver forced.
    These are whole solves; one step of every variant is held as a linear solve, to a backward-error bar, in tests/test_gpu_marker_step.py."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    C_, T_, M_ = shape
    prob = syn.make_marker_chain(C_, T_, M_, seed=sum(shape))
    ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 2)
    assert s.num_iterations == s_ref.num_iterations and s.num_successful_steps == s_ref.num_successful_steps
    assert abs(s.initial_cost - s_ref.initial_cost) < 1e-9 * s_ref.initial_cost
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max())
    # the base blocks are not part of the problem
    assert np.all(got[:6] == prob["params"][:6]) and np.all(got[6 * (C_ + T_):6 * (C_ + T_) + 6] == prob["params"][6 * (C_ + T_):6 * (C_ + T_) + 6])


@pytest.mark.parametrize("iters", [3, None])
def test_marker_chain_at_its_benchmarked_size_matches_the_sparse_oracle(oracle, iters):
    """8 cameras x 5000 shots x 16 markers — the size profiles/r0*_marker_chain_scale.json times (~0.5 M residual blocks, 30 000
    unknowns) — against the oracle's block-sparse model with the time blocks eliminated (MarkerChainSparseModel, pinned to the
    dense model and to the reference's XML in tests/test_oracle_golden.py).  Rounds 3-4 compared this size with the ground truth
    only: the dense oracle cannot hold it.  Three forced iterations (every iterate's cost 1e-9, the accept / reject sequence,
    every block 1e-6 relative) and the whole solve with the reference's tolerances (iteration count, stop reason, parameters)."""
    import os as _os
    prob = syn.make_marker_chain(8, 5000, 16, seed=11)
    nt = max(1, min(len(_os.sched_getaffinity(0)), 32))
    kw = dict(max_num_iterations=iters, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0) if iters else {}
    ref, s_ref, log_ref = oracle.solve_marker_chain(prob, 16, prob["marker_side"], prob["intr"], oracle.options(num_threads=nt, **kw))
    p = capi.Problem.marker_chain(prob)
    sv = capi.Solver(p, capi.default_options(**kw))
    s = sv.run()
    sv.download()
    log = sv.iterations()
    got = p.params.copy()
    sv.close()
    p.close()
    assert (s.termination_type, s.stop_reason, s.num_iterations, s.num_successful_steps) == (s_ref.termination, s_ref.stop_reason, s_ref.num_iterations, s_ref.num_successful_steps)
    assert np.array_equal(log[:, 7], log_ref[:, 7])
    assert np.abs(log[:, 1] - log_ref[:, 1]).max() <= 1e-9 * log_ref[:, 1].max()
    assert abs(s.final_cost - s_ref.final_cost) <= 1e-9 * s_ref.final_cost
    a, b = got.reshape(-1, 6), ref.reshape(-1, 6)
    rel = (np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-12)).max()
    assert rel < 1e-6, rel


@pytest.mark.parametrize("chunks", ["1", "7", "1000"])
def test_marker_chain_chunk_count_does_not_change_the_answer(oracle, chunks):
    """RSBA_MT_CHUNKS: how many workgroups share the times of the elimination (one partial system each, summed in chunk order).
    One chunk, a number that does not divide the times, more chunks than times: the oracle's solution each time (whole solves; the
    partial systems' sum itself is held per step in tests/test_gpu_marker_step.py)."""
    prob = syn.make_marker_chain(8, 120, 12, seed=140)
    os.environ["RSBA_MT_CHUNKS"] = chunks
    try:
        ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 2)
    finally:
        del os.environ["RSBA_MT_CHUNKS"]
    assert s.num_iterations == s_ref.num_iterations and s.num_successful_steps == s_ref.num_successful_steps
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("wg", ["0", "1", "split"])
def test_marker_chain_both_back_substitution_kernels_match_the_oracle(oracle, wg, monkeypatch):
    """The shots' back-substitution: round 6's split form (k_mc_time_step from the slots' records + k_mc_candidate, a thread per
    residual block: the default), a workgroup per shot with a corner of a residual block per lane (k_time_backsub_wg, shots of
    at most 128 residual blocks) or a wavefront per shot (k_time_backsub_terms, any width; RSBA_MT_BACKSUB_WG=0 forces it).  All
    against the oracle, on a shape with all cameras x markers in a shot (96 residual blocks) and on one with few (whole solves; one step of
    each kernel is held as a linear solve in tests/test_gpu_marker_step.py)."""
    if wg != "split":
        monkeypatch.setenv("RSBA_MT_SPLIT_BACKSUB", "0")
    os.environ["RSBA_MT_BACKSUB_WG"] = "1" if wg == "split" else wg
    try:
        for shape, seed in (((8, 60, 12), 5), ((3, 200, 4), 9)):
            prob = syn.make_marker_chain(*shape, seed=seed)
            ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 2)
            assert s.num_iterations == s_ref.num_iterations and s.num_successful_steps == s_ref.num_successful_steps, shape
            assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost, shape
            assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max()), shape
    finally:
        del os.environ["RSBA_MT_BACKSUB_WG"]


def test_marker_chain_automatic_choice_and_dense_cross_check(oracle):
    """schur_impl 1 (default) eliminates once the dense system outgrows one workgroup's solver; the one-workgroup dense
    path (schur_impl 0) on the same problem is the on-device cross-check."""
    prob = syn.make_marker_chain(5, 80, 8, seed=77)   # 6 (5 + 80 + 8) = 558 unknowns > 384
    p = capi.Problem.marker_chain(prob)
    s1 = p.solve()
    a = p.params.copy(); p.close()
    p = capi.Problem.marker_chain(prob)
    s0 = p.solve(capi.default_options(schur_impl=0))
    b = p.params.copy(); p.close()
    assert s1.num_iterations == s0.num_iterations
    assert abs(s1.final_cost - s0.final_cost) < 1e-10 * s0.final_cost
    assert np.abs(a - b).max() < 1e-7
    # and the run is bitwise reproducible
    p = capi.Problem.marker_chain(prob)
    p.solve()
    assert np.array_equal(p.params, a)
    p.close()


def test_marker_chain_large_reduced_system(oracle):
    """More than 64 camera + marker blocks: the reduced system goes through the multi-launch Cholesky (a whole solve; the step itself, on both
    sides of the 384-column hand-over, is held in tests/test_gpu_marker_step.py)."""
    prob = syn.make_marker_chain(36, 24, 36, seed=5, keep=0.5)
    assert 6 * (35 + 35) > 384
    ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 1)
    assert s.num_iterations == s_ref.num_iterations
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("seed", range(12))
def test_marker_chain_random_shapes_match_the_oracle(oracle, seed):
    """Twelve seeded random shapes of the marker-chain model through the time elimination (round 6: the split kernels) — cameras, shots,
    markers, visibility and noise drawn as tools/fuzz_marker_chain.py draws them (120 more: profiles/r06_fuzz_marker_chain_120_seed2026.txt)."""
    rng = np.random.default_rng([seed, 0x3C])
    C_, M_, T_ = int(rng.integers(2, 14)), int(rng.integers(2, 22)), int(rng.integers(3, 160))
    prob = syn.make_marker_chain(C_, T_, M_, seed=int(rng.integers(1, 1 << 30)), keep=float(rng.uniform(0.35, 1.0)), noise_px=float(rng.choice([0.05, 0.3, 1.0])))
    ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 2)
    assert (s.num_iterations, s.num_successful_steps) == (s_ref.num_iterations, s_ref.num_successful_steps), (C_, T_, M_)
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost, (C_, T_, M_)
    assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max()), (C_, T_, M_)


def test_marker_chain_times_wider_than_the_split_kernels_hold(oracle):
    """A shot that touches more camera / marker blocks than the split accumulation's double-buffered records fit in LDS (~110 of the 170 the
    model allows): the library takes round 4's k_time_eliminate for it (32 residual blocks staged at a time, whatever the width) — 60 cameras
    x 60 markers all seen in every shot (118 blocks, 3 481 residual blocks a shot: the split kernels with the chunk sums in memory), 62 x 62
    (122 blocks: k_time_eliminate).  Whole solves; one step of both is held as a linear solve in tests/test_gpu_marker_step.py."""
    for C_, T_, M_ in ((60, 5, 60), (62, 4, 62)):
        prob = syn.make_marker_chain(C_, T_, M_, seed=21, keep=1.0)
        ref, s_ref, got, s = _solve_marker_chain_both(oracle, prob, 2)
        assert s.num_iterations == s_ref.num_iterations, (C_, M_)
        assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost, (C_, M_)
        assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max()), (C_, M_)


def test_golden_fixtures_through_time_elimination(oracle, tmp_path):
    """The committed hongo / test2 inputs with schur_impl = 2: same iteration counts and the reference's own outputs."""
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    p = capi.Problem.correspondence(os.path.join(G, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    s = p.solve(capi.default_options(schur_impl=2))
    assert s.termination_type == capi.CONVERGENCE and s.num_iterations == 7 and s.num_successful_steps == 6
    assert abs(s.initial_cost - 138796.696054) < 1e-5 and abs(s.final_cost - 143.629388852) < 1e-7
    xml = str(tmp_path / "Camera_Transform.xml")
    p.write_outputs(xml, None, None)
    got, want = ol.read_opencv_xml(xml), ol.read_opencv_xml(os.path.join(G, "hongo", "Camera_Transform.xml"))
    for k in want:
        assert np.abs(got[k] - want[k]).max() < 1e-9, k
    p.close()
    intr = ol.read_intrinsics(ol.SERIALS_TEST2)
    p = capi.Problem.correspondence(os.path.join(G, "test2", "correspondence_test.txt"), capi.MODEL_MARKER_CHAIN_TEST2, ol.MARKER_SIDE_TEST2, intr)
    s = p.solve(capi.default_options(schur_impl=2))
    xmlv = ol.read_opencv_xml(os.path.join(G, "test2", "Camera_Transform.xml"))
    assert s.num_iterations == 4 and s.stop_reason == 3
    assert np.abs(p.params[6:9] - xmlv["R1"].ravel()).max() < 1e-9
    assert np.abs(p.params[9:12] - xmlv["t1"].ravel()).max() < 1e-9
    p.close()


# ------------------------------------------------------------------ constant camera blocks
@pytest.mark.parametrize("shape,const,impl", [((8, 2000, 6), (0,), 1), ((24, 3000, 8), (0, 17), 1), ((8, 1500, 6), (3,), 0),
                                              ((70, 1500, 10), (0, 69), 1), ((40, 20000, 8), (0, 21), 1),
                                              # (a constant camera in the reduced system's BORDER — the last camera group, ba_cholesky_border.hpp — and in its leading part)
                                              ((40, 6000, 8), (3, 37), 1), ((64, 4000, 10), (63,), 1), ((33, 3000, 7), (32,), 1)])
def test_constant_cameras_match_oracle(oracle, shape, const, impl):
    """Problem::SetParameterBlockConstant on camera blocks: the cameras keep their bits, the rest follows the oracle's
    trajectory (Jacobian columns dropped, norms without the constant blocks).  (40 cameras x 20k points: every pair tile has
    reducer workgroups, one per 3 x 3 quadrant of its blocks — they zero a constant camera's blocks themselves.)"""
    C_, P_, k_ = shape
    prob = syn.make_problem(C_, P_, k_, seed=C_ + P_)
    ref, s_ref, _ = oracle.solve_points_constant(prob, const)
    p = capi.Problem.points(prob)
    for c in const:
        p.set_camera_constant(c)
    s = p.solve(capi.default_options(schur_impl=impl))
    got = p.params.copy()
    p.close()
    assert s.num_iterations == s_ref.num_iterations and s.num_successful_steps == s_ref.num_successful_steps
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    for c in const:
        assert np.array_equal(got[6 * c:6 * c + 6], prob["params"][6 * c:6 * c + 6])
    assert np.abs(got - ref).max() < 1e-6 * max(1.0, np.abs(ref).max())
    # and it is a different problem from the free one
    free, s_free, _ = oracle.solve_points(prob)
    assert np.abs(free[:6 * C_] - ref[:6 * C_]).max() > 1e-6


@pytest.mark.parametrize("shape,const_cams,huber", [((8, 3000, 6), (), 0.0), ((40, 6000, 8), (3,), 0.0), ((64, 5000, 12), (), 1.5), ((96, 2500, 10), (95,), 0.0)])
def test_constant_points_match_oracle(oracle, shape, const_cams, huber):
    """Problem::SetParameterBlockConstant on POINT blocks (round 6; rsba_problem_set_point_constant), alone and together with constant
    cameras, through every schedule: one workgroup (8 cameras), pipelined + border (40, 64), sparse pair segments + tiled factorisation
    (96), with and without a robust loss.  A constant point keeps its bits, is not eliminated, its observations still pull on their
    cameras; the oracle drops its Jacobian columns and leaves it out of the norms (oracle_solve_points_constant_blocks, itself held to the
    numpy replay's constant_blocks fixture)."""
    C_, P_, k_ = shape
    prob = syn.make_problem(C_, P_, k_, seed=C_ + P_ + 1, outlier_frac=0.05 if huber else 0.0)
    rng = np.random.default_rng(C_)
    const_pts = sorted(int(j) for j in rng.choice(P_, size=P_ // 20, replace=False))
    ref, s_ref, log_ref = oracle.solve_points_constant_blocks(prob, const_cams, const_pts, oracle.options(huber_delta=huber))
    p = capi.Problem.points(prob)
    for c in const_cams:
        p.set_camera_constant(c)
    for j in const_pts:
        p.set_point_constant(j)
    sv = capi.Solver(p, capi.default_options(huber_delta=huber))
    try:
        s = sv.run()
        sv.download()
        log, got = sv.iterations(), p.params.copy()
        report = sv.full_report()
    finally:
        sv.close()
        p.close()
    assert s.num_iterations == s_ref.num_iterations and np.array_equal(log[:, 7], log_ref[:, 7])
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    assert np.abs(log[:, 1] - log_ref[:, 1]).max() < 1e-9 * log_ref[:, 1].max()
    for j in const_pts:
        assert np.array_equal(got[6 * C_ + 3 * j:6 * C_ + 3 * j + 3], prob["params"][6 * C_ + 3 * j:6 * C_ + 3 * j + 3]), "constant point %d moved" % j
    for c in const_cams:
        assert np.array_equal(got[6 * c:6 * c + 6], prob["params"][6 * c:6 * c + 6])
    assert _block_rel(got, ref, C_) < 1e-6
    # it is a different problem from the free one, and the report counts the reduced program as Ceres does
    free, _, _ = oracle.solve_points(prob, oracle.options(huber_delta=huber))
    assert np.abs(free - ref).max() > 1e-6
    assert str(C_ + P_ - len(const_cams) - len(const_pts)) in report


def test_constant_camera_is_refused_for_the_marker_chain_model():
    """rsba_problem_set_camera_constant is the point model's call; the marker-chain models take
    rsba_problem_set_parameter_block_constant (below)."""
    prob = syn.make_marker_chain(3, 10, 4, seed=2)
    p = capi.Problem.marker_chain(prob)
    with pytest.raises(capi.RsbaError):
        p.set_camera_constant(1)
    p.close()


def test_constant_blocks_of_the_marker_chain_model_match_oracle(oracle):
    """rsba_problem_set_parameter_block_constant on the committed hongo input (camera 2, time 3, marker 5: one block of every kind) and
    on a synthetic rig large enough that the time-eliminating path would be chosen — constant blocks select the dense path.  The oracle's
    constant handling is itself held to the numpy replay (tests/test_oracle_golden.py)."""
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    prob = ol.read_correspondence(os.path.join(G, "hongo", "correspondence.txt"))
    Cn, Tn = prob["C"], prob["T"]
    const = [2, Cn + 3, Cn + Tn + 5]
    ref, s_ref, _ = oracle.solve_marker_chain_constant(prob, 0, ol.MARKER_SIDE_MAIN, intr, const)
    p = capi.Problem.correspondence(os.path.join(G, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    for b in const:
        p.set_parameter_block_constant(6 * b)
    with pytest.raises(capi.RsbaError):
        p.set_parameter_block_constant(6 * 2 + 1)   # not the start of a block
    s = p.solve()
    got = p.params.copy()
    p.close()
    assert s.num_iterations == s_ref.num_iterations and abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    for b in const:
        assert np.array_equal(got[6 * b:6 * b + 6], prob["params"][6 * b:6 * b + 6])
    assert np.abs(got - ref).max() < 1e-7 * max(1.0, np.abs(ref).max())
    # a rig with 72 + blocks (more than 384 parameters: the time elimination would be the automatic choice)
    rig = syn.make_marker_chain(4, 60, 8, seed=5)
    const2 = [1, rig["C"] + 7, rig["C"] + rig["T"] + 3]
    ref2, s2_ref, _ = oracle.solve_marker_chain_constant(rig, 0, rig["marker_side"], rig["intr"], const2)
    p2 = capi.Problem.marker_chain(rig)
    for b in const2:
        p2.set_parameter_block_constant(6 * b)
    s2 = p2.solve()
    got2 = p2.params.copy()
    p2.close()
    assert s2.num_iterations == s2_ref.num_iterations and abs(s2.final_cost - s2_ref.final_cost) < 1e-9 * max(s2_ref.final_cost, 1e-12)
    for b in const2:
        assert np.array_equal(got2[6 * b:6 * b + 6], rig["params"][6 * b:6 * b + 6])
    assert np.abs(got2 - ref2).max() < 1e-6 * max(1.0, np.abs(ref2).max())


def test_full_report_of_the_committed_problem():
    """Summary::FullReport() (bundle_adjustment_manager.cpp:95): sizes of the reduced program as Ceres counts them (camera 0
    and marker 0 never enter the problem: 19 blocks / 114 parameters, 68 residual blocks / 544 residuals), Ceres' step
    counts (iteration 0 counts as a successful step) and its termination message."""
    intr = ol.read_intrinsics(ol.SERIALS_MAIN)
    p = capi.Problem.correspondence(os.path.join(G, "hongo", "correspondence.txt"), capi.MODEL_MARKER_CHAIN, ol.MARKER_SIDE_MAIN, intr)
    sv = capi.Solver(p)
    with pytest.raises(capi.RsbaError):
        sv.full_report()          # nothing has run yet
    sv.run()
    rep = sv.full_report()
    sv.close(); p.close()
    lines = {ln[:25].strip(): ln.split() for ln in rep.splitlines() if ln.strip()}
    assert lines["Parameter blocks"][-2:] == ["19", "19"] and lines["Parameters"][-2:] == ["114", "114"]
    assert lines["Residual blocks"][-2:] == ["68", "68"] and lines["Residuals"][-2:] == ["544", "544"]
    assert lines["Linear solver"][-2:] == ["DENSE_SCHUR", "DENSE_SCHUR"]
    assert lines["Minimizer iterations"][-1] == "7" and lines["Successful steps"][-1] == "7" and lines["Unsuccessful steps"][-1] == "0"
    assert abs(float(lines["Initial"][-1]) - 1.387967e5) < 1 and abs(float(lines["Final"][-1]) - 1.436294e2) < 1e-3
    assert "CONVERGENCE (Function tolerance reached. |cost_change|/cost:" in rep and "gfx950" in rep


# ------------------------------------------------------------------ reduced system on several workgroups
@pytest.mark.parametrize("C,P,k", [(32, 2400, 8), (37, 2600, 9), (48, 3000, 10), (64, 3600, 12)])
def test_multi_workgroup_cholesky_matches_oracle_and_single_workgroup(oracle, C, P, k):
    """32 to 64 cameras (37: a padded last panel): the reduced system is factored by four workgroups handing the diagonal
    factors to each other (ba_cholesky_multi.hpp).  Oracle parity, bitwise reproducibility, the same answer (to rounding) from 1, 2, 3 and 6
    workgroups, and from the sequential schedule bit for bit."""
    prob = syn.make_problem(C, P, k, seed=500 + C)
    got, s, log, _ = _compare_solve(oracle, prob, 1)
    again, s2, log2 = capi.solve_points(prob)
    assert np.array_equal(got, again) and np.array_equal(log, log2)
    for g in ("1", "2", "3", "6"):
        os.environ["RSBA_CHOL_WGS"] = g
        try:
            other, so, _ = capi.solve_points(prob)
        finally:
            del os.environ["RSBA_CHOL_WGS"]
        assert so.num_iterations == s.num_iterations
        assert np.abs(other - got).max() < 1e-9 * max(1.0, np.abs(got).max()), g
    os.environ["RSBA_PIPELINE"] = "0"
    os.environ["RSBA_SEG_TARGET"] = "8"
    try:
        seq, s_seq, log_seq = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_PIPELINE"]
        del os.environ["RSBA_SEG_TARGET"]
    assert np.array_equal(got, seq) and np.array_equal(log, log_seq)


def test_multi_workgroup_cholesky_stall_falls_back(oracle, capfd):
    """The gates of the four-workgroup factorisation never open (RSBA_TEST_STALL=1): every workgroup gives up inside its
    budget, the step is repeated with the sequential schedule, the result does not change."""
    prob = syn.make_problem(32, 2000, 8, seed=91)
    ref, s_ref, log_ref = capi.solve_points(prob)
    os.environ["RSBA_TEST_STALL"] = "1"
    try:
        got, s, log = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_TEST_STALL"]
    assert "falling back" in capfd.readouterr().err
    assert np.array_equal(got, ref) and np.array_equal(log, log_ref)


def test_tiled_cholesky_stall_falls_back_to_the_multi_launch_factorisation(oracle, capfd):
    """RSBA_TEST_STALL=3: a diagonal tile of the persistent tiled factorisation looks for its hand-over in the set nobody
    writes this launch (the data is its own flag there: nothing ever arrives).  It must give up inside its budget, every
    other workgroup with it, the step must be repeated with the multi-launch factorisation — for the rest of the solve — and the
    result must be the one of the multi-launch factorisation (same arithmetic per entry in both: identical bits are not
    promised between them, the parity bar is)."""
    prob = syn.make_problem(130, 1500, 12, seed=430)
    ref, s_ref, log_ref = oracle.solve_points(prob)
    os.environ["RSBA_TEST_STALL"] = "3"
    try:
        got, s, log = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_TEST_STALL"]
    err = capfd.readouterr().err
    assert err.count("persistent tiled Cholesky stalled") == 1, err
    assert s.num_iterations == s_ref.num_iterations and np.array_equal(log[:, 7], log_ref[:, 7])
    assert abs(s.final_cost - s_ref.final_cost) < 1e-9 * s_ref.final_cost
    C = prob["C"]
    for a, b in ((got[:6 * C].reshape(-1, 6), ref[:6 * C].reshape(-1, 6)), (got[6 * C:].reshape(-1, 3), ref[6 * C:].reshape(-1, 3))):
        assert (np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-12)).max() < 1e-6


# ------------------------------------------------------------------ persistent tiled Cholesky (more than 64 cameras)
@pytest.mark.parametrize("C,P,k", [(65, 1400, 9), (100, 2200, 10), (128, 2600, 10)])
def test_persistent_tiled_cholesky_matches_oracle_and_multi_launch(oracle, C, P, k):
    """More than 64 cameras: one resident workgroup per 64 x 64 tile of the reduced system, chained by flags
    (ba_cholesky_tiles.hpp).  C = 65: a padded last panel; C = 100: an odd number of panels (the last tile column holds one);
    C = 128: whole tiles, the right-hand side row alone in its tile row.  Oracle parity, the multi-launch factorisation
    (RSBA_CHOL_TILES=0) to rounding, bitwise reproducibility."""
    prob = syn.make_problem(C, P, k, seed=900 + C)
    got, s, log, _ = _compare_solve(oracle, prob, 1)
    again, s2, log2 = capi.solve_points(prob)
    assert np.array_equal(got, again) and np.array_equal(log, log2)
    os.environ["RSBA_CHOL_TILES"] = "0"
    try:
        other, so, _ = capi.solve_points(prob)
    finally:
        del os.environ["RSBA_CHOL_TILES"]
    assert so.num_iterations == s.num_iterations
    assert np.abs(other - got).max() < 1e-9 * max(1.0, np.abs(got).max())
