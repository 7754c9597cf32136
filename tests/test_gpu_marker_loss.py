"""A robust loss (ceres::HuberLoss / CauchyLoss) on the marker-chain models, through the C ABI, against tests/marker_loss_ref.py.

The residual block is one observation (8 residuals); the corrector scales its rows by sqrt(rho'(s)).  Bars (BASELINE's): the same
accept / reject sequence and termination, every iterate's cost to 1e-9 relative, every parameter block to 1e-6 relative, the final
RMS (a plain metric, no loss) to 1e-4 px.  Both paths: the dense one (schur_impl 0) and the time-eliminating one (schur_impl 2) under
every switch test_gpu_parity varies for it.
"""
import json
import os

import numpy as np
import pytest

import marker_loss_ref as ref
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ref.GOLDEN, "marker_chain_hongo_huber_outliers.json")
REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(schur_impl, loss, a, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=a if loss != "none" else 0.0, loss_type=1 if loss == "cauchy" else 0, **kw)


def _solve(prob, model, schur_impl, loss, a, constant_blocks=()):
    pr = capi.Problem.marker_chain(prob, model)
    try:
        for b in constant_blocks:
            pr.set_parameter_block_constant(6 * b)
        s = capi.Solver(pr, _options(schur_impl, loss, a))
        try:
            summ = s.run()
            s.download()
            log = s.iterations()
        finally:
            s.close()
        params = pr.params.copy()
        _, rms = pr.reprojection_error()
    finally:
        pr.close()
    return summ, log, params, rms


_REF = {}


def _reference(key, mc):
    """The reference's trajectory, once per problem (the switch variants share it)."""
    if key is None or key not in _REF:
        x, summary, rows = ref.minimise(mc)
        out = (summary, rows, mc.full(x))
        if key is None:
            return out
        _REF[key] = out
    return _REF[key]


def _check(prob, model, schur_impl, loss, a, constant_blocks=(), expected=None, key=None):
    variant = 1 if model == capi.MODEL_MARKER_CHAIN_TEST2 else 0
    mc = ref.MarkerChain(prob, variant, loss, a, constant_blocks)
    if expected is None:
        summary, rows, final = _reference(key, mc)
    else:
        summary, rows, final = expected["summary"], expected["iterations"], np.array(expected["final_params"]).reshape(-1, 6)
    summ, log, params, rms = _solve(prob, model, schur_impl, loss, a, constant_blocks)
    assert (summ.termination_type, summ.stop_reason, summ.num_iterations) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1)
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    got = params.reshape(-1, 6)
    free = mc.free_blocks
    err = np.abs(got[free] - final[free]).max(axis=1) / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
    assert err.max() < 1e-6, "final parameters differ from the reference's by %.2e relative per block" % err.max()
    fixed = np.setdiff1d(np.arange(got.shape[0]), free)
    np.testing.assert_array_equal(got[fixed], np.asarray(prob["params"]).reshape(-1, 6)[fixed])
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * prob["N"]))
    assert abs(rms - rms_ref) <= 1e-4, (rms, rms_ref)
    return rows


def _fixture():
    d = json.load(open(FIXTURE))
    prob = dict(T=d["T"], C=d["C"], M=d["M"], N=d["N"], t=np.array(d["t"], np.int32), c=np.array(d["c"], np.int32), m=np.array(d["m"], np.int32),
                obs=np.array(d["obs"]).reshape(-1, 8), params=np.array(d["params"]), intr=np.array(d["intr"]).reshape(-1, 4), marker_side=d["marker_side"])
    return d, prob


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_hongo_huber_fixture(schur_impl):
    """The committed fixture (hongo, 5 % of its corners 30 px off, Huber 2 px), on the dense path and with the time blocks eliminated.
    Without the loss the trajectory is the loss-free one."""
    d, prob = _fixture()
    _check(prob, capi.MODEL_MARKER_CHAIN, schur_impl, d["loss"], d["loss_scale"], expected=d["expected"])


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_hongo_cauchy(schur_impl):
    prob = ref.displace_corners(ref.hongo(), 0.05, 30.0, 11)
    _check(prob, capi.MODEL_MARKER_CHAIN, schur_impl, "cauchy", 2.0, key="hongo_cauchy")


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_test2_huber(schur_impl):
    prob = ref.displace_corners(ref.test2(), 0.05, 25.0, 12)
    _check(prob, capi.MODEL_MARKER_CHAIN_TEST2, schur_impl, "huber", 1.5, key="test2_huber")


def _rig(shape):
    C, T, M = shape
    return ref.displace_corners(syn.make_marker_chain(C, T, M, seed=40 + C + T + M), 0.05, 40.0, C * T * M)


# the switches test_marker_chain_time_elimination_matches_oracle varies (with a loss RSBA_MT_SPLIT=0 keeps the split elimination: round 4's
# k_time_eliminate has no block-wide s to weigh a row with)
SWITCHES = [{}, {"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SOLVE_LDS": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
@pytest.mark.parametrize("shape", [(4, 40, 6), (12, 40, 20), (8, 400, 16)], ids=lambda s: "x".join(map(str, s)))
def test_synthetic_rigs_time_eliminated(shape, loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(_rig(shape), capi.MODEL_MARKER_CHAIN, 2, loss, 2.0, key=(shape, loss))


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_synthetic_rig_dense(loss):
    _check(_rig((12, 40, 20)), capi.MODEL_MARKER_CHAIN, 0, loss, 2.0, key=((12, 40, 20), loss))


# the three back-substitutions, selected as test_marker_chain_both_back_substitution_kernels_match_the_oracle selects them (with a loss
# RSBA_MT_BACKSUB_WG is not taken: a corner per lane has no block-wide s; the wavefront-per-time kernel runs instead)
@pytest.mark.parametrize("env", [{}, {"RSBA_MT_SPLIT_BACKSUB": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "0"}],
                         ids=["split", "wg", "terms"])
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_back_substitutions(loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(_rig((4, 40, 6)), capi.MODEL_MARKER_CHAIN, 2, loss, 2.0, key=((4, 40, 6), loss))


def test_constant_blocks_with_a_loss():
    prob = ref.displace_corners(syn.make_marker_chain(4, 30, 6, seed=31), 0.05, 40.0, 31)
    C, T = prob["C"], prob["T"]
    const = (2, C + 5, C + T + 3)
    for model in (capi.MODEL_MARKER_CHAIN, capi.MODEL_MARKER_CHAIN_TEST2):
        _check(prob, model, 0, "huber", 2.0, constant_blocks=const)


@pytest.mark.parametrize("schur_impl,shape", [(0, (6, 40, 9)), (2, (8, 5000, 16))], ids=["dense", "eliminated_8x5000x16"])
def test_a_loss_no_block_reaches_adds_the_same_bits(schur_impl, shape):
    """Huber with a beyond every block's |r|: the loss instances must produce the loss-free run bit for bit (at the benchmarked size too,
    where test_gpu_parity holds the loss-free run to the sparse oracle)."""
    prob = syn.make_marker_chain(*shape, seed=34)
    a = 1e6
    s0, log0, x0, rms0 = _solve(prob, capi.MODEL_MARKER_CHAIN, schur_impl, "none", 0.0)
    s1, log1, x1, rms1 = _solve(prob, capi.MODEL_MARKER_CHAIN, schur_impl, "huber", a)
    assert log0.shape[0] > 2
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_repeated_runs_are_bit_identical(schur_impl):
    d, prob = _fixture()
    pr = capi.Problem.marker_chain(prob, capi.MODEL_MARKER_CHAIN)
    s = capi.Solver(pr, _options(schur_impl, "huber", 2.0))
    try:
        runs = []
        for _ in range(2):
            s.run()
            s.download()
            runs.append((s.iterations(), pr.params.copy()))
        np.testing.assert_array_equal(runs[0][0], runs[1][0])
        np.testing.assert_array_equal(runs[0][1], runs[1][1])
    finally:
        s.close()
        pr.close()


def _covariance_check(prob, model, loss, a, blocks, schur_impl=0):
    """Solve, then (J~'J~)^-1 at the solved parameters against the reference's, to 1e-8 of each block's largest entry."""
    variant = 1 if model == capi.MODEL_MARKER_CHAIN_TEST2 else 0
    pr = capi.Problem.marker_chain(prob, model)
    s = capi.Solver(pr, _options(schur_impl, loss, a, max_num_iterations=20))
    try:
        s.run()
        s.download()
        s.covariance_compute()
        x = pr.params.copy()
        mc = ref.MarkerChain(dict(prob, params=x), variant, loss, a)
        cov, free = ref.covariance(mc, mc.x0())
        at = {b: 6 * i for i, b in enumerate(free)}
        for p in blocks:
            for q in blocks:
                got = s.covariance_block(6 * p, 6 * q)
                want = cov[at[p]:at[p] + 6, at[q]:at[q] + 6]
                assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), (p, q)
        # apply_loss_function = 0: the loss-free covariance at the same parameters.  Not bit for bit: k_cov_mc_lin adds its products into the
        # system with fp64 atomics, in an order that differs from launch to launch (two loss-free computes differ alike), so to rounding, at
        # the bar test_gpu_covariance holds the dense and time-eliminating paths to
        s.covariance_compute(apply_loss_function=0)
        plain = [s.covariance_block(6 * p, 6 * q) for p in blocks for q in blocks]
    finally:
        s.close()
        pr.close()
    pr0 = capi.Problem.marker_chain(dict(prob, params=x), model)
    s0 = capi.Solver(pr0, _options(schur_impl, "none", 0.0))
    try:
        s0.covariance_compute()
        for k, (p, q) in enumerate((p, q) for p in blocks for q in blocks):
            want = s0.covariance_block(6 * p, 6 * q)
            assert np.abs(plain[k] - want).max() <= 1e-10 * np.abs(want).max(), (p, q)   # (observed 1.2e-12)
    finally:
        s0.close()
        pr0.close()


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_covariance_hongo_huber(schur_impl):
    d, prob = _fixture()
    C, T = prob["C"], prob["T"]
    _covariance_check(prob, capi.MODEL_MARKER_CHAIN, "huber", 2.0, [1, 2, 3] + [C + T + m for m in range(1, 11)], schur_impl)


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_covariance_rig_cauchy(schur_impl):
    """schur_impl 2: the free time blocks are eliminated inside k_cov_mc_lin, their rows through the corrector too."""
    prob = ref.displace_corners(syn.make_marker_chain(5, 40, 8, seed=35), 0.05, 40.0, 35)
    C, T, M = prob["C"], prob["T"], prob["M"]
    _covariance_check(prob, capi.MODEL_MARKER_CHAIN, "cauchy", 2.0, list(range(1, C)) + [C + T + m for m in range(1, M)], schur_impl)
