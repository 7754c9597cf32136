"""Pins of tests/marker_loss_ref.py, the numpy reference the marker-chain robust-loss tests hold the HIP path to.

  * with no loss it reproduces the reference's committed hongo and test2 Camera_Transform.xml (the replay's bar, 1e-12);
  * with Huber and Cauchy on hongo its trajectory agrees with tools/replay_point_model's complex-step DENSE Jacobian put through
    the corrector here (the replay itself applies no loss to this model) to 1e-12 relative;
  * the committed fixture regenerates bit for bit from tools/marker_chain_loss_fixture.py.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import marker_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("which,variant,iterations,final_cost", [("hongo", 0, 7, 143.629388852), ("test2", 1, 4, 13.301709)])
def test_no_loss_reproduces_the_references_xml(which, variant, iterations, final_cost):
    rp = _tool("replay_point_model")
    prob = ref.hongo() if which == "hongo" else ref.test2()
    mc = ref.MarkerChain(prob, variant)
    x, summary, rows = ref.minimise(mc)
    assert (len(rows) - 1, summary["termination"], summary["reason"]) == (iterations, "CONVERGENCE", "function")
    assert abs(summary["final_cost"] - final_cost) < 1e-6
    blocks = mc.full(x)
    xml = rp.read_xml_matrices(os.path.join(ref.GOLDEN, which, "Camera_Transform.xml"))
    for c in range(prob["C"]):
        R = xml["R%d" % c]
        got = rp.rodrigues(blocks[c, :3]) if R.shape == (3, 3) else blocks[c, :3].reshape(3, 1)
        assert np.abs(got - R).max() < 1e-12 and np.abs(blocks[c, 3:] - xml["t%d" % c][:, 0]).max() < 1e-12


@pytest.mark.parametrize("loss,a", [("huber", 2.0), ("cauchy", 2.0)])
def test_loss_agrees_with_the_replays_dense_jacobian(loss, a):
    """The replay's minimise driven by its own marker-chain residuals and a dense complex-step J, corrected per 8-residual block."""
    rp = _tool("replay_point_model")
    prob = ref.displace_corners(ref.hongo(), 0.05, 30.0, 7)
    rprob = rp.mc_problem(os.path.join(ref.GOLDEN, "hongo", "correspondence.txt"), ref.HONGO_SERIALS, ref.HONGO_SIDE, False)
    rprob["obs"] = prob["obs"].copy()
    rprob["loss"], rprob["loss_scale"] = loss, a

    def evaluate(x, p, with_jacobian):
        r = rp.mc_residuals(x.astype(complex), p).real
        s = np.sum(r.reshape(-1, 8) ** 2, axis=1)
        rho, rho1 = rp.loss(p, s)
        cost = 0.5 * float(np.sum(rho))
        if not with_jacobian:
            return cost, None, None, float(np.sum(s))
        _, _, J, _ = rp.mc_evaluate(x, p, True)
        sq = np.repeat(np.sqrt(rho1), 8)
        return cost, r * sq, J * sq[:, None], float(np.sum(s))

    rp.evaluate = evaluate   # (this module instance only: the tool on disk is untouched)
    xr, sr, rows_r = rp.minimise(rprob)
    mc = ref.MarkerChain(prob, 0, loss, a)
    x, s, rows = ref.minimise(mc)
    assert [(rw["valid"], rw["successful"]) for rw in rows] == [(rw["valid"], rw["successful"]) for rw in rows_r]
    assert (s["termination"], s["reason"]) == (sr["termination"], sr["reason"])
    assert any(rw["valid"] and not rw["successful"] for rw in rows) or len(rows) > 5
    for rw, rr in zip(rows, rows_r):
        assert abs(rw["cost"] - rr["cost"]) <= 1e-12 * rr["cost"], (rw["iteration"], rw["cost"], rr["cost"])
        assert abs(rw["gradient_max_norm"] - rr["gradient_max_norm"]) <= 1e-9 * rr["gradient_max_norm"]
    assert np.abs(x - xr).max() <= 1e-9 * np.abs(xr).max()
    # the loss is doing something: the loss-free trajectory differs
    _, s0, _ = ref.minimise(ref.MarkerChain(prob, 0))
    assert abs(s0["final_cost"] - s["final_cost"]) > 1.0


def test_corrected_normal_equations_match_a_dense_jacobian():
    """H = J~'J~ and g = J~'r~ scattered by blocks equal the dense products (a Test2 rig with a constant block and Cauchy)."""
    prob = ref.displace_corners(ref.test2(), 0.1, 20.0, 3)
    mc = ref.MarkerChain(prob, 1, "cauchy", 1.5, constant_blocks=(prob["C"] + 1,))
    x = mc.x0()
    cost, rt, Jt, H, g, _ = mc.linearise(x)
    Jd = np.zeros((8 * mc.N, mc.n))
    for k in range(mc.N):
        for q in range(18):
            if mc.cols[k, q] >= 0:
                Jd[8 * k:8 * k + 8, mc.cols[k, q]] += Jt[k, :, q]
    assert np.abs(H - Jd.T @ Jd).max() <= 1e-12 * np.abs(H).max()
    assert np.abs(g - Jd.T @ rt.ravel()).max() <= 1e-12 * np.abs(g).max()
    # complex-step J against central differences of the residuals, one column
    full = mc.full(x)
    J = mc.jacobians(full)
    k = np.flatnonzero(mc.cols[:, 7] >= 0)[0]
    e = 1e-6
    fp, fm = full.copy(), full.copy()
    b = prob["C"] + prob["t"][k]
    fp[b, 1] += e
    fm[b, 1] -= e
    fd = (mc.residuals(fp)[k] - mc.residuals(fm)[k]) / (2 * e)
    assert np.abs(fd - J[k, :, 7]).max() <= 1e-5 * np.abs(J[k, :, 7]).max()


def test_fixture_regenerates_bit_identically():
    fx = _tool("marker_chain_loss_fixture")
    committed = open(fx.OUT).read()
    assert fx.build() == committed
    d = json.loads(committed)
    rows = d["expected"]["iterations"]
    assert d["loss"] == "huber" and d["loss_scale"] == 2.0
    # about 5 % of the corners moved
    moved = np.abs(np.array(d["obs"]) - ref.hongo()["obs"].ravel()).reshape(-1, 2).max(axis=1) > 1.0
    assert 0.02 < moved.mean() < 0.1
    assert d["expected"]["summary"]["termination"] == "CONVERGENCE" and len(rows) > 8
