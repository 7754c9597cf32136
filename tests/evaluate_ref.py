"""numpy reference of ceres::Problem::Evaluate without the Jacobian (rsba_solver_evaluate): residuals in the problem's observation
order, the squared norm s of every residual block, the cost 1/2 sum rho(s) and the gradient J'r in the problem's parameter layout.

Rows come from the oracle's per-observation functions (oracle_point_residual_jacobian / oracle_marker_residual_jacobian, pinned to
the reference's committed outputs), as tests/covariance_ref.py takes J; the loss is marker_loss_ref.rho_and_rho1.  With a loss
applied a block's residuals and Jacobian rows are scaled by sqrt(rho'(s)) (Ceres' corrector for rho'' <= 0), so the gradient is
rho'(s) J'r per block.  Gradient slots of constant blocks, of blocks no residual references and of the fixed base blocks of the
marker-chain models are 0.0, as ProgramEvaluator leaves such blocks out.

Besides the values, `finish` returns what a rounding bound on a gradient entry needs: sum_i |J_ik|, sum_i |J_ik r_i| and the number
of terms n_k of every slot k (corrected rows)."""
from types import SimpleNamespace

import numpy as np

import marker_loss_ref as mlr


def point_rows(oracle, prob, params):
    """Raw rows of the point model at params -> list of (r (2,), [(offset, J (2 x size)), ...]) per observation."""
    C = prob["C"]
    intr = np.asarray(prob["intr"], float).reshape(-1, 4)
    obs = np.asarray(prob["obs"], float).reshape(-1, 2)
    rows = []
    for i in range(prob["N"]):
        c, p = int(prob["cam_idx"][i]), int(prob["pt_idx"][i])
        r, jc, jp = oracle.point_residual_jacobian(params[6 * c:6 * c + 6], params[6 * C + 3 * p:6 * C + 3 * p + 3], intr[c], obs[i])
        rows.append((r, [(6 * c, jc), (6 * C + 3 * p, jp)]))
    return rows


def marker_rows(oracle, prob, params, variant):
    """Raw rows of the marker-chain models.  variant 0: camera 0 and marker 0 are the fixed base blocks (no parameters of any
    residual); 1 (Test2): camera 0 only."""
    C, T = prob["C"], prob["T"]
    intr = np.asarray(prob["intr"], float).reshape(-1, 4)
    obs = np.asarray(prob["obs"], float).reshape(-1, 8)
    rows = []
    for i in range(prob["N"]):
        c, t, m = int(prob["c"][i]), int(prob["t"][i]), int(prob["m"][i])
        cb, tb, mb = c, C + t, C + T + m
        cam = params[6 * cb:6 * cb + 6] if c != 0 else None
        mar = params[6 * mb:6 * mb + 6] if (variant == 1 or m != 0) else None
        r, j = oracle.marker_residual_jacobian(cam, params[6 * tb:6 * tb + 6], mar, prob["marker_side"], intr[c], obs[i])
        blocks = [(6 * tb, j[:, 6:12])]
        if cam is not None:
            blocks.append((6 * cb, j[:, 0:6]))
        if mar is not None:
            blocks.append((6 * mb, j[:, 12:18]))
        rows.append((r, blocks))
    return rows


def finish(rows, num_parameters, constant_offsets=(), loss="none", a=0.0, apply_loss=True):
    """rows -> residuals, s, cost, gradient (+ abs_J, abs_Jr, n_terms per slot, `live` mask of the slots that are computed).
    constant_offsets: (offset, size) of the constant blocks."""
    N = len(rows)
    d = len(rows[0][0]) if N else 0
    raw = np.array([r for r, _ in rows], float).reshape(N, d)
    s = np.sum(raw * raw, axis=1)
    if apply_loss:
        rho, rho1 = mlr.rho_and_rho1(s, loss, a)
    else:
        rho, rho1 = s, np.ones_like(s)
    sq = np.sqrt(rho1)
    res = raw * sq[:, None]
    g, abs_J, abs_Jr = np.zeros(num_parameters), np.zeros(num_parameters), np.zeros(num_parameters)
    n_terms = np.zeros(num_parameters, np.int64)
    live = np.zeros(num_parameters, bool)
    for i, (_, blocks) in enumerate(rows):
        for off, J in blocks:
            Jt = sq[i] * J
            sl = slice(off, off + J.shape[1])
            g[sl] += Jt.T @ res[i]
            abs_J[sl] += np.abs(Jt).sum(0)
            abs_Jr[sl] += (np.abs(Jt) * np.abs(res[i])[:, None]).sum(0)
            n_terms[sl] += d
            live[sl] = True
    for off, size in constant_offsets:
        live[off:off + size] = False
    g[~live] = 0.0
    return SimpleNamespace(residuals=res.reshape(-1), raw=raw.reshape(-1), s=s, cost=0.5 * float(np.sum(rho)), gradient=g, abs_J=abs_J,
                           abs_Jr=abs_Jr, n_terms=n_terms, live=live)


def point_constant_offsets(prob, constant_cameras=(), constant_points=()):
    return [(6 * c, 6) for c in constant_cameras] + [(6 * prob["C"] + 3 * p, 3) for p in constant_points]


def point_evaluate(oracle, prob, params, constant_cameras=(), constant_points=(), loss="none", a=0.0, apply_loss=True):
    return finish(point_rows(oracle, prob, params), len(params), point_constant_offsets(prob, constant_cameras, constant_points), loss, a,
                  apply_loss)


def marker_evaluate(oracle, prob, params, variant, constant_blocks=(), loss="none", a=0.0, apply_loss=True):
    return finish(marker_rows(oracle, prob, params, variant), len(params), [(6 * b, 6) for b in constant_blocks], loss, a, apply_loss)
