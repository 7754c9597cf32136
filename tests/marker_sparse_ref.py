"""A numpy reference for the marker-chain models with the time blocks ELIMINATED, for sizes marker_loss_ref's dense system cannot hold.

It shares no code with the product.  From tests/marker_loss_ref.py it takes the residuals, the complex-step Jacobians and the loss
(MarkerChain); everything below the rows is its own:

  per time t     V_t = J_t'J_t (6 x 6), g_t, W_t = J_t'J_r (6 x n_r, the time's free cameras and markers), from the corrected rows
  reduced        U = J_r'J_r, g_r over the free cameras and markers (every residual block, a constant time's included)
  LM step        Jacobi scale s = 1 / (1 + sqrt(diag H)) over the free parameters, fixed at iteration 0; in scaled coordinates
                 D = clamp(diag) / radius, S = U + D_r - sum_t W_t' (V_t + D_t)^-1 W_t, the reduced solve, back-substitution
                 delta_t = -(V_t + D_t)^-1 (g_t + W_t delta_r)
  constant       no columns, no step, out of the norms and the scale; a constant time is simply not a variable (its rows still
                 feed U and g_r); n_r = 0: every time on its own
  minimiser      marker_loss_ref.minimise's loop (Ceres' LM), step by step the same.
"""
import numpy as np

import marker_loss_ref as ref


class SparseMarkerChain:
    def __init__(self, prob, variant=0, loss="none", a=0.0, constant_blocks=()):
        self.mc = mc = ref.MarkerChain(prob, variant, loss, a, constant_blocks)
        C, T = mc.C, mc.T
        free = mc.free_blocks
        self.time_free = free[(free >= C) & (free < C + T)]                 # free time blocks
        self.red_free = free[(free < C) | (free >= C + T)]                   # free cameras, then markers
        self.nr = 6 * self.red_free.size
        self.nt = self.time_free.size
        nb = C + T + mc.M
        rpos = -np.ones(nb, np.int64)
        rpos[self.red_free] = np.arange(self.red_free.size)
        tpos = -np.ones(nb, np.int64)
        tpos[self.time_free] = np.arange(self.nt)
        self.cam_r = np.where(mc.has_cam, rpos[np.where(mc.has_cam, mc.c, 0)], -1)            # reduced block of each residual's camera
        self.mar_r = np.where(mc.has_mar, rpos[np.where(mc.has_mar, C + T + mc.m, 0)], -1)    # ... marker
        self.tim_f = tpos[C + mc.t]                                                          # free time of each residual (-1: constant)
        # where the free blocks sit in marker_loss_ref's vector x (the free blocks' order)
        at = -np.ones(nb, np.int64)
        at[free] = np.arange(free.size)
        self.x_red = (6 * at[self.red_free][:, None] + np.arange(6)).ravel()
        self.x_tim = (6 * at[self.time_free][:, None] + np.arange(6)).ravel()

    def x0(self):
        return self.mc.x0()

    def linearise(self, x):
        """cost, corrected rows, U (n_r x n_r), g_r, V (nt, 6, 6), g_t (nt, 6), W (nt, 6, n_r), raw sum of squares."""
        mc = self.mc
        full = mc.full(x)
        r = mc.residuals(full)
        J = mc.jacobians(full)
        s = np.sum(r * r, axis=1)
        rho, rho1 = ref.rho_and_rho1(s, mc.loss, mc.a)
        sq = np.sqrt(rho1)
        rt, Jt = r * sq[:, None], J * sq[:, None, None]
        Jc, Jtm, Jm = Jt[:, :, 0:6], Jt[:, :, 6:12], Jt[:, :, 12:18]
        nr, nt = self.nr, self.nt
        nrb = nr // 6
        # reduced blocks: U by (row block, column block) pairs of each residual, into a dump block nrb for the absent / constant ones
        cb = np.where(self.cam_r >= 0, self.cam_r, nrb)
        mb = np.where(self.mar_r >= 0, self.mar_r, nrb)
        U4 = np.zeros((nrb + 1, nrb + 1, 6, 6))
        np.add.at(U4, (cb, cb), np.einsum("kra,krb->kab", Jc, Jc))
        np.add.at(U4, (mb, mb), np.einsum("kra,krb->kab", Jm, Jm))
        Ucm = np.einsum("kra,krb->kab", Jc, Jm)
        np.add.at(U4, (cb, mb), Ucm)
        np.add.at(U4, (mb, cb), np.transpose(Ucm, (0, 2, 1)))
        U = U4[:nrb, :nrb].transpose(0, 2, 1, 3).reshape(nr, nr)
        g4 = np.zeros((nrb + 1, 6))
        np.add.at(g4, cb, np.einsum("kra,kr->ka", Jc, rt))
        np.add.at(g4, mb, np.einsum("kra,kr->ka", Jm, rt))
        g_r = g4[:nrb].ravel()
        # time blocks
        tf = np.where(self.tim_f >= 0, self.tim_f, nt)
        V = np.zeros((nt + 1, 6, 6))
        np.add.at(V, tf, np.einsum("kra,krb->kab", Jtm, Jtm))
        gt = np.zeros((nt + 1, 6))
        np.add.at(gt, tf, np.einsum("kra,kr->ka", Jtm, rt))
        wc = np.einsum("kra,krb->kab", Jtm, Jc)                               # (N, 6, 6): time row, camera column
        wm = np.einsum("kra,krb->kab", Jtm, Jm)
        Wb = np.zeros((nt + 1, nrb + 1, 6, 6))
        np.add.at(Wb, (tf, cb), wc)
        np.add.at(Wb, (tf, mb), wm)
        W = Wb[:nt, :nrb].transpose(0, 2, 1, 3).reshape(nt, 6, nr)
        return 0.5 * float(np.sum(rho)), rt, Jt, U, g_r, V[:nt], gt[:nt], W, float(np.sum(s))

    def gradient(self, lin):
        """The free parameters' gradient (reduced, then times) for the norms."""
        return np.concatenate([lin[4], lin[6].ravel()])

    def diag(self, lin):
        return np.concatenate([np.diag(lin[3]), np.einsum("tii->ti", lin[5]).ravel()])

    def step(self, lin, scale, radius, min_lm_diagonal, max_lm_diagonal):
        """delta in marker_loss_ref's x order (None: a factorisation failed)."""
        _, _, _, U, g_r, V, gt, W, _ = lin
        nr, nt = self.nr, self.nt
        sr, st = scale[:nr], scale[nr:].reshape(nt, 6)
        Us = U * np.outer(sr, sr)
        Ur = Us + np.diag(np.clip(np.diag(Us), min_lm_diagonal, max_lm_diagonal) / radius)
        Vs = V * st[:, :, None] * st[:, None, :]
        dV = np.clip(np.einsum("tii->ti", Vs), min_lm_diagonal, max_lm_diagonal) / radius
        Vd = Vs + dV[:, :, None] * np.eye(6)[None]
        Ws = W * st[:, :, None] * sr[None, None, :]
        bt = st * gt
        try:
            np.linalg.cholesky(Vd)
            Vi = np.linalg.inv(Vd)
        except np.linalg.LinAlgError:
            return None
        S = Ur - np.einsum("tar,tab,tbq->rq", Ws, Vi, Ws)
        rhs = sr * g_r - np.einsum("tar,tab,tb->r", Ws, Vi, bt)
        if nr > 0:
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                return None
            yr = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        else:
            yr = np.zeros(0)
        yt = np.einsum("tab,tb->ta", Vi, bt - np.einsum("tar,r->ta", Ws, yr))
        delta = np.zeros(self.mc.n)
        delta[self.x_red] = -sr * yr
        delta[self.x_tim] = -(st * yt).ravel()
        return delta


def minimise(smc, max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
             max_lm_diagonal=1e32, max_invalid=5):
    """Ceres' LM with the time blocks eliminated -> (x, summary, iteration rows), as marker_loss_ref.minimise returns them."""
    mc = smc.mc
    x = smc.x0()
    rows = []
    lin = smc.linearise(x)
    cost, sumsq = lin[0], lin[8]
    g = smc.gradient(lin)
    gmax = lambda g: float(np.abs(g).max()) if g.size else 0.0   # noqa: E731
    scale = 1.0 / (1.0 + np.sqrt(smc.diag(lin)))
    rows.append(dict(iteration=0, cost=cost, cost_change=0.0, gradient_max_norm=gmax(g), step_norm=0.0, relative_decrease=0.0,
                     trust_region_radius=initial_radius, valid=0, successful=0))
    out = dict(initial_cost=cost)

    def done(term, reason):
        return x, dict(out, termination=term, reason=reason, final_cost=cost, final_sumsq=sumsq), rows

    if gmax(g) <= gradient_tolerance:
        return done("CONVERGENCE", "gradient")
    radius, dec, invalid, it = initial_radius, 2.0, 0, 0
    while True:
        if it >= max_num_iterations:
            return done("NO_CONVERGENCE", "max_iterations")
        if gmax(g) <= gradient_tolerance:
            return done("CONVERGENCE", "gradient")
        if radius < min_radius:
            return done("CONVERGENCE", "min_radius")
        it += 1
        row = dict(iteration=it, cost=cost, cost_change=0.0, gradient_max_norm=gmax(g), step_norm=0.0, relative_decrease=0.0,
                   trust_region_radius=radius, valid=0, successful=0)
        delta = smc.step(lin, scale, radius, min_lm_diagonal, max_lm_diagonal)
        ok = delta is not None
        if ok:
            mcc = mc.model_cost_change(lin[1], lin[2], delta)
            ok = bool(np.all(np.isfinite(delta))) and mcc > 0.0
        if not ok:
            invalid += 1
            radius /= dec
            dec *= 2.0
            row["trust_region_radius"] = radius
            rows.append(row)
            if invalid >= max_invalid:
                return done("FAILURE", "invalid_steps")
            continue
        invalid = 0
        row["valid"] = 1
        xc = x + delta
        cand, _ = mc.cost(xc)
        row["step_norm"] = float(np.linalg.norm(delta))
        if row["step_norm"] <= parameter_tolerance * (np.linalg.norm(x) + parameter_tolerance):
            rows.append(row)
            return done("CONVERGENCE", "parameter")
        row["cost_change"] = cost - cand
        if abs(cost - cand) <= function_tolerance * cost:
            rows.append(row)
            return done("CONVERGENCE", "function")
        rel = (cost - cand) / mcc
        row["relative_decrease"] = rel
        if np.isfinite(cand) and rel > min_relative_decrease:
            x = xc
            lin = smc.linearise(x)
            cost, sumsq = lin[0], lin[8]
            g = smc.gradient(lin)
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            dec = 2.0
            row.update(successful=1, cost=cost, gradient_max_norm=gmax(g))
        else:
            radius /= dec
            dec *= 2.0
        row["trust_region_radius"] = radius
        rows.append(row)
