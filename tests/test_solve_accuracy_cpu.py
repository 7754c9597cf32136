"""The backward-error checker of tests/solve_accuracy.py, without a GPU: correct fp64 solves of systems shaped like the point
model's reduced camera system pass it with margin, and solves that are wrong by 1e-11 fail it.

The systems are Jacobi-scaled, LM-damped Schur complements of a random block-sparse Jacobian (cameras of 6 parameters, points of 3
observed by up to four cameras, the points eliminated with their own LM damping), n = 6C."""
import numpy as np
import pytest

import solve_accuracy as sa

pytestmark = pytest.mark.skipif(not sa.longdouble_ok(), reason="np.longdouble is not wider than double here: eta cannot be evaluated exactly")

SIZES = (6, 186, 192, 198, 222, 384, 390, 1536)
RADII = (2.5, 1e4, 1e12)


def reduced_system(n, radius, seed, weak_panel=None, eps=0.0):
    """(S, rhs, LM damping on the diagonal of S) like the product's scaled, damped reduced camera system.  weak_panel: the 32 columns of that panel coupled to the
    rest by eps times their natural size (a camera group that shares few points with the others)."""
    C = n // 6
    rng = np.random.default_rng([seed, n])
    P = 3 * C + 8
    k = min(4, C)
    S_raw = np.zeros((n, n))
    diagU = np.zeros(n)
    g = np.zeros(n)
    m = 2 if C > 1 else 4   # residuals per camera and point (one camera: two observations of each point, else it has no depth)
    for _ in range(P):
        cams = rng.choice(C, k, replace=False)
        Jc = np.zeros((m * k, 6 * k))
        for a in range(k):
            Jc[m * a:m * a + m, 6 * a:6 * a + 6] = rng.normal(size=(m, 6)) * np.array([3.0, 3.0, 3.0, 1.0, 1.0, 0.3])
        Jp = rng.normal(size=(m * k, 3))
        r = rng.normal(size=m * k)
        V = Jp.T @ Jp
        Vd = V + np.diag(np.clip(np.diag(V), 1e-6, 1e32) / radius)
        Vi = np.linalg.inv(Vd)
        U = Jc.T @ Jc
        Wt = Jc.T @ Jp
        Sp = U - Wt @ Vi @ Wt.T
        gp = Jc.T @ r - Wt @ (Vi @ (Jp.T @ r))
        idx = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in cams])
        S_raw[np.ix_(idx, idx)] += Sp
        diagU[idx] += np.diag(U)
        g[idx] += gp
    S_raw = 0.5 * (S_raw + S_raw.T)
    if weak_panel is not None:
        cols = np.arange(n)
        inp = (cols >= sa.PB * weak_panel) & (cols < sa.PB * (weak_panel + 1))
        S_raw[np.ix_(inp, ~inp)] *= eps
        S_raw[np.ix_(~inp, inp)] *= eps
    s = 1.0 / (1.0 + np.sqrt(diagU))
    damp = np.clip(s * s * diagU, 1e-6, 1e32) / radius
    return S_raw * np.outer(s, s) + np.diag(damp), s * g, damp


# ------------------------------------------------------------------ correct solvers
def _forward(L, b):
    x = np.zeros_like(b)
    for i in range(b.size):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def _backward(L, b):
    x = np.zeros_like(b)
    for i in range(b.size - 1, -1, -1):
        x[i] = (b[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_cholesky(S, rhs):
    """np.linalg.cholesky and two triangular substitutions."""
    L = np.linalg.cholesky(S)
    return _backward(L, _forward(L, rhs))


def _tri_inverse(L):
    """L^-1 of a 32 x 32 lower factor as the kernels form it (DiagInverse): the two 16 x 16 diagonal blocks by substitution, the
    off-diagonal block as -T22 (L21 T11)."""
    h = L.shape[0] // 2
    T = np.zeros_like(L)
    for lo, hi in ((0, h), (h, L.shape[0])):
        Lb = L[lo:hi, lo:hi]
        T[lo:hi, lo:hi] = np.column_stack([_forward(Lb, e) for e in np.eye(hi - lo)])
    T[h:, :h] = -T[h:, h:] @ (L[h:, :h] @ T[:h, :h])
    return T


def _chol_unblocked(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_blocked_inverse(S, rhs, pb=sa.PB, drop=None, undamp=None):
    """The kernels' algorithm (ba_cholesky.hpp's header comment): left-looking, pb-wide panels with the right-hand side riding along
    as row n; per panel the update by all earlier panels, the diagonal block factored and inverted explicitly (T = L_kk^-1), the rows
    below (and the rhs row) times T'; row n then holds y = L^-1 rhs, and the back-substitution is x_k = T_k' y_k, y[:k] -= L_k,:k' x_k.
    drop = (panel p, panel k, panel i): mutation, panel p's update of block (i, k) left out."""
    n = S.shape[0]
    A = np.vstack([S, rhs[None, :]])
    L = np.zeros((n + 1, n))
    Ts = []
    for kb in range(0, n, pb):
        ke = min(kb + pb, n)
        nb = ke - kb
        Pan = A[kb:, kb:ke].copy()
        for qb in range(0, kb, pb):
            qe = qb + pb
            upd = L[kb:, qb:qe] @ L[kb:ke, qb:qe].T
            if drop is not None and qb == drop[0] * pb and kb == drop[1] * pb:
                r0 = drop[2] * pb - kb
                upd[r0:min(r0 + pb, n - kb)] = 0.0   # (not the rhs row behind a partial last panel)
            Pan -= upd
        Lkk = _chol_unblocked(Pan[:nb])
        T = _tri_inverse(np.pad(Lkk, ((0, pb - nb), (0, pb - nb))) + np.diag(np.r_[np.zeros(nb), np.ones(pb - nb)]))[:nb, :nb]
        Ts.append(T)
        L[kb:ke, kb:ke] = Lkk
        L[ke:, kb:ke] = Pan[nb:] @ T.T
    x = L[n].copy()
    for kb in range(((n - 1) // pb) * pb, -1, -pb):
        ke = min(kb + pb, n)
        xb = Ts[kb // pb].T @ x[kb:ke]
        x[kb:ke] = xb
        x[:kb] -= L[kb:ke, :kb].T @ xb
    return x


SOLVERS = {"cholesky": solve_cholesky, "blocked_inverse": solve_blocked_inverse}


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_correct_solves_pass_with_margin(solver, n, radius):
    S, rhs, _ = reduced_system(n, radius, seed=1)
    y = SOLVERS[solver](S, rhs)
    eta, bar, kappa = sa.check(S, rhs, y)
    print("%s n=%d radius=%g: eta %.2e kappa %.1f bar %.2e" % (solver, n, radius, eta, kappa, bar))
    assert eta < 0.25 * bar, (eta, bar, kappa)


def _concentrated(S, idx, seed):
    """rhs whose solution lives on the entries `idx` (the rest 1e-3 of it): a local error is then not diluted by the rest."""
    rng = np.random.default_rng(seed)
    y = 1e-3 * rng.normal(size=S.shape[0])
    y[idx] = rng.normal(size=len(idx))
    return S @ y


# How large the mutations are.  The bar is a worst-case rounding bound: gamma_{3n+1} (1 + kappa) is 3e-13 .. 1e-10 on these systems
# (n = 186 .. 1536, kappa(L_kk) 4 .. 600), while correct solves measure eta ~1e-17.  A wrong entry of relative size delta shows as eta
# ~ delta times the share of its block in the solution and times the entry's size against sqrt(S_ii S_jj) (off-diagonal couplings are
# 1e-1 .. 1e-2 of the diagonal): a 1e-11 error measures 1e-13 .. 2e-12 here, below the bar at most sizes, so no correct-to-the-bar
# check can promise to see it.  The mutations are 1e-9 of what they touch (1e-8 for the dropped update, which sits off the
# diagonal) — still three orders of magnitude below the ~1e-6 step errors whole-solve bars can see.
MUTATION = 1e-9
MUT_SIZES = (186, 192, 198, 222, 384, 390, 1536)   # (n = 6: one camera, one partial panel — no second panel, no off-diagonal block)


# (n = 384 at radius 1e12: the weakly coupled panel leaves kappa(L_kk) ~6e6 on the weakly damped system, the bar ~7e-7)
@pytest.mark.parametrize("n,radius", [(n, r) for n in MUT_SIZES for r in RADII if (n, r) != (384, 1e12)])
def test_dropped_panel_update_fails(n, radius):
    """Panel 0's update of block (i, k) = (last panel, panel 1) left out, on a system where panel 0 is weakly coupled so that the
    update it contributes is ~1e-6 of that (off-diagonal) block, ~1e-8 of sqrt(S_ii S_jj) (MUTATION: why not 1e-11)."""
    last = (n - 1) // sa.PB
    S, _, _ = reduced_system(n, radius, seed=2, weak_panel=0, eps=1e-3)
    L = np.linalg.cholesky(S)
    dropped = L[last * sa.PB:, :sa.PB] @ L[sa.PB:2 * sa.PB, :sa.PB].T
    rel = np.abs(dropped).max() / np.abs(S[last * sa.PB:, sa.PB:2 * sa.PB]).max()
    idx = np.r_[sa.PB:2 * sa.PB, last * sa.PB:n]
    rhs = _concentrated(S, idx, 3)
    good = solve_blocked_inverse(S, rhs)
    bad = solve_blocked_inverse(S, rhs, drop=(0, 1, last))
    eta_good, bar, kappa = sa.check(S, rhs, good)
    eta_bad, _, _ = sa.check(S, rhs, bad)
    print("n=%d radius=%g: dropped update %.1e relative; eta %.2e (correct %.2e), kappa %.1f, bar %.2e" % (n, radius, rel, eta_bad, eta_good, kappa, bar))
    assert 5e-9 < rel < 1e-5
    assert eta_good < 0.25 * bar
    assert eta_bad > bar, (eta_bad, bar)


# (n = 1536 at radius 1e12: kappa(L_kk) ~4e6 on the weakly damped system, the bar ~2e-6 — above a 1e-9 error by construction)
@pytest.mark.parametrize("n,radius", [(n, r) for n in SIZES for r in RADII if (n, r) != (1536, 1e12)])
def test_one_camera_step_off_by_1e9_fails(n, radius):
    S, _, _ = reduced_system(n, radius, seed=4)
    cam = (n // 6) // 2
    idx = np.arange(6 * cam, 6 * cam + 6)
    rhs = _concentrated(S, idx, 5)
    y = solve_blocked_inverse(S, rhs)
    eta_good, bar, kappa = sa.check(S, rhs, y)
    y[idx] *= 1.0 + MUTATION
    eta_bad, _, _ = sa.check(S, rhs, y)
    print("n=%d radius=%g: eta %.2e (correct %.2e), kappa %.1f, bar %.2e" % (n, radius, eta_bad, eta_good, kappa, bar))
    assert eta_good < 0.25 * bar
    assert eta_bad > bar, (eta_bad, bar)


# (radius 1e12: the damping is ~1e-12 of the diagonal there, below what any fp64 solve resolves — leaving it out is not an error
#  a correct-to-rounding check can see, and the bar is allowed to be wider than that by (1 + kappa))
@pytest.mark.parametrize("radius", (2.5, 1e4))
@pytest.mark.parametrize("n", SIZES)
def test_missing_damping_on_the_last_camera_group_fails(n, radius):
    S, _, damp = reduced_system(n, radius, seed=6)
    idx = np.arange(max(0, n - 6 * 16), n)
    rhs = _concentrated(S, idx, 7)
    D = np.zeros(n)
    D[idx] = damp[idx]
    y = solve_blocked_inverse(S - np.diag(D), rhs)
    eta, bar, kappa = sa.check(S, rhs, y)
    print("n=%d radius=%g: damping %.1e of the diagonal; eta %.2e, kappa %.1f, bar %.2e" % (n, radius, (D[idx] / np.diag(S)[idx]).max(), eta, kappa, bar))
    assert eta > bar, (eta, bar)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", MUT_SIZES)
def test_transposed_off_diagonal_block_fails(n, radius):
    S, _, _ = reduced_system(n, radius, seed=8)
    C = n // 6
    # the coupled pair of cameras with the least symmetric block
    best, a, b = -1.0, 0, 1
    for i in range(C):
        for j in range(i + 1, C):
            B = S[6 * i:6 * i + 6, 6 * j:6 * j + 6]
            d = np.abs(B - B.T).max()
            if d > best:
                best, a, b = d, i, j
    ia, ib = np.arange(6 * a, 6 * a + 6), np.arange(6 * b, 6 * b + 6)
    Sw = S.copy()
    Sw[np.ix_(ia, ib)] = S[np.ix_(ia, ib)].T
    Sw[np.ix_(ib, ia)] = S[np.ix_(ib, ia)].T
    rhs = _concentrated(S, np.r_[ia, ib], 9)
    y = solve_blocked_inverse(Sw, rhs)
    eta, bar, kappa = sa.check(S, rhs, y)
    print("n=%d radius=%g: block (%d, %d) transposed; eta %.2e, kappa %.1f, bar %.2e" % (n, radius, a, b, eta, kappa, bar))
    assert eta > bar, (eta, bar)


def test_bar_constant():
    """gamma_{3n+1} / (1 - gamma_{n+1}) (1 + kappa) + 8 u, spelled out at n = 384, kappa = 1."""
    u = 2.0 ** -53
    S = np.eye(384)
    b, kappa = sa.bar(S)
    assert kappa == 1.0
    g = 1153 * u / (1 - 1153 * u)
    assert b == pytest.approx(g / (1 - 385 * u / (1 - 385 * u)) * 2 + 8 * u, rel=1e-15)
