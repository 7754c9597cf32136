"""The path a step of the point model takes — schedule, factorisation, workgroups, back-substitution — for a camera count and the
RSBA_* switches, stated independently of the library: tests/test_gpu_reduced_solve.py holds the path a step reports on the GPU to
it, tests/test_step_plan_host.py the library's host-side plan (csrc/ba_step_plan.hpp) for every camera count."""
TG, PB, MAXN = 16, 32, 384   # RSBA_TG cameras per group, RSBA_PB panel width, RSBA_CHOL_MAXN
CUS = 256                    # MI355X compute units (the persistent tiles must all fit: 2 per CU)


def expected_path(env, C, impl):
    """The selection rules of rsba_solver_create / PointsStep (ba_solver.hip) for one rank."""
    n = 6 * C
    m = (n + PB - 1) // PB * PB
    pipeline = env.get("RSBA_PIPELINE", "1") != "0"
    tiles_small = env.get("RSBA_TILES_SMALL", "0") != "0" and n <= MAXN and C > TG
    chol_tiles = env.get("RSBA_CHOL_TILES", "1") != "0"
    bsm = int(env.get("RSBA_BACKSUB_MULTI", "2"))
    pipelined = pipeline and impl != 0 and C > TG and n <= MAXN
    ngroups = (C + TG - 1) // TG
    border_ok = env.get("RSBA_BORDER", "1") != "0" and ngroups >= 3
    wgs, diag, border = 1, False, 0
    want = int(env["RSBA_CHOL_WGS"]) if "RSBA_CHOL_WGS" in env else (3 if border_ok else 6)
    if want > 1 and impl != 0 and 6 * PB <= n <= MAXN:
        wgs = min(want, 8)
        np_rule = 3 * (ngroups - 1) if border_ok else m // PB
        diag = wgs >= 2 and (np_rule - 2 + wgs - 2) // (wgs - 1) <= 4
        if not diag:
            wgs = 1
        if border_ok and diag:
            border = 6 * TG * (ngroups - 1)
    nrt = (m + 1 + 63) // 64
    tiles = nrt * (nrt + 1) // 2 if (n > MAXN or tiles_small) and chol_tiles and nrt * (nrt + 1) // 2 <= 2 * CUS else 0
    if pipelined:
        tiled = False
    else:
        tiled = n > MAXN or (tiles_small and tiles > 0)
    if not tiled:
        fact = ("diag_border" if border else "diag") if diag else "one_wg"
        return dict(schedule="pipelined" if pipelined else "sequential", factorisation=fact,
                    workgroups=wgs + (1 if border else 0) if diag else 1, border_cols=border, tiles=0, backsub="in_kernel", sys_fused=False)
    if tiles:
        backsub = "chain" if bsm >= 2 else ("multi" if bsm == 1 else "one_wg")
        return dict(schedule="sequential", factorisation="tiles_small" if n <= MAXN else "tiled", workgroups=tiles, border_cols=0, tiles=tiles,
                    backsub=backsub, sys_fused=env.get("RSBA_SYS_FUSED", "1") != "0")
    r0 = min(PB, n)
    nrt1 = (n + 1 - r0 + 63) // 64
    return dict(schedule="sequential", factorisation="multi_launch", workgroups=nrt1 * (nrt1 + 1) // 2, border_cols=0, tiles=0, backsub="one_wg",
                sys_fused=False)
