"""TEST INFRASTRUCTURE for the whole-rig start (rsba_problem_start_rig): a Python restatement of the propagation's rounds
(csrc/ba_rig_start_plan.hpp), written from the rule and sharing no code with the planner; the crafted co-visibility graphs of the host test;
the builder and runner of tests/rig_start_plan_driver.cpp; and the problems the GPU tests share with it.  Only tests and tools import it.

The rule: from the known blocks (the caller's flags; the base camera always) a TIME round fits every unknown time that some known camera
detected, a CAMERA round every unknown camera that detected a known time; rounds take turns, a round that would fit nothing is not
launched, and the propagation ends when a time round and a camera round in a row fit nothing.  Then `sweeps` passes: all fitted times,
then all fitted cameras.  What no round reaches is unreachable."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
TIME, CAMERA = 0, 1


def plan(C, T, cam, tim, known=None, sweeps=0):
    """-> dict(launches=[(which, sweep, [blocks])], num_rounds, unreachable_times, unreachable_cameras)"""
    cam, tim = [int(v) for v in cam], [int(v) for v in tim]
    flags = set() if known is None else {b for b in range(C + T) if known[b]}
    if C > 0:
        flags.add(0)
    given = set(flags)
    cams_of_time = {t: {c for c, tt in zip(cam, tim) if tt == t} for t in range(T)}
    times_of_cam = {c: {t for cc, t in zip(cam, tim) if cc == c} for c in range(C)}
    launches, fitted, turn, idle = [], set(), TIME, 0
    while idle < 2:
        if turn == TIME:
            new = [t for t in range(T) if C + t not in flags and any(c in flags for c in cams_of_time[t])]
            add = {C + t for t in new}
        else:
            new = [c for c in range(C) if c not in flags and any(C + t in flags for t in times_of_cam[c])]
            add = set(new)
        if new:
            launches.append((turn, 0, new))
            flags |= add
            fitted |= add
            idle = 0
        else:
            idle += 1
        turn = CAMERA if turn == TIME else TIME
    rounds = len(launches)
    for s in range(1, sweeps + 1):
        for which, blocks in ((TIME, [t for t in range(T) if C + t in fitted]), (CAMERA, [c for c in range(C) if c in fitted])):
            if blocks:
                launches.append((which, s, blocks))
    assert not (fitted & given)
    return dict(launches=launches, num_rounds=rounds, unreachable_times=[t for t in range(T) if C + t not in flags],
                unreachable_cameras=[c for c in range(C) if c not in flags])


def csr(n, key):
    """(ptr, obs): the observations grouped by key, in observation order inside a group."""
    key = np.asarray(key, int)
    order = np.argsort(key, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))]) if n else np.zeros(1, int)
    return [int(v) for v in ptr], [int(v) for v in order]


def graphs():
    """name -> (C, T, M, cam, tim, known or None, sweeps, what the rule gives in words: (round kinds, unreachable times, cameras))"""
    g = {}
    full = [(c, t) for t in range(5) for c in range(3)]
    g["every camera sees every time"] = (3, 5, 2, full, None, 1, ([TIME, CAMERA], [], []))
    # camera 0: times 0-1; camera 1: times 1-2; camera 2: times 2-3 (time 3 is seen by camera 2 alone: a fifth round)
    chain = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)]
    g["a chain of cameras"] = (3, 3, 2, chain, None, 2, ([TIME, CAMERA, TIME, CAMERA], [], []))
    g["a chain whose last camera has a shot of its own"] = (3, 4, 2, chain + [(2, 3)], None, 0, ([TIME, CAMERA, TIME, CAMERA, TIME], [], []))
    g["a camera with no shared shot"] = (3, 4, 2, [(0, 0), (1, 0), (0, 1), (2, 2), (2, 3)], None, 1, ([TIME, CAMERA], [2, 3], [2]))
    g["a time nobody detected"] = (2, 3, 2, [(0, 0), (1, 0), (0, 2), (1, 2)], None, 1, ([TIME, CAMERA], [1], []))
    g["all cameras given"] = (3, 4, 2, [(0, 0), (1, 1), (2, 2), (1, 3), (2, 3)], [1, 1, 1, 0, 0, 0, 0], 1, ([TIME], [], []))
    g["the times given"] = (3, 2, 2, [(0, 0), (1, 0), (2, 1)], [0, 0, 0, 1, 1], 1, ([CAMERA], [], []))
    g["camera 0 saw nothing"] = (2, 2, 2, [(1, 0), (1, 1)], None, 1, ([], [0, 1], [1]))
    g["several detections a pair, out of order"] = (3, 3, 4, [(2, 2), (0, 0), (1, 2), (0, 0), (1, 0), (2, 2), (1, 0), (0, 1)], None, 1,
                                                    ([TIME, CAMERA, TIME, CAMERA], [], []))
    out = {}
    for name, (C, T, M, rows, known, sweeps, want) in g.items():
        out[name] = (C, T, M, [r[0] for r in rows], [r[1] for r in rows], known, sweeps, want)
    return out


def build_driver(directory):
    """The driver under AddressSanitizer and UBSan -> its path."""
    exe = os.path.join(str(directory), "rig_start_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "rig_start_plan_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, args=()):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "rig start driver: ok" in r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()]


def host_start(exe, path, prob, model, known=None, sweeps=0):
    """The whole start on the host, serially (the driver's `fit`): -> (blocks (C + T) x 6, rms, status, iterations)."""
    C, T, M, N = prob["C"], prob["T"], prob["M"], prob["N"]
    dist = prob.get("dist")
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, float).ravel())   # noqa: E731
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %r %d %d\n" % (1 if model == 2 else 0, C, T, M, N, 0 if dist is None else 1, float(prob["marker_side"]), sweeps,
                                                   0 if known is None else 1))
        f.write(num(prob["intr"]) + "\n")
        if dist is not None:
            f.write(num(dist) + "\n")
        f.write(num(prob["params"]) + "\n")
        if known is not None:
            f.write(" ".join(str(int(v)) for v in known) + "\n")
        for i in range(N):
            f.write("%d %d %d %s\n" % (prob["c"][i], prob["t"][i], prob["m"][i], num(prob["obs"][i])))
    (line,) = run_driver(exe, ["fit", str(path)])
    return (np.array(line["blocks"]).reshape(C + T, 6), np.array(line["rms"]), np.array(line["status"]), np.array(line["iterations"]))


# ---- the problems the host test and the GPU tests share -------------------------------------------------------------------------
def keep_rows(prob, mask):
    """A copy of a synthetic.make_marker_chain problem with the rows of mask only."""
    out = dict(prob)
    mask = np.asarray(mask, bool)
    for k in ("t", "c", "m", "obs"):
        out[k] = np.ascontiguousarray(np.asarray(prob[k])[mask])
    out["N"] = int(mask.sum())
    return out


def small_problem(dist=None, seed=60):
    """3 cameras x 4 times x 4 markers, every pair detected (keep = 1): the shape of the oracle comparisons and of the host fit.  With
    coefficients the detections are the truth's distorted projection plus the generator's noise level."""
    from realsensecalibration_amd import synthetic as syn
    prob = syn.make_marker_chain(3, 4, 4, seed=seed, keep=1.0)
    if dist is not None:
        import marker_distortion_ref as mdr
        prob = mdr.redetect(prob, dist, 0.3, seed)
    return prob


def oracle_minimiser(prob, variant, free_blocks, dist=None):
    """The (C + T + M) x 6 minimiser with every block but free_blocks constant at prob["params"], the free ones started from the truth.
    Tolerances: only the parameter tolerance can fire, at a step below 1e-11 (1 + |x|) — function and gradient tolerance are zero.  Pinhole:
    the C oracle's solve_marker_chain_constant.  With coefficients, which that oracle does not take, marker_distortion_ref's numpy
    restatement of the same Levenberg-Marquardt on the distorted functors with the same constant blocks."""
    nb = prob["C"] + prob["T"] + prob["M"]
    start = np.asarray(prob["params"], float).reshape(nb, 6).copy()
    truth = np.asarray(prob["truth"], float).reshape(nb, 6)
    free_blocks = sorted(int(b) for b in free_blocks)
    start[free_blocks] = truth[free_blocks]
    const = [b for b in range(nb) if b not in free_blocks]
    p2 = dict(prob, params=start.ravel())
    if dist is None:
        import oracle_lib as ol
        o = ol.load()
        opts = o.options(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=1e-11, max_num_iterations=200)
        params, s, _ = o.solve_marker_chain_constant(p2, variant, prob["marker_side"], np.asarray(prob["intr"], float).ravel(), const, opts=opts, max_log=256)
        assert s.termination == 0, (s.termination, s.stop_reason)
        return params.reshape(nb, 6)
    import marker_distortion_ref as mdr
    import marker_loss_ref as ref
    mc = mdr.MarkerChainDist(p2, dist, variant=variant, constant_blocks=const)
    x, summary, _ = ref.minimise(mc, max_num_iterations=200, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=1e-11)
    assert summary["termination"] == "CONVERGENCE", summary
    return mc.full(x)
