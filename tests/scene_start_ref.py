"""TEST INFRASTRUCTURE for the scene start (rsba_problem_start_scene): a Python restatement of the three-kind propagation
(csrc/ba_scene_start_plan.hpp), written from the rule and sharing no code with the planner; the crafted graphs of the host test; the
builder and runner of tests/scene_start_driver.cpp; and the problems the GPU tests share with it.  Only tests and tools import it.

The rule: the known blocks are the caller's flags over cameras, times and markers, the base camera always, and marker 0 where it is the
base marker (the chain model; in the Test2 wiring it is an ordinary block).  A detection serves a block when its two OTHER blocks are known.
Rounds take turns TIME, MARKER, CAMERA: each fits every unknown block of its kind that some detection serves; a round that would fit
nothing is not launched, and three such rounds in a row end the propagation.  Then `sweeps` passes: all fitted times, then all fitted
markers, then all fitted cameras.  What no round reaches is unreachable."""
import json
import os
import subprocess

import numpy as np

import rig_start_ref as rs

ROOT = rs.ROOT
CSRC = rs.CSRC
TIME, CAMERA, MARKER = 0, 1, 2
ORDER = (TIME, MARKER, CAMERA)


def plan(C, T, M, cam, tim, mar, known=None, sweeps=0, base_marker=True):
    """-> dict(launches=[(which, sweep, [blocks])], num_rounds, unreachable_times, unreachable_cameras, unreachable_markers); a block is
    named by (kind, index) here, not by its place in the flags."""
    rows = [(int(c), int(t), int(m)) for c, t, m in zip(cam, tim, mar)]
    have = set()
    if known is not None:
        have |= {(CAMERA, c) for c in range(C) if known[c]}
        have |= {(TIME, t) for t in range(T) if known[C + t]}
        have |= {(MARKER, m) for m in range(M) if known[C + T + m]}
    if C > 0:
        have.add((CAMERA, 0))
    if M > 0 and base_marker:
        have.add((MARKER, 0))
    given = set(have)
    size = {TIME: T, CAMERA: C, MARKER: M}

    def served(kind, index):
        for c, t, m in rows:
            names = {CAMERA: c, TIME: t, MARKER: m}
            if names[kind] == index and all((k, names[k]) in have for k in names if k != kind):
                return True
        return False

    launches, fitted, idle, turn = [], set(), 0, 0
    while idle < 3:
        kind = ORDER[turn % 3]
        turn += 1
        new = [b for b in range(size[kind]) if (kind, b) not in have and served(kind, b)]
        if not new:
            idle += 1
            continue
        idle = 0
        launches.append((kind, 0, new))
        have |= {(kind, b) for b in new}
        fitted |= {(kind, b) for b in new}
    rounds = len(launches)
    for s in range(1, sweeps + 1):
        for kind in ORDER:
            blocks = [b for b in range(size[kind]) if (kind, b) in fitted]
            if blocks:
                launches.append((kind, s, blocks))
    assert not (fitted & given)
    return dict(launches=launches, num_rounds=rounds, unreachable_times=[t for t in range(T) if (TIME, t) not in have],
                unreachable_cameras=[c for c in range(C) if (CAMERA, c) not in have],
                unreachable_markers=[m for m in range(M) if (MARKER, m) not in have])


def graphs():
    """name -> (C, T, M, cam, tim, mar, known or None, sweeps, base_marker, what the rule gives in words: (round kinds, unreachable times,
    cameras, markers))"""
    g = {}
    full = [(c, t, m) for t in range(3) for c in range(3) for m in range(3)]
    g["every camera sees every marker at every time"] = (3, 3, 3, full, None, 1, True, ([TIME, MARKER, CAMERA], [], [], []))
    # the shape of the committed hongo file: without a shot of the base marker by the base camera there is no first round
    blind = [r for r in full if not (r[0] == 0 and r[2] == 0)]
    g["camera 0 never sees marker 0"] = (3, 3, 3, blind, None, 1, True, ([], [0, 1, 2], [1, 2], [1, 2]))
    # camera 0 sees markers 0 and 1, camera 1 markers 0, 1 and 2: marker 2 waits for camera 1
    lone = [(0, t, m) for t in range(2) for m in (0, 1)] + [(1, t, m) for t in range(2) for m in (0, 1, 2)]
    g["a marker only camera 1 sees"] = (2, 2, 3, lone, None, 1, True, ([TIME, MARKER, CAMERA, MARKER], [], [], []))
    # at time 2 camera 0 sees marker 2 alone (and camera 1 nothing): the time waits for the marker round; camera 1 joins in between
    late = [(0, 0, 0), (0, 0, 2), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 2, 2)]
    g["a time at which the known cameras see only marker 2"] = (2, 3, 3, late, None, 2, True, ([TIME, MARKER, CAMERA, TIME], [], [], [1]))
    g["test2 wiring, nothing flagged"] = (3, 3, 3, full, None, 1, False, ([], [0, 1, 2], [1, 2], [0, 1, 2]))
    g["test2 wiring, marker 0 flagged"] = (3, 3, 3, full, [0] * 6 + [1, 0, 0], 1, False, ([TIME, MARKER, CAMERA], [], [], []))
    g["the board given, a chain of cameras"] = (3, 3, 2, [(0, 0, 0), (0, 1, 1), (1, 1, 0), (1, 2, 1), (2, 2, 0)], [0] * 6 + [1, 1], 1, True,
                                                ([TIME, CAMERA, TIME, CAMERA], [], [], []))
    g["cameras and times given, out of order"] = (2, 2, 4, [(1, 1, 3), (0, 0, 1), (1, 0, 2), (0, 1, 3), (1, 1, 1)], [1, 1, 1, 1, 0, 0, 0, 0], 1, True,
                                                  ([MARKER], [], [], []))
    out = {}
    for name, (C, T, M, rows, known, sweeps, base, want) in g.items():
        out[name] = (C, T, M, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], known, sweeps, base, want)
    return out


def rig_graphs_with_the_board_given():
    """Every graph of rig_start_ref.graphs() with a marker index dealt to each row and all markers flagged:
    name -> (C, T, M, cam, tim, mar, known C + T + M, sweeps, the (C + T) flags rig_start_ref.plan takes)"""
    out = {}
    for name, (C, T, M, cam, tim, known, sweeps, _) in rs.graphs().items():
        flags = list(known) if known is not None else [0] * (C + T)
        out[name] = (C, T, M, cam, tim, [i % M for i in range(len(cam))], flags + [1] * M, sweeps, known)
    return out


def build_driver(directory):
    """The driver under AddressSanitizer and UBSan -> its path (rig_start_ref.build_driver's command line)."""
    exe = os.path.join(str(directory), "scene_start_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "scene_start_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, args=()):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "scene start driver: ok" in r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()]


def write_plan_cases(path, cases):
    """cases: (C, T, M, cam, tim, mar, known or None, sweeps, base_marker) -> the driver's `plan` file."""
    with open(path, "w") as f:
        for C, T, M, cam, tim, mar, known, sweeps, base in cases:
            f.write("%d %d %d %d %d %d %d\n" % (C, T, M, len(cam), sweeps, 0 if known is None else 1, 1 if base else 0))
            if known is not None:
                f.write(" ".join(str(int(v)) for v in known) + "\n")
            f.write("".join("%d %d %d\n" % r for r in zip(cam, tim, mar)))


def host_start(exe, path, prob, model, known=None, sweeps=0):
    """The whole scene start on the host, serially (the driver's `fit`): -> (blocks (C + T + M) x 6, rms, status, iterations)."""
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
    return (np.array(line["blocks"]).reshape(C + T + M, 6), np.array(line["rms"]), np.array(line["status"]), np.array(line["iterations"]))


# ---- the problems the host test and the GPU tests share -------------------------------------------------------------------------
MARKER_CASES = {"chain": (1, "pinhole"), "test2": (2, "pinhole"), "distorted": (1, "distorted")}


def marker_case(name):
    """rig_start_ref.small_problem (3 x 4 x 4, every pair detected) with cameras and times given at the problem's values and markers 1-3
    zeroed: -> (model, dist or None, problem as generated, the same with the markers zeroed, flags, the free blocks).  The Test2 wiring flags
    marker 0 too."""
    import marker_pose_ref as mp
    model, config = MARKER_CASES[name]
    dist = mp.DIST3[config]
    prob = rs.small_problem(dist)
    C, T, M = prob["C"], prob["T"], prob["M"]
    free = [C + T + m for m in range(1, M)]
    zeroed = dict(prob, params=np.asarray(prob["params"], float).copy())
    for b in free:
        zeroed["params"][6 * b:6 * b + 6] = 0.0
    known = [1] * (C + T) + [1 if model == 2 else 0] + [0] * (M - 1)
    return model, dist, prob, zeroed, known, free


def unknown_board(prob):
    """A copy of prob with every camera, time and non-base marker block zeroed (the base blocks of the chain model are zeros already)."""
    out = dict(prob, params=np.asarray(prob["params"], float).copy())
    nb = prob["C"] + prob["T"] + prob["M"]
    keep = prob["C"] + prob["T"]            # marker 0: the base marker, the identity
    blocks = out["params"].reshape(nb, 6)   # (a view)
    base = blocks[keep].copy()
    blocks[:] = 0.0
    blocks[keep] = base
    return out
