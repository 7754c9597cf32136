"""The single-marker pose fit of the host build under AddressSanitizer and UBSan: tests/marker_pose_driver.cpp (a stand-alone program with
its own main) is compiled with ba_marker_pose.hpp, the C ABI's host units and include/rsba/correspondencer.h, as
tests/test_distortion_math_host.py builds its driver, and run directly on the synthetic set of tests/marker_pose_ref.py with the
reference's poses beside it.  It checks the header routine against the reference at 1e-6, the C entry and the C++ mirror for the same
bits, the degenerate inputs, the argument checks and rsba_problem_initial_time_poses on a problem made of those detections."""
import os
import subprocess

import marker_pose_ref as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "marker_pose_driver.cpp")] + [os.path.join(CSRC, f) for f in ("ba_problem.cpp", "rsba_capi.cpp", "ba_initial_guess.cpp", "ba_schur_plan.cpp")]


def test_marker_pose_under_asan_and_ubsan(tmp_path):
    cases = tmp_path / "cases.txt"
    with open(cases, "w") as f:
        for config in sorted(mp.DIST3):
            n = 60
            corners, cam, intr, dist, _ = mp.batch(config, n)
            want, rms = mp.reference(config, n)
            for i in range(n):
                d = [0.0] * 5 if dist is None else dist[cam[i]]
                row = list(intr[cam[i]]) + [0 if dist is None else 1] + list(d) + [mp.SIDE] + list(corners[i]) + list(want[i]) + [rms[i]]
                f.write(" ".join(repr(float(v)) if not isinstance(v, int) else str(v) for v in row) + "\n")
    exe = str(tmp_path / "marker_pose_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + SOURCES + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "marker pose driver: ok" in r.stdout and "over 180 cases" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]

