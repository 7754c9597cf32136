"""The host plans behind the queries of a solver with free intrinsics under the extended layout — PlanEvalMarkerIntr
(csrc/ba_evaluate_plan.cpp) and CovMarkerIntrColumns / CovPlanMarkerIntrRows (csrc/ba_covariance_plan.hpp) — under the host sanitizers:
tests/marker_intr_query_plan_driver.cpp, a stand-alone program with its own main, is compiled with -fsanitize=address,undefined and
run as a child process.  It checks the extended block lists (every detection once in its camera's list, ascending, through the
(obs, slot) encoding the sum kernel decodes, never past the J'r buffer), the live and held masks, the intrinsics blocks' columns and
the resolution of their offsets, on a seeded random rig with an undetected camera, one observation and the empty problem.  Nothing
loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")


def test_marker_intr_query_plan_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "marker_intr_query_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "marker_intr_query_plan_driver.cpp"), os.path.join(CSRC, "ba_evaluate_plan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "marker intrinsics query plan driver: ok" in r.stdout and "random rig: " in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
