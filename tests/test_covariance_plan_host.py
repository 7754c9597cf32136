"""The host-only plan of the covariance (csrc/ba_covariance_plan.hpp) under the host sanitizers: tests/covariance_plan_driver.cpp, a
stand-alone program, is compiled with -fsanitize=address,undefined and run as a child process.  From the problem alone it checks what
the kernels rely on — the column map (which blocks get columns and where, the eliminated times, a sharded solver's summed flags), the
marker chain's rows in stable time order with their observations, weights and 18-bit masks, the cross tables of the time-eliminating
path with their block cap, and, end to end, offset resolution and the pair plan: the driver plays the kernels on a known symmetric
matrix and every ordered pair of offsets must unpack to that matrix's block, beside the return codes of the single-pair call.  Cases:
the hongo wiring on both paths and both model variants, a rig with constant blocks, masks, weights, a time without rows and
unreferenced blocks, the point model with a point order, constant points and a second rank's cameras, the empty problem and one
observation.  Nothing loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")


def test_covariance_plan_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "covariance_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "covariance_plan_driver.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "hongo", "correspondence.txt")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "covariance plan driver: ok" in r.stdout and "hongo: 68 observations checked" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
