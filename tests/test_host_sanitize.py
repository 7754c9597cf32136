"""Sanitizer builds of the host side of librsba (the reference has no sanitizer runs; this project's host
code gets them).  ba_problem.cpp, rsba_capi.cpp, ba_initial_guess.cpp and ba_schur_plan.cpp are compiled with
-fsanitize=address,undefined together with tests/host_sanitize_driver.cpp, which walks the file readers (committed
fixtures, short / malformed / out-of-range inputs), the accessors one past either end, the writers, the front end's pose
algebra / EPnP, and the planning of the point model's set-up: layouts and Schur work lists for synthetic visibilities,
checked against the contracts the kernels rely on.  A second build with -fsanitize=thread runs the planning section alone:
its point dealing writes one shared counter array from up to eight threads.  GPU sanitizers are not available on the pool;
the kernels are not in these builds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host_sanitize_driver.cpp")] + [os.path.join(CSRC, f) for f in ("ba_problem.cpp", "rsba_capi.cpp", "ba_initial_guess.cpp", "ba_schur_plan.cpp")]


def _build(exe, sanitize):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + sanitize + ["-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC] +
                          SOURCES + ["-o", exe])


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_sanitize_driver")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    scratch = tmp_path / "out"
    scratch.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden"), str(scratch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host sanitize driver: ok" in r.stdout and "schur plans checked" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]


def test_schur_planning_under_tsan(tmp_path):
    exe = str(tmp_path / "host_sanitize_driver_tsan")
    _build(exe, ["-fsanitize=thread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    r = subprocess.run([exe, "--plans"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host sanitize driver: ok" in r.stdout and "schur plans checked" in r.stdout
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
