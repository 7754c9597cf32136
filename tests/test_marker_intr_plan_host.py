"""The host-only plan of the marker chain's time elimination WITH intrinsics blocks (csrc/ba_marker_plan.hpp, PlanMarkerChain's last
argument: schur_impl = 3) under the host sanitizers: tests/marker_intr_plan_driver.cpp, a stand-alone program, is compiled with
-fsanitize=address,undefined and run as a child process.  The driver builds every case itself — 3 x 12 x 4 with masks [0x3F] * 3 and
[0x0F, 0, 0x33], a constant camera pose with a free block, Test2's wiring, sparse detections, a time at the width limit, 2 x 1400 x 2,
T = 1, one camera — and checks the column order, the third slot of every residual block, ascending slot lists, that every (residual
block, pair kind) lies in exactly one pair item of its chunk, the held components, the width refusals, and that with no mask set or
without the opt-in every table is byte-identical to the plan without intrinsics.  Nothing loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
SWITCHES = ("RSBA_MT_SPLIT", "RSBA_MT_ACC_MFMA", "RSBA_MT_CHUNKS", "RSBA_MT_BACKSUB_WG", "RSBA_MT_SPLIT_BACKSUB", "RSBA_MT_FORK", "RSBA_MT_SOLVE_LDS",
            "RSBA_CHOL_TILES", "RSBA_DEBUG")


def test_plan_with_intrinsics_blocks_keeps_its_contracts(tmp_path):
    exe = str(tmp_path / "marker_intr_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "marker_intr_plan_driver.cpp"), "-o", exe])
    child = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=child, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "marker intr plan driver: ok" in r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
