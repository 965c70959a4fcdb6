"""csrc/gunrock/app/handle_runner.hpp on the host: tests/host/handle_runner_check.hip exercises the pieces that make no GPU call
(the borrowed CSR, the init state and its ABI codes, the trace copy-out) as a stand-alone program built with the address and
undefined-behaviour sanitizers on the host side, so a free of a caller's array, a read after one or a store past an output array
ends the program with a report.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"


def test_host_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "handle_runner_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Xarch_host", SANITIZE,
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                            "-I", os.path.join(ROOT, "gunrockinst_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "handle_runner_check.hip"), SANITIZE, "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "handle_runner host checks passed" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
