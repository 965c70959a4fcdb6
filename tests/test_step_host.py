"""csrc/gunrock/oprtr/step.hpp and csrc/gunrock/app/step_host.hpp on the host: tests/host/step_check.hip pins the pieces that
make no GPU call (the tile rule, Narrow and the limits a schedule gives, the parsing of the four loop options and its ABI codes,
the grids of a step) to values that follow from their formulas, as a stand-alone program built with the address and
undefined-behaviour sanitizers on the host side, so an option value that no integer holds or a free of what was never made ends
the program with a report.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"


def test_host_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Xarch_host", SANITIZE,
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                            "-I", os.path.join(ROOT, "gunrockinst_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "step_check.hip"), SANITIZE, "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "step host checks passed" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
