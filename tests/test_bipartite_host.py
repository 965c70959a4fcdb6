"""The host side of the bipartite matching (csrc/gunrock/app/bipartite): the options with their ranges and ABI codes, the lane / wave
/ workgroup split of a frontier column, the layout of the pinned read-back buffer and the narrow-or-wide decision for a level.
tests/host/bipartite_check.hip pins them to values that follow from their formulas, as a stand-alone program built with the address
and undefined-behaviour sanitizers on the host side.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"


def test_host_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bipartite_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-value",
                            "-Wno-unused-function", "-Xarch_host", SANITIZE, "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "gunrockinst_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "bipartite_check.hip"), SANITIZE, "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "bipartite host checks passed" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
