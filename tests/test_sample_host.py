"""The host side of the neighbourhood sampling (csrc/gunrock/app/sample/sample_enactor.hpp's SampleOptions and the __host__ __device__
functions of sample_functor.hpp): tests/host/sample_check.hip pins the option parsing and its ABI codes, the fanout and hop validation,
the group-width and count formulas, the strategy AUTO picks, and the host side of Floyd's subset against the literals
tests/test_sample_cpu.py pins, as a stand-alone program built with the address and undefined-behaviour sanitizers on the host side.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"


def test_host_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sample_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-value",
                            "-Xarch_host", SANITIZE, "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                            "-I", os.path.join(ROOT, "gunrockinst_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "sample_check.hip"), SANITIZE, "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sample host checks passed" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
