"""The plan of subgraph matching (csrc/gunrock/app/sm/sm_plan.hpp): |Aut(H)| and the symmetry-breaking constraints of the named
patterns, the matching orders, the masks of a house, every refusal and, by a host search over the plan's levels on a fixed 10-vertex
graph, constrained count x aut == unconstrained count == the count of a search that knows nothing of the plan, for every connected
pattern of up to 5 vertices.  tests/host/sm_check.hip is a stand-alone program built with the address and undefined-behaviour
sanitizers on the host side.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"


def test_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sm_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-value",
                            "-Wno-unused-function", "-Xarch_host", SANITIZE, "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "gunrockinst_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "sm_check.hip"), SANITIZE, "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sm host checks passed" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
