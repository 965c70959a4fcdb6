"""The ctypes calls of every problem class of gunrockinst_amd.capi, replayed against a recording stand-in for the library and
compared with tests/golden/capi_call_log.json: which symbol each method calls, with which arguments, what it returns, which
attributes it leaves on the handle and what it raises when the library refuses.  Needs neither the library nor a GPU.

`python tests/test_capi_calls_cpu.py --record` rewrites the golden file from the capi.py in the tree.

Argument forms in the log: ints, floats, bytes and None as they are; byref(x) and pointer objects as the name of their ctypes
type; a c_void_p as its value ("host" for the address of a host array, which differs from run to run).  Results: scalars as
"type:value", arrays as dtype and shape, never their contents."""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gunrockinst_amd import capi  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "capi_call_log.json")

# the symbols that return a count (or a negated code) instead of a code
COUNT_SYMBOLS = {
    "grx_bfs_level_trace", "grx_mst_round_trace", "grx_mis_round_trace", "grx_kcore_level_trace", "grx_kcore_shells",
    "grx_truss_level_trace", "grx_truss_edges", "grx_truss_classes", "grx_scc_phase_trace", "grx_scc_condensation",
    "grx_msbfs_level_trace", "grx_bcc_phase_trace", "grx_bcc_edges", "grx_bcc_block_cut", "grx_maxflow_phase_trace",
    "grx_maxflow_pairs", "grx_matching_round_trace", "grx_matching_pairs", "grx_c4_edges", "grx_lp_round_trace",
    "grx_wl_round_trace"}
COUNT = 3
HANDLE = 0x1000
ALL_CALLS_CODE = -2  # the refusal pass in which every call fails
FIRST_CALL_CODES = (-1, 1, -4, -5, -6, -7, -8)  # the refusal passes in which the first call of a method returns the code


def _norm_arg(a):
    if a is None or isinstance(a, (int, float, bytes)):
        return a.decode() if isinstance(a, bytes) else a
    if type(a).__name__ == "CArgObject":  # byref(x)
        return type(a._obj).__name__
    if isinstance(a, C.c_void_p):
        return a.value if a.value is None or a.value < (1 << 32) else "host"
    return type(a).__name__


class Recorder:
    """Stands in for the loaded library: every attribute is a function that logs its call, writes a non-zero value that depends
    on the argument's position into every scalar passed by reference and every fixed-length array, and returns 0, COUNT for the
    counting symbols, or the refusal code that is armed."""

    def __init__(self):
        self.log = []
        self.code = None
        self.first_only = False

    def arm(self, code, first_only):
        self.code, self.first_only = code, first_only

    def __getattr__(self, symbol):
        if not symbol.startswith(("grx_", "gunrock_")):
            raise AttributeError(symbol)

        def call(*args):
            self.log.append([symbol, [_norm_arg(a) for a in args]])
            for i, a in enumerate(args):  # values that depend on the position: two fields swapped in a declaration show
                if type(a).__name__ == "CArgObject":
                    x = a._obj
                    x.value = i + (HANDLE if isinstance(x, C.c_void_p) else 1.5 if isinstance(x, (C.c_float, C.c_double)) else COUNT)
                elif isinstance(a, C.Array):
                    a[:] = [10 * i + j for j in range(len(a))]
            if self.code is not None:
                code = self.code
                if self.first_only:
                    self.code = None
                return code
            return COUNT if symbol in COUNT_SYMBOLS else 0
        return call


def _norm(x, owner=None):
    if x is None:
        return None
    if owner is not None and x is owner:
        return "self"
    if isinstance(x, np.ndarray):
        return {"array": x.dtype.name, "shape": list(x.shape)}
    if isinstance(x, dict):
        return {"dict": {k: _norm(v, owner) for k, v in sorted(x.items())}}
    if isinstance(x, (tuple, list)):
        return {type(x).__name__: [_norm(v, owner) for v in x]}
    if isinstance(x, (bool, int, float, str)) or isinstance(x, np.generic):
        return "%s:%r" % (type(x).__name__, x.item() if isinstance(x, np.generic) else x)
    return type(x).__name__


def _attrs(p):
    return {k: _norm(v) for k, v in sorted(vars(p).items()) if not k.startswith("_")}


# the 3-vertex path 0 - 1 - 2, both directions, and made-up device addresses
RO, CI = [0, 1, 3, 4], [1, 0, 2, 1]
W4, V3 = [5, 6, 6, 5], [2, 0, 1]
D_RO, D_CI, D_W, D_IRO, D_ICI, D_X = 0x100, 0x200, 0x300, 0x400, 0x500, 0x600


def S(name, *args, **kwargs):
    return name, args, kwargs


def _common(option="wave_min_row"):
    return [S("set_option", option, 2), S("reset"), S("enact"), S("enact", 7), S("stats"), S("device_results")]


# per class: scripts, each a constructor step and the method steps of one handle, closed at its end
SCRIPTS = {
    "BfsProblem": [
        [S("__init__", True, True, True, 1), S("init", 3, RO, CI), S("set_inverse_graph"), S("set_inverse_graph", D_IRO, D_ICI, 0.5, 0.25),
         S("auto_inverse"), S("auto_inverse", False), S("set_tuning"), S("set_tuning", 1.0, 2.0, 3.0, 4), S("set_head_pass"),
         S("set_head_pass", 1, 2), S("set_option", "fused_publish", 1), S("set_label_deferral"), S("set_label_deferral", 1, 2),
         S("set_binned_min_edges", 9), S("set_cooperative_launch"), S("set_cooperative_launch", False), S("set_persistent_limit", 8),
         S("set_twc_limit", 7), S("reset", 1), S("reset", 1, 2.0), S("enact", 1), S("enact", 1, 7, 2), S("stats"), S("level_trace"),
         S("level_trace", 8), S("extract"), S("device_results"), S("mask_flushes"), S("fused_publications"), S("stream_idle"),
         S("relabel_info")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI), S("extract")]],
    "CcProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("reset"), S("enact"), S("enact", 7), S("stats"), S("extract"), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "MstProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI, W4), S("reset"), S("enact"), S("enact", 7), S("stats"), S("round_trace"),
         S("round_trace", 8), S("extract"), S("extract", False), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init", 2, RO, CI, W4)]],
    "MisProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_tail"), S("set_tail", False), S("reset"), S("enact"), S("enact", 2, 7),
         S("stats"), S("round_trace"), S("round_trace", 8), S("extract"), S("extract", False), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, V3, 0x1FFFFFFFF)],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_X, 5)]],
    "TcProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "strategy", 2), S("reset"), S("enact"), S("enact", 7), S("stats"),
         S("extract"), S("extract", False), S("clustering"), S("clustering", False), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init", 2, RO, CI)]],
    "KcoreProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "schedule", 1), S("reset"), S("enact"), S("enact", 2, 7), S("stats"),
         S("level_trace"), S("extract"), S("extract", False), S("shells"), S("members", 1), S("members", 1, False), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "TrussProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "schedule", 1), S("reset"), S("enact"), S("enact", 2, 7), S("stats"),
         S("level_trace"), S("edges"), S("support"), S("extract"), S("extract", False), S("classes"), S("members", 1),
         S("members", 1, False), S("vertex_truss"), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "SccProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI)] + _common() + [S("phase_trace"), S("extract"), S("extract", False), S("summary"),
         S("sizes"), S("condensation"), S("condensation", 0), S("condensation", 2)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_IRO, D_ICI)]],
    "BccProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI)] + _common() + [S("phase_trace"), S("edges"), S("extract"), S("summary"),
         S("block_cut"), S("block_cut", 0), S("block_cut", 2)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "MaxflowProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "max_rounds", 2), S("reset", 0, 2), S("enact"), S("enact", 7),
         S("stats"), S("phase_trace"), S("pairs"), S("extract"), S("arc_flow"), S("summary"), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W)]],
    "MatchingProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI)] + _common() + [S("round_trace"), S("pairs"), S("extract"), S("summary"),
         S("contract"), S("contract", D_X), S("contract", [1, 2]), S("contract", V3), S("coarse_extract"), S("coarse_device")],
        [S("__init__"), S("init", 3, RO, CI, W4, 0x1FFFFFFFF)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W, 5)]],
    "CliqueProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "strategy", 1), S("reset"), S("enact", 3), S("enact", 4, 7),
         S("stats"), S("extract"), S("extract", False), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_X)]],
    "C4Problem": [
        [S("__init__", True, 1), S("init", 3, RO, CI)] + _common("edges") + [S("extract"), S("extract", False), S("edges"),
         S("extract_edges")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "RwProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "length", 4), S("set_option", "seed", 9), S("reset", [0, 2]),
         S("enact"), S("enact", 7), S("stats"), S("extract"), S("extract", False, False, True), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W)]],
    "SampleProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "seed", 9), S("set_fanouts", [2, -1]), S("reset", [0, 2]),
         S("enact"), S("enact", 7), S("stats"), S("sizes"), S("extract"), S("extract", False), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W)]],
    "SimProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "metric", 1), S("reset"), S("pairs", [0, 1], [2, 2]),
         S("pairs", [0, 1], [2, 2], 7), S("pairs", [0, 1], [2]), S("extract_pairs"), S("pairs_device", 2, D_X, D_W),
         S("pairs_device", 2, D_X, D_W, 7), S("topk", [0, 2], 2), S("topk", [0, 2], 2, 7), S("extract_topk"),
         S("topk_device", 2, D_X, 2), S("topk_device", 2, D_X, 2, 7), S("stats"), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "SpgemmProblem": [
        [S("__init__", True, 1), S("init", (3, 3), RO, CI), S("set_right", (3, 3), RO, CI), S("set_right", (3, 3), RO, CI, W4),
         S("set_right_device", (3, 3), 4, D_RO, D_CI), S("set_right_device", (3, 3), 4, D_RO, D_CI, D_W), S("set_option", "right", 2),
         S("reset"), S("enact"), S("enact", 7), S("stats"), S("sizes"), S("extract"), S("extract", False), S("device_results")],
        [S("__init__"), S("init", (3, 3), RO, CI, W4)],
        [S("__init__"), S("init", (3, 3), RO, CI, V3)],
        [S("__init__"), S("init_device", (3, 3), 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", (3, 3), 4, D_RO, D_CI, D_W)]],
    "LpProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_classes", [0, 1, 0]), S("set_classes", [0, 1, 0], 4), S("set_classes", [0, 1]),
         S("set_option", "mode", 1), S("reset"), S("reset", V3), S("reset", W4), S("enact"), S("enact", 7), S("stats"), S("round_trace"),
         S("extract"), S("summary"), S("device_results")],
        [S("__init__"), S("init", 3, RO, CI, W4)],
        [S("__init__"), S("init", 3, RO, CI, V3)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W)]],
    "WlProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "history", 1), S("reset"), S("reset", V3), S("reset", W4), S("enact"),
         S("enact", 7), S("stats"), S("round_trace"), S("extract"), S("history"), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "MsbfsProblem": [
        [S("__init__", True, 1), S("init", 3, RO, CI), S("set_option", "direction", 1), S("reset", [0, 2, 2]), S("reset", [1], False),
         S("enact"), S("enact", 7), S("stats"), S("level_trace"), S("depths"), S("depths", 1, 1), S("source_summary"),
         S("vertex_summary"), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_IRO, D_ICI)]],
    "PrProblem": [
        [S("__init__", 1), S("init", 3, RO, CI), S("set_inverse_graph"), S("set_inverse_graph", D_IRO, D_ICI), S("set_inverse_graph", build=True),
         S("reset"), S("reset", 1, 0.5, 0.25), S("enact"), S("enact", 5, 7), S("stats"), S("extract"), S("extract", 2), S("device_results")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "BcProblem": [
        [S("__init__", 1), S("init", 3, RO, CI), S("run"), S("run", 1, 7, 2.0), S("extract")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI)]],
    "SsspProblem": [
        [S("__init__", True, True, 1), S("init", 3, RO, CI, W4), S("set_inverse_graph"), S("set_inverse_graph", D_IRO, D_ICI, D_X, 9),
         S("pull_levels"), S("reset", 1), S("reset", 1, 2.0), S("enact", 1), S("enact", 1, 7), S("stats"), S("extract")],
        [S("__init__"), S("init", 3, RO, CI, W4, 8), S("extract")],
        [S("__init__"), S("init_device", 3, 4, D_RO, D_CI, D_W, 2.5)]],
}


def _call(p, step):
    name, args, kwargs = step
    try:
        return _norm(getattr(p, name)(*args, **kwargs), p)
    except Exception as e:  # the refusal is what is recorded
        return "raises %s: %s" % (type(e).__name__, e)


def _make(cls, step):
    return cls(*step[1], **step[2])


def _label(step):
    return "%s(%s)" % (step[0], ", ".join([repr(a) for a in step[1]] + ["%s=%r" % kv for kv in sorted(step[2].items())]))


def _refusals(rec, cls, script, j):
    """what step j does when the library refuses: {outcome with the code written as N: [codes]}"""
    out = {}
    for code, first_only in [(ALL_CALLS_CODE, False)] + [(c, True) for c in FIRST_CALL_CODES]:
        rec.arm(None, False)
        if j == 0:
            rec.arm(code, first_only)
            try:
                _make(cls, script[0]).close()
                got = "constructed"
            except Exception as e:
                got = "raises %s: %s" % (type(e).__name__, e)
        else:
            p = _make(cls, script[0])
            for step in script[1:j]:
                _call(p, step)
            rec.arm(code, first_only)
            got = _call(p, script[j])
            got = got if isinstance(got, str) else json.dumps(got, sort_keys=True)
            rec.arm(None, False)
            p.close()
        rec.arm(None, False)
        out.setdefault(got.replace("(code %d)" % code, "(code N)"), []).append(code)
    return out


def replay():
    """every script against a fresh recorder: {class: [[{"call", "log", "result", "attrs", "refused"} per step] per script]}"""
    saved = capi._LIB
    rec = capi._LIB = Recorder()
    try:
        record = {}
        for name, scripts in sorted(SCRIPTS.items()):
            cls = getattr(capi, name)
            record[name] = []
            for script in scripts:
                steps = []
                rec.log = []
                p = _make(cls, script[0])
                for j, step in enumerate(list(script) + [S("close")]):
                    result = "self" if j == 0 else _call(p, step)
                    steps.append({"call": _label(step), "log": rec.log, "result": result, "attrs": _attrs(p)})
                    rec.log = []
                for j, step in enumerate(script):
                    steps[j]["refused"] = _refusals(rec, cls, script, j)
                    rec.log = []
                record[name].append(steps)
        return record
    finally:
        gc.collect()  # a handle dropped without close() destroys itself: let it do so while the stand-in is installed
        capi._LIB = saved


def _write(record):
    with open(GOLDEN_FILE, "w") as f:
        f.write("{\n")
        names = sorted(record)
        for i, name in enumerate(names):
            f.write(" %s: [\n" % json.dumps(name))
            for k, steps in enumerate(record[name]):
                f.write("  [\n" + ",\n".join("   " + json.dumps(s, sort_keys=True) for s in steps) + "\n  ]%s\n" % ("," if k + 1 < len(record[name]) else ""))
            f.write(" ]%s\n" % ("," if i + 1 < len(names) else ""))
        f.write("}\n")


def _problem_classes():
    return {name: c for name, c in vars(capi).items()
            if isinstance(c, type) and issubclass(c, capi._Handle) and c not in (capi._Handle, capi.HostGraph) and not name.startswith("_")}


def test_every_public_method_of_every_problem_class_is_driven():
    classes = _problem_classes()
    assert sorted(classes) == sorted(SCRIPTS) and len(classes) == 23
    for name, cls in classes.items():
        public = {m for m in dir(cls) if not m.startswith("_") and callable(getattr(cls, m))} | {"__init__"}
        driven = {step[0] for script in SCRIPTS[name] for step in script} | {"close"}
        assert public == driven, (name, public ^ driven)


def test_calls_results_and_refusals_match_the_recorded_log():
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(replay()))
    assert sorted(got) == sorted(golden)
    for name in sorted(got):
        assert len(got[name]) == len(golden[name]), name
        for k, (steps, want) in enumerate(zip(got[name], golden[name])):
            assert [s["call"] for s in steps] == [s["call"] for s in want], (name, k)
            for s, w in zip(steps, want):
                for part in ("log", "result", "attrs", "refused"):
                    assert s.get(part) == w.get(part), "%s script %d, %s: %s differs\n got  %r\n want %r" % (
                        name, k, s["call"], part, s.get(part), w.get(part))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_capi_calls_cpu.py --record")
    _write(replay())
    print("wrote %s (%d bytes)" % (GOLDEN_FILE, os.path.getsize(GOLDEN_FILE)))
