"""CPU: the numpy restatement of the comparison of two predictions (tests/audit_ref.py; include/ethcnn.h "comparing two predictions")
against what the suite already trusts -- the partition decisions (decide_ref) and the simulator (sim_ref) -- and against the edge
cases of the definition worked out by hand; plus what the feature settles without a GPU: the struct layouts, the bindings, the tool's
and the launchers' argument handling."""
import os
import subprocess
import sys

import numpy as np
import pytest

import audit_ref as ref
import calib_ref
import decide_ref
import sim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "audit_plan.py")
NATIVE = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "video_to_cu_depth")
BAD_AUDIT_VALUES = ("x", "-1", "+4", "2.5", "1e3", " 4", "4 ", "4\n", "0x4", "1234567")   # both launchers refuse exactly these forms


def _two_sides(rng, n):
    """a, and b = a with a third of its values drawn afresh and a few moved by one ulp: no rejected CTU"""
    a = calib_ref.edge_probs(rng, n)
    b = ref.perturbed(rng, a, ulp_share=0.1, big_share=0.1, big=1e-3)
    fresh = rng.integers(0, 3, size=b.shape) == 0
    b = np.where(fresh, calib_ref.edge_probs(rng, n), b).astype(np.float32)
    return a, b


@pytest.mark.parametrize("layout", ["per-ctu", "frame"])
def test_restatement_against_decisions_and_simulator(layout):
    """500 random CTUs, 12 candidates: search_diff_ctus = the CTUs whose decide codes differ between the sides, checked_a / checked_b =
    the simulator's checked[].  The frame is 1272 x 1592: 20 x 25 CTUs, the last column 56 wide and the last row 56 high."""
    rng = np.random.default_rng(41)
    a, b = _two_sides(rng, 500)
    w, h = (1272, 1592) if layout == "frame" else (None, None)
    sets = sim_ref.Set(), sim_ref.Set()
    for s, p in zip(sets, (a, b)):
        if layout == "frame":
            s.add_frames(p, None, w, h)
        else:
            s.add(p)
        assert s.info()["rejected_ctus"] == 0
    seen = 0
    for cand in decide_ref.candidates(rng, 12):
        got = ref.compare(a, b, 1e-4, cand, w, h)
        codes = [decide_ref.decide(s, cand)["codes"] for s in sets]
        want = int((codes[0] != codes[1]).any(axis=1).sum())
        assert got["search_diff_ctus"] == want
        seen += want
        for side, s in zip(("checked_a", "checked_b"), sets):
            assert got[side] == [int(x) for x in s.evaluate(cand)[0]["checked"]]
        assert np.array_equal((got["flags"] & ref.SEARCH) != 0, (codes[0] != codes[1]).any(axis=1))
    assert seen > 500  # not vacuous: searches do differ


@pytest.mark.parametrize("case", ref.crafted_cases(), ids=lambda c: c["name"])
def test_edge_cases_of_the_definition(case):
    got = ref.compare(case["a"], case["b"], case["tol"], case["thr"], case["width"], case["height"])
    for field, want in case["expect"].items():
        assert got[field] == want, field
    if case["name"] == "rejected on one side":
        assert got["flags"].tolist() == [0, ref.REJECTED, ref.OVER_TOL]
    if case["name"] == "200 x 136":  # partial CTUs on both edges: the searches visit frame-edge nodes, and something differs on every count
        assert got["rejected_ctus"] == 0 and got["search_diff_ctus"] > 0 and min(got["class_diff"][1:]) > 0 and min(got["over_tol"]) > 0
        sets = sim_ref.Set(), sim_ref.Set()
        for s, p in zip(sets, (case["a"], case["b"])):
            s.add_frames(p, None, 200, 136)
        assert got["checked_a"] == [int(x) for x in sets[0].evaluate(case["thr"])[0]["checked"]]
        assert sets[0].evaluate(case["thr"])[0]["edge_split"].sum() > 0


def test_split_rule():
    """the stats of a set = those of its parts combined: sums add, a maximum goes by (value, lowest index)"""
    rng = np.random.default_rng(43)
    a, b = _two_sides(rng, 301)
    cand = decide_ref.candidates(rng, 4)[0]
    whole = ref.compare(a, b, 1e-4, cand)
    for cut in (1, 77, 300):
        parts = ref.compare(a[:cut], b[:cut], 1e-4, cand), ref.compare(a[cut:], b[cut:], 1e-4, cand)
        assert ref.stats_equal(ref.combine(*parts), whole), ref.mismatch(ref.combine(*parts), whole)
    # a tie across the cut: the first part's index wins
    a2 = np.full((4, 21), np.float32(0.5), np.float32)
    b2 = a2.copy()
    b2[1, 0] = b2[3, 0] = np.float32(0.75)
    parts = ref.compare(a2[:2], b2[:2], 1e-4), ref.compare(a2[2:], b2[2:], 1e-4)
    assert ref.combine(*parts)["worst_ctu"] == [1, 0, 0] == ref.compare(a2, b2, 1e-4)["worst_ctu"]
    empty = ref.compare(a2[:0], b2[:0], 1e-4)
    assert empty["worst_ctu"] == [-1, -1, -1] and ref.stats_equal(ref.combine(empty, parts[0]), parts[0])


def test_struct_layouts_and_bindings(pkg, tmp_path):
    """the sizes and offsets the header states are those of the C structs and of the binding's dtypes; every new entry is declared,
    exported and bound"""
    e = pkg.ethcnn
    fields = ("ctus", "rejected_ctus", "over_tol", "bits_diff", "class_diff", "search_diff_ctus", "checked_a", "checked_b", "worst_ctu", "max_abs", "with_thr")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ethcnn.h"\nint main(void) {\n  printf("%zu %zu", sizeof(ethcnn_compare_stats), '
                   'sizeof(ethcnn_audit_result));\n' +
                   "".join('  printf(" %%zu", offsetof(ethcnn_compare_stats, %s));\n' % f for f in fields) +
                   "".join('  printf(" %%zu", offsetof(ethcnn_audit_result, %s));\n' % f for f in ("plan", "passes", "fast_passes", "reserved")) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [200, 216, 0, 8, 16, 40, 64, 88, 96, 128, 160, 184, 196, 200, 204, 208, 212]
    assert e.COMPARE_STATS.itemsize == 200 and e.AUDIT_RESULT.itemsize == 216
    assert [e.COMPARE_STATS.fields[f][1] for f in fields] == got[2:13]
    assert [e.AUDIT_RESULT.fields[f][1] for f in ("stats", "plan", "passes", "fast_passes", "reserved")] == [0] + got[13:]
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    lib = pkg.load_library()
    for name in ("ethcnn_compare_probs", "ethcnn_compare_probs_device", "ethcnn_compare_frames", "ethcnn_compare_frames_device", "ethcnn_audit_plan_bytes",
                 "ethcnn_audit_plan_device", "ethcnn_audit_plan_yuv_file"):
        assert name + "(" in header and getattr(lib, name) and name in e.SIGNATURES
    # two sets of 5 x 510 x 84 = 214,200 bytes, the first rounded up to 16 so that the second starts aligned
    assert lib.ethcnn_audit_plan_bytes(1920, 1088, 5) == 214208 + 214200 and lib.ethcnn_audit_plan_bytes(1920, 1088, 4) == 2 * 4 * 510 * 84
    assert lib.ethcnn_audit_plan_bytes(0, 64, 1) < 0


def test_thr_info_on_the_grid(pkg, tmp_path):
    e = pkg.ethcnn
    p = tmp_path / "Thr_info.txt"
    p.write_text("0.75 0.25 0.5 0.4 1.0 0.0\n")
    assert e.read_thr_info_k(str(p), "ai") == ([768, 512, 1024], [256, 410, 0])
    assert e.read_thr_info_k(str(p), "ldp") == ([256, 410, 0], [768, 512, 1024])
    for text in ("0.5 0.5 0.5", "0.5 0.5 0.5 0.5 0.5 1.5", "a b c d e f"):
        p.write_text(text)
        with pytest.raises(ValueError):
            e.read_thr_info_k(str(p), "ai")


def test_tool_refuses_bad_arguments_before_a_context(tmp_path):
    """exit status 1 and no GPU touched: this machine may have none, and the tool must say so only after its arguments are in order"""
    good = tmp_path / "a.dat"
    np.zeros(12 * 21, "<f4").tofile(str(good))
    short = tmp_path / "b.dat"
    np.zeros(11 * 21, "<f4").tofile(str(short))
    thr = tmp_path / "Thr_info.txt"
    thr.write_text("0.5 0.5 0.5\n")
    for argv in ([], ["--case", good, good, 200], ["--case", good, good, 100, 136], ["--case", good, short, 200, 136], ["--case", good, tmp_path / "absent.dat", 200, 136],
                 ["--case", good, good, 200, 136, "--plan", 3], ["--case", good, good, 200, 136, "--tol", "x"], ["--case", good, good, 200, 136, "--tol", -1],
                 ["--case", good, good, 200, 136, "--thr-info", thr], ["--case", good, good, 200, 136, "--thr-info", thr, "--order", "ai"],
                 ["--yuv", good, 200, 136, 32], ["--yuv", good, 200, 136, 32, "--plan", 1, "--model-dir", "."], ["--yuv", good, 200, 136, 32, "--plan", 3, "--model-dir", ".", "--step", 0],
                 ["--yuv", good, 200, 136, 32, "--plan", 3, "--model-dir", ".", "--flags-out", "f"], ["--case", good, good, 200, 136, "--yuv", good, 200, 136, 32]):
        r = subprocess.run([sys.executable, TOOL] + [str(x) for x in argv], capture_output=True, text=True, env=dict(os.environ, ETHCNN_LIB="/nonexistent/libethcnn.so"))
        assert r.returncode == 1 and r.stderr and "Traceback" not in r.stderr, (argv, r.stderr)


def test_launcher_reads_the_audit_variable_only_beside_a_plan(pkg, monkeypatch):
    v = pkg.video_to_cu_depth
    monkeypatch.delenv("ETHCNN_DEVICES", raising=False)
    monkeypatch.delenv("ETHCNN_FC1_PLAN", raising=False)
    monkeypatch.setenv("ETHCNN_FC1_PLAN_AUDIT", "x")
    assert v.plan_audit_from_env() == 0              # no plan: not read
    monkeypatch.setenv("ETHCNN_FC1_PLAN", "3")
    for bad in BAD_AUDIT_VALUES:
        monkeypatch.setenv("ETHCNN_FC1_PLAN_AUDIT", bad)
        with pytest.raises(ValueError):
            v.plan_audit_from_env()
    monkeypatch.setenv("ETHCNN_FC1_PLAN_AUDIT", "4")
    assert v.plan_audit_from_env() == 4
    with pytest.raises(ValueError):
        v.plan_audit_from_env((10, 420))
    monkeypatch.setenv("ETHCNN_DEVICES", "0,1")
    with pytest.raises(ValueError):
        v.plan_audit_from_env()
    monkeypatch.setenv("ETHCNN_FC1_PLAN_AUDIT", "0")
    assert v.plan_audit_from_env((10, 420)) == 0
    monkeypatch.setenv("ETHCNN_FC1_PLAN_AUDIT", "")
    assert v.plan_audit_from_env() == 0


def test_native_launcher_parses_the_audit_variable_like_the_python_one(pkg, tmp_path):
    """the native launcher refuses a malformed value before it creates a context (exit status 1, the variable named, nothing written);
    a well-formed one gets past the parsing (what stops the run then -- no file, no GPU -- does not name the variable), and without
    ETHCNN_FC1_PLAN the variable is not read"""
    def run(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
        e.update(env)
        return subprocess.run([NATIVE, "absent.yuv", "64", "64", "32"], cwd=str(tmp_path), capture_output=True, text=True, env=e)

    for bad in BAD_AUDIT_VALUES:
        r = run(ETHCNN_FC1_PLAN="3", ETHCNN_FC1_PLAN_AUDIT=bad)
        assert r.returncode == 1 and "ETHCNN_FC1_PLAN_AUDIT" in r.stderr, (bad, r.stderr)
    for good in ("0", "4", "007", "999999"):
        r = run(ETHCNN_FC1_PLAN="3", ETHCNN_FC1_PLAN_AUDIT=good)
        assert r.returncode == 1 and "ETHCNN_FC1_PLAN_AUDIT" not in r.stderr, (good, r.stderr)
    r = run(ETHCNN_FC1_PLAN_AUDIT="x")
    assert "ETHCNN_FC1_PLAN_AUDIT" not in r.stderr
    assert not os.listdir(str(tmp_path))
    for extra in ({"ETHCNN_DEVICES": "0,1"}, {"ETHCNN_INPUT_BIT_DEPTH": "10"}):   # an audit on two devices, or of a deep source, is refused
        r = run(ETHCNN_FC1_PLAN="3", ETHCNN_FC1_PLAN_AUDIT="4", **extra)
        assert r.returncode == 1 and "ETHCNN_FC1_PLAN_AUDIT" in r.stderr, extra
