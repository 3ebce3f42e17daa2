"""CPU: the host-only part of the search budget (include/ethcnn.h "search budget") -- the default ladder, the companion thresholds and
the per-frame choice of the library against the restatement in tests/budget_ref.py (Python integers) and against the properties the
choice promises -- and the refusals of tools/control_budget.py and of the launcher's budget mode, which come before a GPU is touched.
The kernels and the end-to-end runs are in tests/test_gpu_budget.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import budget_ref as bref
import sim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "control_budget.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
ENTRIES = ("default_ladder", "companion_thr", "choose", "cost", "cost_device", "bake_device", "bake", "control")
MODES = {"frame": bref.FRAME, "carry": bref.CARRY}
M = 10 ** 6


def _random_checked(rng, frames, k, hi, monotone):
    """uint32 [frames, k + 1, 4]; column k (the full search) dominates every rung; monotone: costs fall along the ladder"""
    c = rng.integers(0, hi, size=(frames, k + 1, 4), dtype=np.uint64)
    if monotone:
        c = np.sort(c, axis=1)[:, ::-1]
        c = np.concatenate([c[:, 1:], c[:, :1]], axis=1)
    else:
        c[:, k] = c.max(axis=1)
    c[0, :k] = c[0, k]            # a frame on which nothing saves anything
    if frames > 2:
        c[2] = 0                  # an empty frame: every cost is 0
    return c.astype(np.uint32)


def _same(got, want):
    rung, over, cost, full = want
    assert got["rung"].tolist() == rung and got["over"].astype(int).tolist() == over
    assert [int(x) for x in got["cost"]] == cost and [int(x) for x in got["full"]] == full


def test_default_ladder_and_companion(pkg, tmp_path):
    e = pkg.ethcnn
    lad = e.budget_default_ladder()
    assert lad.dtype == e.SIM_THR and lad.shape == (513,) == (e.BUDGET_DEFAULT_RUNGS,)
    j = np.arange(513)
    for l in range(3):
        assert np.array_equal(lad["up_k"][:, l], 1024 - j) and np.array_equal(lad["down_k"][:, l], j - 1)
    assert np.array_equal(lad, bref.default_ladder())
    assert (lad[0]["up_k"].tolist(), lad[0]["down_k"].tolist()) == tuple(list(x) for x in ref.FULL) == tuple(list(x) for x in e.SIM_FULL_SEARCH)
    assert lad[512]["up_k"].tolist() == [512] * 3 and lad[512]["down_k"].tolist() == [511] * 3   # only bin == 512 is left to "both"
    comp = e.budget_companion_thr()
    assert (comp["up_k"].tolist(), comp["down_k"].tolist()) == tuple(list(x) for x in bref.COMPANION)
    for order, line in (("ai", "0.75 0.25 0.75 0.25 0.75 0.25"), ("ldp", "0.25 0.75 0.25 0.75 0.25 0.75")):
        path = str(tmp_path / ("Thr_%s.txt" % order))
        e.sim_write_thr_info(path, comp, order)
        assert [float(t) for t in open(path).read().split()] == [float(t) for t in line.split()]
    lib = pkg.load_library()
    assert lib.ethcnn_budget_default_ladder(None) == e.ERR_ARG and lib.ethcnn_budget_companion_thr(None) == e.ERR_ARG


@pytest.mark.parametrize("monotone", [True, False])
@pytest.mark.parametrize("k", [1, 3, 64, 513])
def test_choose_agrees_with_the_restatement_and_keeps_its_promises(pkg, k, monotone):
    e = pkg.ethcnn
    rng = np.random.default_rng(1000 * k + monotone)
    checked = _random_checked(rng, 40, k, 5000, monotone)
    weights = (64, 16, 4, 1) if k != 3 else (7, 0, 3, 11)
    costs = (checked.astype(object) * np.array(weights, object)).sum(axis=2)   # Python integers [F, K + 1]
    seen = {"over": 0, "under": 0, "deep": 0, "carried": 0}
    for ppm in (0, 1, 250000, 500000, 999999, M):
        for mode in ("frame", "carry"):
            got = e.budget_choose(checked, weights, ppm, mode)
            _same(got, bref.choose(checked, weights, ppm, MODES[mode]))
            carry = 0
            for f in range(checked.shape[0]):
                r, full = int(got["rung"][f]), int(costs[f, k])
                assert int(got["cost"][f]) == costs[f, r] and int(got["full"][f]) == full
                allow = ppm * full + (carry if mode == "carry" else 0)
                if got["over"][f]:
                    assert all(costs[f, i] * M > allow for i in range(k))              # nothing fits
                    assert costs[f, r] == min(costs[f, :k]) and r == list(costs[f, :k]).index(costs[f, r])
                    carry = 0                                                         # the carry resets after an over-budget frame
                    seen["over"] += 1
                else:
                    assert costs[f, r] * M <= allow and all(costs[f, i] * M > allow for i in range(r))
                    seen["carried"] += mode == "carry" and costs[f, r] * M > ppm * full  # a frame that lives on what others left
                    carry = allow - costs[f, r] * M
                    seen["under"] += 1
                    seen["deep"] += r > 0
            if mode == "carry":  # the cumulative inequality between over-budget frames
                run_cost = run_full = 0
                for f in range(checked.shape[0]):
                    if got["over"][f]:
                        run_cost = run_full = 0
                        continue
                    run_cost, run_full = run_cost + int(got["cost"][f]), run_full + int(got["full"][f])
                    assert run_cost * M <= ppm * run_full
            if ppm == M:
                assert not got["rung"].any() and not got["over"].any()                 # the full budget: the most thorough rung
            if ppm == 0:
                assert np.array_equal(got["over"], np.array([min(costs[f, :k]) > 0 for f in range(checked.shape[0])]))
    assert seen["over"] and seen["under"]
    if k > 1:
        assert seen["deep"] and seen["carried"]


def test_choose_with_weights_near_2_to_32(pkg):
    e = pkg.ethcnn
    rng = np.random.default_rng(32)
    checked = _random_checked(rng, 25, 9, 1 << 30, False)   # counters as large as a frame below 2^24 CTUs can give
    weights = (2 ** 32 - 1, 2 ** 32 - 2, 2 ** 31 + 1, 2 ** 32 - 5)
    assert max(sum(w * int(x) for w, x in zip(weights, c)) for c in checked.reshape(-1, 4)) > 2 ** 62
    for ppm in (0, 333333, M):
        for mode in ("frame", "carry"):
            _same(e.budget_choose(checked, weights, ppm, mode), bref.choose(checked, weights, ppm, MODES[mode]))
    # a cost of 2^64 or more has no place in the outputs: refused
    big = np.full((1, 2, 4), 2 ** 32 - 1, np.uint32)
    with pytest.raises(pkg.EthCnnError) as err:
        e.budget_choose(big, weights, 500000, "frame")
    assert err.value.code == e.ERR_ARG and "64 bits" in str(err.value)
    with pytest.raises(ValueError):
        bref.choose(big, weights, 500000, bref.FRAME)


def test_choose_argument_errors_leave_the_outputs_untouched(pkg):
    e = pkg.ethcnn
    lib = pkg.load_library()
    checked = _random_checked(np.random.default_rng(3), 5, 4, 100, True)
    w = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
    wbig = (ctypes.c_uint64 * 4)(64, 16, 2 ** 32, 1)
    rung, over = np.full(5, -7, np.int32), np.full(5, 9, np.uint8)
    cost, full = np.full(5, 77, np.uint64), np.full(5, 78, np.uint64)
    outs = (rung.ctypes.data, over.ctypes.data, cost.ctypes.data, full.ctypes.data)
    p = checked.ctypes.data
    for args in ((p, 5, 4, w, M + 1, 0), (p, 5, 0, w, 5, 0), (p, 5, 4097, w, 5, 0), (None, 5, 4, w, 5, 0), (p, 5, 4, None, 5, 0), (p, 5, 4, w, 5, 2),
                 (p, 5, 4, w, 5, -1), (p, -1, 4, w, 5, 0), (p, 5, 4, wbig, 5, 1)):
        assert lib.ethcnn_budget_choose(*(args + outs)) == e.ERR_ARG, args[1:]
    assert (rung == -7).all() and (over == 9).all() and (cost == 77).all() and (full == 78).all()
    assert lib.ethcnn_budget_choose(p, 5, 4, w, 500000, 1, None, None, None, None) == 0       # every output may be NULL
    assert lib.ethcnn_budget_choose(None, 0, 4, w, 500000, 1, *outs) == 0 and (rung == -7).all()  # no frames: a no-op
    assert lib.ethcnn_budget_choose(p, 5, 4, w, 500000, 1, *outs) == 0 and (rung >= 0).all()
    for bad in ("both", 2, None):
        with pytest.raises(ValueError):
            e.budget_choose(checked, None, 5, bad)
    with pytest.raises(ValueError):
        e.budget_choose(checked[:, :, :3], None, 5, "frame")


def test_header_library_and_binding_carry_exactly_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "search budget" in header
    declared = set(re.findall(r"\bint (ethcnn_budget_\w+)\(", header))
    assert declared == {"ethcnn_budget_" + n for n in ENTRIES}
    assert set(re.findall(r"\b(ethcnn_budget_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) == declared
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in declared:
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    for const in ("ETHCNN_BUDGET_FRAME = 0", "ETHCNN_BUDGET_CARRY = 1", "ETHCNN_BUDGET_DEFAULT_RUNGS 513", "ETHCNN_BUDGET_MAX_RUNGS 4096"):
        assert const in header
    e = pkg.ethcnn
    assert (e.BUDGET_FRAME, e.BUDGET_CARRY, e.BUDGET_MAX_RUNGS) == (0, 1, 4096)
    for method in ("budget_cost", "budget_cost_device", "budget_bake", "budget_bake_device", "budget_control"):
        assert callable(getattr(pkg.PartitionSim, method))


def _tool(args, cwd):
    return subprocess.run([sys.executable, TOOL] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


def test_tool_refuses_bad_shares_modes_and_ladders_before_a_gpu_is_touched(tmp_path):
    np.zeros((12, 21), "<f4").tofile(str(tmp_path / "p.dat"))
    case = ["--case", "-", "p.dat", "208", "144"]
    (tmp_path / "five.txt").write_text("1 0 1 0 1\n")
    (tmp_path / "high.txt").write_text("1 0 1 0 1 0\n1.5 0 1 0 1 0\n")
    (tmp_path / "word.txt").write_text("1 0 1 0 one 0\n")
    (tmp_path / "empty.txt").write_text("\n")
    for args, word in ((["--budget", "1.5"], "share"), (["--budget", "-0.1"], "share"), (["--budget", "half"], "share"), (["--budget", "nan"], "share"),
                       (["--budget", "0.5", "--mode", "both"], "frame and carry"),
                       (["--budget", "0.5", "--order", "ai", "--ladder", "five.txt"], "line 1"),
                       (["--budget", "0.5", "--order", "ai", "--ladder", "high.txt"], "line 2"),
                       (["--budget", "0.5", "--order", "ai", "--ladder", "word.txt"], "line 1"),
                       (["--budget", "0.5", "--order", "ai", "--ladder", "empty.txt"], "rungs"),
                       (["--budget", "0.5", "--order", "ai", "--ladder", "absent.txt"], "absent.txt"),
                       (["--budget", "0.5", "--weights", "1", "2", "3", "4294967296"], "weights")):
        r = _tool(args + ["--out", "out.dat", "--thr-out", "thr.txt"] + ([] if "--order" in args else ["--order", "ai"]) + case, tmp_path)
        assert r.returncode == 1 and "control_budget.py: error:" in r.stderr and word in r.stderr, (args, r.returncode, r.stderr[-300:])
        assert "Traceback" not in r.stderr
    # a command line of the wrong form: the usage text, status 2, as the sibling tools
    for args in ([], case, ["--budget", "0.5"] + case, ["--budget", "0.5", "--thr-out", "thr.txt"] + case,
                 ["--budget", "0.5", "--out", "out.dat", "--samples", "s.dat", "--model", "m", "--qp", "32"]):
        r = _tool(args, tmp_path)
        assert r.returncode == 2 and "control_budget.py" in r.stderr, (args, r.returncode)
    assert sorted(os.listdir(str(tmp_path))) == ["empty.txt", "five.txt", "high.txt", "p.dat", "word.txt"]  # no output, no temp file


def _launch(cwd, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([sys.executable, LAUNCHER, "seq.yuv", "64", "64", "32"], cwd=str(cwd), env=e, capture_output=True, text=True, timeout=120)


def test_launcher_refuses_before_a_gpu_is_touched(tmp_path):
    """every refusal comes before the context is made: exit status 1, the message, no cu_depth.dat (on a machine without a GPU the
    accepted case below would fail at the context instead, with another message)"""
    np.zeros(64 * 64 * 3 // 2, np.uint8).tofile(str(tmp_path / "seq.yuv"))
    thr = tmp_path / "Thr_info.txt"
    companion = "0.75 0.25 0.75 0.25 0.75 0.25"
    thr.write_text(companion + "\n")
    for env, word in (({"ETHCNN_SEARCH_BUDGET": "1.5"}, "ETHCNN_SEARCH_BUDGET='1.5'"), ({"ETHCNN_SEARCH_BUDGET": "-1"}, "share"),
                      ({"ETHCNN_SEARCH_BUDGET": "lots"}, "share"), ({"ETHCNN_SEARCH_BUDGET": "nan"}, "share"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_MODE": "both"}, "frame, carry"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4"}, "four integers"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4 x"}, "four integers"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_DEVICES": "0,1"}, "ETHCNN_DEVICES")):
        r = _launch(tmp_path, ETHCNN_SYNTHETIC_SEED=1, **env)
        assert r.returncode == 1 and word in r.stderr and "Traceback" not in r.stderr, (env, r.returncode, r.stderr[-300:])
    for text in ("0.5 0.5 0.5 0.5 0.5 0.5\n", "0.25 0.75 0.25 0.75 0.25 0.75\n", "0.75 0.25 0.75 0.25 0.75\n", companion + " 0.75\n", "0.75 0.25 0.75 0.25 0.75 zero\n",
                 None):
        if text is None:
            os.remove(str(thr))
        else:
            thr.write_text(text)
        r = _launch(tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4")
        assert r.returncode == 1 and companion in r.stderr and "Thr_info.txt" in r.stderr and "Traceback" not in r.stderr, (text, r.stderr[-300:])
    assert sorted(os.listdir(str(tmp_path))) == ["seq.yuv"]
