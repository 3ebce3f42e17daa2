"""CPU: the numpy restatement of the threshold calibration on reached nodes (tests/reach_ref.py; include/ethcnn.h "threshold calibration
on reached nodes") against the identities the header states -- the simulator's wrong decisions are sums over the histogram, a level
depends only on the levels above it, the full search counts every node -- and against the calibrator's restatement on level 0; a set
on which the teacher-forced choice breaks its own budget in the simulated search while the reached choice holds it; the header, the
library and the binding carry the two entries; the command-line tool refuses bad arguments before it touches a GPU.  Integers only:
every comparison is equality."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import decide_ref as dref
import reach_ref as rr
import sim_ref as ref
import test_gpu_ladder as tl   # the frames / small / perctu cases are those of the labelled walk, made once and never changed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "calibrate_thresholds.py")
GATES = (ref.GATES_NONE, ref.GATES_AI, ref.GATES_LDP)


def _cands(seed, k=24):
    """the fixed four of decide_ref.candidates (the fourth is crossed), random ones, and the ends of the ranges"""
    c = dref.candidates(np.random.default_rng(seed), k)
    c[4] = ref.thr((0, 0, 0), (-1, -1, -1))
    c[5] = ref.thr((1024, 0, 1024), (1024, 1024, -1))
    c[6] = ref.thr((0, 1024, 0), (0, -1, 1024))
    assert (c["down_k"] > c["up_k"]).any()
    return c


def check_identities(s, cands, gates, hist, ev):
    """the identities of the header between a histogram [K, 3, 2, 1025] and the evaluation counters of the same candidates"""
    for c in range(cands.size):
        up, down = cands[c]["up_k"], cands[c]["down_k"]
        for l in range(3):
            assert int(ev[c]["wrong_split"][l]) == int(hist[c, l, 0, int(up[l]) + 1:].sum()), (c, l)
            assert int(ev[c]["wrong_stop"][l]) == int(hist[c, l, 1, :min(int(down[l]), int(up[l])) + 1].sum()), (c, l)
        assert np.array_equal(hist[c, 0], hist[0, 0])                                          # level 0 sees no threshold


@pytest.mark.parametrize("gates", GATES)
@pytest.mark.parametrize("name", ["frames", "small", "perctu"])
def test_wrong_decisions_are_sums_over_the_histogram(name, gates):
    s = tl._case(name)[-1]
    cands = _cands(41)
    hist = rr.reach_hist(s, cands, gates)
    ev = s.evaluate(cands, gates)
    check_identities(s, cands, gates, hist, ev)
    # against vacuous passes (with depths uniform in 0..3 nearly every CTU is labelled split: level 0 has next to no unsplit node)
    assert ev["wrong_split"][:, 1:].any(axis=0).all() and ev["wrong_stop"].any(axis=0).all()
    assert int(hist[1].sum()) == 21 * int((s.labelled & s.inside.all(axis=1)).sum())           # candidate 1 is the full search
    assert hist.sum(axis=(1, 2, 3)).min() < hist[1].sum()                                      # pruning reaches fewer nodes


def test_gates_change_the_bins_that_are_counted():
    """decide_ref.gate_case: sub-batches of 1024 and 32 whose gates 1 / 2 close under GATE_CAND for both gated orders"""
    probs, labels = dref.gate_case(np.random.default_rng(2112))
    s = ref.Set()
    s.add_frames(probs, labels, 2112, 2048)
    cands = _cands(42)
    cands[7] = ref.thr((600, 700, 800), (300, 300, 200))   # LDP gates 1 and 2 close over nodes that land in BOTH: their sub-CUs read zeros
    cands[8] = ref.thr((400, 650, 800), (500, 300, 200))   # crossed at level 0: a CTU behind a closed AI gate 1 is still split, and reads zeros
    hists = {}
    for gates in GATES:
        hists[gates] = rr.reach_hist(s, cands, gates)
        check_identities(s, cands, gates, hists[gates], s.evaluate(cands, gates))
    # (while down_k <= up_k a closed AI gate lies under a node that stopped: candidate 7 moves nothing there)
    assert np.array_equal(hists[ref.GATES_AI][7], hists[ref.GATES_NONE][7])
    for gates, c in ((ref.GATES_AI, 8), (ref.GATES_LDP, 7)):
        assert not np.array_equal(hists[gates][c], hists[ref.GATES_NONE][c])
        assert hists[gates][c, 1:, :, 0].sum() > hists[ref.GATES_NONE][c, 1:, :, 0].sum()      # zeroed bins land in bin 0
    assert np.array_equal(hists[ref.GATES_AI][1], hists[ref.GATES_NONE][1])                    # the full search: down_k = -1 < M closes no gate ...
    full = hists[ref.GATES_LDP][1]                                                             # ... up_k = 1024 >= M closes every one: the same nodes, all read 0
    assert full[1:, :, 1:].sum() == 0 and np.array_equal(full.sum(axis=2), hists[ref.GATES_NONE][1].sum(axis=2))
    assert np.array_equal(hists[ref.GATES_LDP][:, 0], hists[ref.GATES_NONE][:, 0])             # level 0 is never gated


@pytest.mark.parametrize("which", ["small", "random"])
def test_the_full_search_counts_every_node(which):
    if which == "small":
        probs, depth = tl._case("small")[:2]
    else:
        rng = np.random.default_rng(257)
        probs, depth = calib_ref.edge_probs(rng, 257), calib_ref.random_depths(rng, 257)
    s = ref.Set()
    s.add(probs, depth)
    hist = rr.reach_hist(s, ref.thr(*ref.FULL))[0]
    assert np.array_equal(hist[0], calib_ref.histogram(probs, depth)[0][0])                    # level 0 is the calibrator's
    for l, (a, b) in enumerate(rr.SPANS):                                                      # every level: a direct count of all its nodes
        for t in (0, 1):
            want = np.bincount(s.bins[:, a:b][s.truth[:, a:b] == bool(t)], minlength=1025)
            assert np.array_equal(hist[l, t], want.astype(np.uint64)), (l, t)
        assert int(hist[l].sum()) == probs.shape[0] * (b - a)
    teacher = calib_ref.histogram(probs, depth)[0]                                             # the teacher-forced populations are subsets
    assert (teacher[1:] <= hist[1:]).all() and teacher[2].sum() < hist[2].sum()
    assert teacher[1].sum() < hist[1].sum() or which == "small"                                # (depths uniform in 0..3: every CTU of "small" is labelled split)


@pytest.mark.parametrize("gates", GATES)
def test_a_level_does_not_move_with_the_thresholds_at_or_below_it(gates):
    s = tl._case("frames")[-1]
    rng = np.random.default_rng(43)
    base = _cands(44, 8)
    for l in range(3):
        moved = base.copy()
        moved["up_k"][:, l:] = rng.integers(0, 1025, size=(base.size, 3 - l))
        moved["down_k"][:, l:] = rng.integers(-1, 1025, size=(base.size, 3 - l))
        a, b = rr.reach_hist(s, base, gates), rr.reach_hist(s, moved, gates)
        assert np.array_equal(a[:, :l + 1], b[:, :l + 1]), l
        if l < 2:
            assert not np.array_equal(a[:, l + 1:], b[:, l + 1:])                              # ... while the levels below it do


@pytest.mark.parametrize("gates", GATES)
@pytest.mark.parametrize("eps", [(0, 0), (20000, 20000), (10 ** 6, 10 ** 6), ((0, 50000, 300000), (100000, 0, 20000))])
def test_the_reached_choice_meets_the_simulated_search_exactly(gates, eps):
    s = tl._case("frames")[-1]
    eps_down, eps_up = [e if isinstance(e, tuple) else (e,) * 3 for e in eps]
    levels, thr, counts = rr.calibrate_reached(s, eps_down, eps_up, gates)
    for l, lv in enumerate(levels):
        assert (int(counts["wrong_stop"][l]), int(counts["wrong_split"][l])) == (lv["miss"], lv["fsplit"])
        assert lv["miss"] * 10 ** 6 <= eps_down[l] * lv["n1"] and lv["fsplit"] * 10 ** 6 <= eps_up[l] * lv["n0"]
        assert (int(thr["up_k"][l]), int(thr["down_k"][l])) == (lv["up_k"], lv["down_k"])
    final = rr.reach_hist(s, thr, gates)[0]
    assert [int(final[l, 0].sum()) for l in range(3)] == [lv["n0"] for lv in levels]           # n0 / n1 are the classes the result reaches
    assert [int(final[l, 1].sum()) for l in range(3)] == [lv["n1"] for lv in levels]
    with pytest.raises(ValueError):
        rr.calibrate_reached(s, (10 ** 6 + 1, 0, 0), eps_up, gates)
    plain = ref.Set()
    plain.add(tl._case("perctu")[2])
    with pytest.raises(ValueError):
        rr.calibrate_reached(plain, eps_down, eps_up, gates)


def _off_distribution_set():
    """1000 CTUs labelled unsplit and 1000 with random depths.  The 64 x 64 head answers 0.5 everywhere, so every 32 x 32 node is
    reached.  The 32 x 32 head is a noisy teacher under the split-labelled CTUs, the only ones the calibrator counts at level 1, and
    over-confident (uniform in 0.5..1) under the unsplit-labelled ones, where every 32 x 32 flag is unsplit"""
    rng = np.random.default_rng(2029)
    n = 1000
    depth = np.concatenate([np.zeros((n, 16), np.uint8), rng.integers(0, 4, size=(n, 16)).astype(np.uint8)])
    t = ref.Set()
    t.add(np.zeros((2 * n, 21), np.float32), depth)
    probs = tl._teacher(np.random.default_rng(2030), t.truth, t.labelled)
    probs[:, 0] = 0.5
    probs[:n, 1:5] = (np.rint(rng.uniform(0.5, 1.0, size=(n, 4)) * 128) / 128.0).astype(np.float32)
    s = ref.Set()
    s.add(probs, depth)
    return probs, depth, s


def test_the_teacher_forced_choice_breaks_its_budget_where_the_reached_choice_holds_it():
    probs, depth, s = _off_distribution_set()
    eps = (50000,) * 3
    forced = calib_ref.choose(calib_ref.histogram(probs, depth)[0], eps, eps)
    thr = ref.thr([lv["up_k"] for lv in forced], [lv["down_k"] for lv in forced])
    ev = s.evaluate(thr)[0]
    reached = rr.reach_hist(s, thr)[0]
    n0, n1 = int(reached[1, 0].sum()), int(reached[1, 1].sum())                                # the level-1 classes that choice reaches
    assert forced[1]["fsplit"] * 10 ** 6 <= eps[1] * forced[1]["n0"]                           # its promise, on the population it counted ...
    assert n0 > 2 * forced[1]["n0"]                                                            # ... the search meets many more unsplit nodes ...
    assert int(ev["wrong_split"][1]) * 10 ** 6 > 5 * eps[1] * n0                               # ... and wrongly splits over five times the budget
    levels, thr2, counts = rr.calibrate_reached(s, eps, eps)
    for l in range(3):
        assert int(counts["wrong_split"][l]) * 10 ** 6 <= eps[l] * levels[l]["n0"] and int(counts["wrong_stop"][l]) * 10 ** 6 <= eps[l] * levels[l]["n1"]
    assert levels[1]["n0"] == n0 and levels[1]["n1"] == n1                                     # (level 0 is the same choice: the same nodes are reached)
    assert levels[1]["up_k"] > forced[1]["up_k"]


def test_header_library_and_binding_carry_the_two_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\bint (ethcnn_reach_\w+)\(", code))
    assert declared == {"ethcnn_reach_hist", "ethcnn_reach_calibrate"} == set(re.findall(r"\b(ethcnn_reach_\w+)\(", header))
    assert "#define ETHCNN_REACH_HIST_WORDS ETHCNN_CALIB_HIST_WORDS" in header and "#define ETHCNN_REACH_MAX_CAND 256" in header
    lib = ctypes.CDLL(os.path.join(ROOT, "hevc-complexity-reduction_amd", "lib", "libethcnn.so"))
    for name in declared:
        assert getattr(lib, name)
    e = pkg.ethcnn
    assert {n for n in e.SIGNATURES if n.startswith("ethcnn_reach_")} == declared
    assert e.REACH_MAX_CAND == 256 and callable(e.PartitionSim.reach_hist) and callable(e.PartitionSim.calibrate_reached)
    lib2 = pkg.load_library()                                                                  # a NULL simulator is refused before anything is read
    assert lib2.ethcnn_reach_hist(None, None, 1, 0, None) == e.ERR_ARG
    assert lib2.ethcnn_reach_calibrate(None, None, None, 0, None, None, None) == e.ERR_ARG


@pytest.mark.parametrize("args", [
    ["--gates", "ai", "--case", "l", "p", "64", "64"],                                         # --gates without --reached
    ["--gates", "ldp", "--out", "o.txt", "--order", "ldp", "--case", "l", "p", "64", "64"],
    ["--reached", "--gates", "open", "--case", "l", "p", "64", "64"],                          # a bad value
    ["--reached", "--gates", "--case", "l", "p", "64", "64"],
    ["--reached", "--gates"],
])
def test_tool_refuses_before_a_gpu_is_touched(tmp_path, args):
    r = subprocess.run([sys.executable, TOOL] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "calibrate_thresholds.py [--eps-down" in r.stderr and "error:" in r.stderr, (r.returncode, r.stderr[-300:])
    assert os.listdir(str(tmp_path)) == [] and r.stdout == ""


def test_parse_without_reached_is_unchanged():
    spec = importlib.util.spec_from_file_location("calibrate_thresholds", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    opt, cases = tool.parse(["--eps-down", "1", "2", "3", "--out", "t.txt", "--order", "ldp", "--hist", "h.dat", "--json", "--case", "l", "p", "208", "144",
                             "--skip-label-frames", "1"])
    assert opt == {"eps_down": [1, 2, 3], "eps_up": [50000] * 3, "out": "t.txt", "order": "ldp", "hist": "h.dat", "reliability_out": None, "json": True,
                   "device": 0, "source_format": (8, 420)}
    assert cases == [{"kind": "case", "labels": "l", "probs": "p", "w": 208, "h": 144, "skip": 1}]
    for extra, gates in (([], "ldp"), (["--gates", "none"], "none")):                          # --gates defaults to --order's value when --out is given
        got, _ = tool.parse(["--reached", "--out", "t.txt", "--order", "ldp", "--case", "l", "p", "208", "144"] + extra)
        assert got["reached"] is True and got["gates"] == gates
    assert tool.parse(["--reached", "--case", "l", "p", "208", "144"])[0]["gates"] == "none"
