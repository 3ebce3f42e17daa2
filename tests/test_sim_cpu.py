"""CPU: the numpy restatement of the partition-search simulator (tests/sim_ref.py; include/ethcnn.h "partition-search simulation")
against hand-worked CTUs, the closed form of the full search, the calibrator's restatement on level 0, and the properties of its search;
the header and the library carry every entry; the command-line tool refuses bad arguments before it touches a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import sim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "simulate_thresholds.py")
MID = ref.thr((600, 700, 800), (400, 300, 200))
ENTRIES = ("create", "destroy", "reset", "add", "add_device", "add_frames", "add_frames_device", "info", "eval", "sweep", "search", "write_thr_info")


def _counts(c):
    return {f: np.atleast_1d(c[f]).tolist() for f in ref.FIELDS}


def _hand_ctu():
    """64: bin 700; 32: bins 100, 800, 500, 500; 16: bin 900 except raster block 2 (x16 = 2, y16 = 0, inside 32 x 32 block 1): bin 100"""
    p = np.full((1, 21), 900 / 1024.0, np.float32)
    p[0, 0] = 700 / 1024.0
    p[0, 1:5] = np.array([100, 800, 500, 500]) / 1024.0
    p[0, 5 + 2] = 100 / 1024.0
    return p


def test_hand_worked_ctu():
    # 64: 700 > 600 split only.  32 block 0: 100 <= 300 current only (checked, its 16s never visited).  Block 1: 800 > 700 split only;
    # its 16s are raster 2, 3, 6, 7: raster 2 (bin 100 <= 200) current only, the other three split only -> 12 CUs of 8.  Blocks 2, 3:
    # 500 is neither: both (checked), their eight 16s (bin 900 > 800) split only -> 32 CUs of 8.
    want = {"checked": [0, 3, 1, 44], "split_only": [1, 1, 11], "current_only": [0, 1, 1], "both": [0, 2, 0], "edge_split": [0, 0, 0]}
    for depth, wrong in ((None, {"wrong_split": [0, 0, 0], "wrong_stop": [0, 0, 0], "bad_ctus": [0]}),
                         (np.zeros((1, 16), np.uint8), {"wrong_split": [1, 1, 11], "wrong_stop": [0, 0, 0], "bad_ctus": [1]}),
                         (np.full((1, 16), 3, np.uint8), {"wrong_split": [0, 0, 0], "wrong_stop": [0, 1, 1], "bad_ctus": [1]})):
        s = ref.Set()
        s.add(_hand_ctu(), depth)
        got = _counts(s.evaluate(MID)[0])
        assert got == dict(want, **wrong), (depth, got)
    # the grid is exact: one ulp above 600 / 1024 is bin 601 > 600, 600 / 1024 itself is not
    for p64, split in ((np.float32(600 / 1024.0), 0), (np.nextafter(np.float32(600 / 1024.0), np.float32(1)), 1)):
        p = _hand_ctu()
        p[0, 0] = p64
        s = ref.Set()
        s.add(p)
        assert s.evaluate(MID)[0]["split_only"][0] == split
    # down > up: HM tests "split only" first
    s = ref.Set()
    s.add(_hand_ctu())
    got = s.evaluate(ref.thr((600, 700, 800), (1024, 1024, 1024)))[0]
    assert got["split_only"].tolist() == [1, 1, 3] and got["current_only"].tolist() == [0, 3, 1] and got["both"].tolist() == [0, 0, 0]


def test_rejected_ctu_counts_nowhere():
    p = np.concatenate([_hand_ctu(), _hand_ctu(), _hand_ctu(), _hand_ctu()])
    p[1, 20], p[2, 3], p[3, 0] = np.nan, -0.5, 1.5
    s = ref.Set()
    s.add(p, np.zeros((4, 16), np.uint8))
    one = ref.Set()
    one.add(_hand_ctu(), np.zeros((1, 16), np.uint8))
    assert s.info() == {"ctus": 4, "whole_ctus": 1, "labelled_ctus": 1, "rejected_ctus": 3, "sub_batches": 0}
    assert ref.equal(s.evaluate(MID), one.evaluate(MID))
    with pytest.raises(calib_ref.BadDepth):
        s.add(_hand_ctu(), np.full((1, 16), 4, np.uint8))


@pytest.mark.parametrize("w,h", [(128, 192), (200, 136), (208, 144), (64, 64), (72, 8)])
def test_full_search_is_counted_from_geometry_alone(w, h):
    rng = np.random.default_rng(w)
    frames = 2
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    s = ref.Set()
    s.add_frames(calib_ref.edge_probs(rng, frames * nctu), None, w, h)
    got = s.evaluate(ref.thr(*ref.FULL))[0]
    sizes = (64, 32, 16)
    inside = [(w // z) * (h // z) for z in sizes]
    touched = [-(-w // z) * -(-h // z) for z in sizes]
    assert got["checked"].tolist() == [frames * x for x in inside + [(w // 8) * (h // 8)]]
    assert got["both"].tolist() == [frames * x for x in inside] and not got["split_only"].any() and not got["current_only"].any()
    assert got["edge_split"].tolist() == [frames * (t - i) for t, i in zip(touched, inside)]
    assert s.info()["whole_ctus"] == frames * (w // 64) * (h // 64) and s.info()["sub_batches"] == frames
    if w % 64 == 0 and h % 64 == 0:  # whole CTUs: 1 / 4 / 16 / 64 checks each
        assert got["checked"].tolist() == [frames * nctu * x for x in (1, 4, 16, 64)]


def test_level_0_is_the_calibrators_miss_and_fsplit():
    rng = np.random.default_rng(257)
    n, k = 257, 512
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    hist, _ = calib_ref.histogram(probs, depth)
    s = ref.Set()
    s.add(probs, depth)
    for kk in (k, 0, 300, 1023):
        got = s.evaluate(ref.thr((kk,) * 3, (kk,) * 3))[0]
        miss, fsplit = int(hist[0, 1, :kk + 1].sum()), int(hist[0, 0, kk + 1:].sum())
        assert (int(got["wrong_stop"][0]), int(got["wrong_split"][0])) == (miss, fsplit)
        if kk == k:
            assert miss > 0 and fsplit > 0
    assert ref.fills_every_field(s.evaluate(MID), edges=0)


def test_gates_of_the_ai_order_change_nothing_and_those_of_the_ldp_order_do():
    rng = np.random.default_rng(11)
    w, h, frames = 2560, 1920, 2  # 1200 CTUs a frame: sub-batches of 1024 and 176
    probs = calib_ref.edge_probs(rng, frames * 1200).reshape(frames, 1200, 21)
    probs[:, 1024:, 0] = np.minimum(probs[:, 1024:, 0], np.float32(500 / 1024.0))
    probs[:, 1024:, 1:5] = np.minimum(probs[:, 1024:, 1:5], np.float32(600 / 1024.0))
    s = ref.Set()
    s.add_frames(probs, None, w, h)
    assert s.info()["sub_batches"] == 4 and s.m1[1] == 500 and s.m2[1] == 600
    cands = ref.thr([(600, 700, 800), (400, 700, 800), (400, 500, 800), (450, 650, 800), (1024, 1024, 1024), (500, 600, 700)],
                    [(400, 300, 200), (300, -1, 200), (300, -1, 200), (400, 300, 200), (-1, -1, -1), (500, 600, 700)])
    none, ai, ldp = (s.evaluate(cands, g) for g in (ref.GATES_NONE, ref.GATES_AI, ref.GATES_LDP))
    assert ref.equal(none, ai)
    differs = [not ref.equal(none[i:i + 1], ldp[i:i + 1]) for i in range(cands.size)]
    # up0 = 600 >= M1 = 500 closes gate 1 of the capped sub-batches; up0 = 400 with up1 = 700 >= M2 closes gate 2 only
    assert differs == [True, True, False, True, False, False]  # (the full search reads no bin; under the last, no capped CTU is split)
    # the AI-order gates change nothing only while down_k <= up_k: with down0 = 500 > up0 = 400 a CTU of a sub-batch whose gate 1 is
    # closed (every p64 <= down0) is still split (p64 > up0 is tested first) and then reads zeroed p32
    crossed = ref.thr((400, 650, 800), (500, 300, 200))
    assert not ref.equal(s.evaluate(crossed, ref.GATES_NONE), s.evaluate(crossed, ref.GATES_AI))
    # candidate 0 under the LDP gates: in the capped sub-batches every p32 and p16 reads 0: bin 0 <= down: current only at 32
    capped = ref.Set()
    z = probs[:, 1024:].copy()
    z[:, :, 1:] = 0
    capped.add(z.reshape(-1, 21))
    rest = ref.Set()
    rest.add(probs[:, :1024].reshape(-1, 21))
    both = np.zeros(1, ref.COUNTS)
    for f in ref.FIELDS:
        both[f] = capped.evaluate(cands[:1])[f] + rest.evaluate(cands[:1])[f]
    assert ref.equal(both, ldp[:1])


def test_search_never_increases_cost_and_stays_feasible():
    rng = np.random.default_rng(5)
    n = 100
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    # probabilities that lean towards the truth, so that pruning is possible at all
    t = np.zeros((n, 21), bool)
    d = depth.astype(np.int64)
    t[:, 0], t[:, 1:5], t[:, 5:] = d.sum(axis=1) > 8, d[:, calib_ref.IDX32].sum(axis=2) > 6, d == 3
    probs = np.where(t, np.float32(0.5) + probs / 2, probs / 2).astype(np.float32)
    s = ref.Set()
    s.add(probs, depth)
    weights = (64, 16, 4, 1)
    cost = lambda c: sum(w * int(x) for w, x in zip(weights, c["checked"]))
    full = s.evaluate(ref.thr(*ref.FULL))[0]
    assert int(full["bad_ctus"]) == 0 and full["checked"].tolist() == [n, 4 * n, 16 * n, 64 * n]
    last = cost(full)
    for rounds in (0, 1, 8):
        thr, counts, ran = s.search(ref.thr(*ref.FULL), ref.GATES_NONE, weights, 100000, rounds)
        assert ran <= rounds and ref.equal(s.evaluate(thr)[0], counts)
        assert int(counts["bad_ctus"]) * 10 ** 6 <= 100000 * n and cost(counts) <= last
        last = cost(counts)
    assert last < cost(full)
    again = s.search(thr, ref.GATES_NONE, weights, 100000, 8)  # a fixed point stays: one round that changes nothing
    assert again[0] == thr and again[2] == 1
    with pytest.raises(ValueError):
        s.search(ref.thr((0, 0, 0), (1024, 1024, 1024)), ref.GATES_NONE, weights, 0)  # infeasible start
    unlabelled = ref.Set()
    unlabelled.add(probs)
    with pytest.raises(ValueError):
        unlabelled.search(ref.thr(*ref.FULL), ref.GATES_NONE, weights, 1000)


def test_header_declares_every_entry_and_the_library_exports_it(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    declared = set(re.findall(r"\b(ethcnn_sim_\w+)\(", header))
    assert declared == {"ethcnn_sim_" + e for e in ENTRIES}
    lib = ctypes.CDLL(os.path.join(ROOT, "hevc-complexity-reduction_amd", "lib", "libethcnn.so"))
    for name in declared:
        assert getattr(lib, name)
    for const in ("ETHCNN_SIM_GATES_NONE = 0", "ETHCNN_SIM_GATES_AI = 1", "ETHCNN_SIM_GATES_LDP = 2", "ETHCNN_SIM_SWEEP_MAX 1026"):
        assert const in header
    e = pkg.ethcnn
    assert e.SIM_THR.itemsize == 24 and e.SIM_COUNTS.itemsize == 23 * 8 and e.SIM_THR == ref.THR and e.SIM_COUNTS == ref.COUNTS
    assert pkg.PartitionSim is e.PartitionSim
    # the writer is host only: the calibrator's line and token orders
    lib2 = pkg.load_library()
    assert lib2.ethcnn_sim_write_thr_info(b"x", None, 0) == e.ERR_ARG
    bad = e.sim_thr((0, 0, 1025), (0, 0, 0))
    assert lib2.ethcnn_sim_write_thr_info(b"x", bad.ctypes.data, 0) == e.ERR_ARG and not os.path.exists("x")


@pytest.mark.parametrize("order", ["ai", "ldp"])
def test_thr_info_writer_matches_the_calibrators_line(pkg, tmp_path, order):
    path = str(tmp_path / "Thr_info.txt")
    for up, down in (((1024, 1024, 1024), (-1, -1, -1)), ((600, 700, 800), (400, 300, 200)), ((0, 5, 1), (1024, 7, 0))):
        pkg.ethcnn.sim_write_thr_info(path, pkg.ethcnn.sim_thr(up, down), order)
        assert open(path).read() == calib_ref.thr_info_line([{"down_k": d, "up_k": u} for d, u in zip(down, up)], order)
        assert os.listdir(str(tmp_path)) == ["Thr_info.txt"]


@pytest.mark.parametrize("args", [
    [],                                                                                   # no mode
    ["--thr-info", "t.txt", "--order", "ai"],                                             # no case
    ["--thr-info", "t.txt", "--case", "l", "p", "64", "64"],                              # no order
    ["--thr-info", "t.txt", "--order", "ai", "--sweep", "up0", "--case", "l", "p", "64", "64"],  # two modes
    ["--sweep", "up3", "--case", "l", "p", "64", "64"],
    ["--search", "--order", "ai", "--out", "o.txt", "--case", "l", "p", "64", "64"],      # no budget
    ["--search", "--max-bad-ppm", "2000000", "--order", "ai", "--out", "o.txt", "--case", "l", "p", "64", "64"],
    ["--thr-info", "t.txt", "--order", "ai", "--gates", "open", "--case", "l", "p", "64", "64"],
    ["--thr-info", "t.txt", "--order", "ai", "--yuv", "s.yuv", "64", "64", "32"],         # no model directory
    ["--thr-info", "t.txt", "--order", "ai", "--weights", "1", "2", "--case", "l", "p", "64", "64"],
])
def test_tool_argument_errors_exit_non_zero(args):
    r = subprocess.run([sys.executable, TOOL] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "simulate_thresholds.py MODE" in r.stderr, (r.returncode, r.stderr[-300:])
