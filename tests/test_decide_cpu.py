"""CPU: the numpy restatement of the partition decisions (tests/decide_ref.py; include/ethcnn.h "partition decisions") against the
simulator's restatement (tests/sim_ref.py) through the library's host-only ethcnn_decide_counts_from_codes, and the properties that tie
codes, reach and depth together.  Everything is integers: every comparison is equality.

One property is NOT as one might first state it.  "A labelled CTU is bad <=> some block's reach lacks its label's bit" holds from right
to left only: the simulator judges every decided node by its own flag, whatever happened above it, so a SPLIT ONLY node below the
label's leaf -- visited through a BOTH node that the label does not split -- is a wrong_split and makes the CTU bad although the label
stays reachable (test_bad_flag_against_reach holds the smallest such CTU).  The exact statement, asserted here for consistent quadtree
labels: bad <=> reach lacks a label bit OR a SPLIT ONLY node lies below the label's leaf.

The tool's end-to-end run needs the kernel and lives in tests/test_gpu_decide.py; here it only refuses bad command lines."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import decide_ref as dref
import sim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "decide_partition.py")
ENTRIES = ("ethcnn_decide_device", "ethcnn_decide", "ethcnn_decide_set_piece", "ethcnn_decide_frames_device", "ethcnn_decide_counts_from_codes")
ORDERS = (ref.GATES_NONE, ref.GATES_AI, ref.GATES_LDP)
_SETS = {}


def _set(name):
    """(sim_ref.Set, edges that can cross the frame, labelled), made once and never changed"""
    if name not in _SETS:
        s = ref.Set()
        if name == "per_ctu":
            rng = np.random.default_rng(301)
            probs, depth = calib_ref.edge_probs(rng, 300), calib_ref.random_depths(rng, 300)
            probs[7, 3], probs[150, 20] = np.nan, 1.5          # two rejected rows
            s.add(probs, depth)
            _SETS[name] = (s, 0, True)
        elif name == "frames_labelled":
            rng = np.random.default_rng(208)
            probs = calib_ref.edge_probs(rng, 3 * 12).reshape(3, 12, 21)
            labels = rng.integers(0, 4, size=(4, 9, 13)).astype(np.uint8)
            labels[1:, :4, :4] = np.array([3, 0, 2], np.uint8)[:, None, None]  # every level has both classes
            s.add_frames(probs, labels, 208, 144, 1)
            square = rng.integers(0, 4, size=(8, 8, 8)).astype(np.uint8)
            square[::2, 4:, :4], square[1::2, :4, 4:] = 0, 1
            s.add_frames(calib_ref.edge_probs(rng, 8 * 4).reshape(8, 4, 21), square, 128, 128)
            _SETS[name] = (s, 2, True)
        elif name == "frames_ragged":
            rng = np.random.default_rng(200)
            s.add_frames(calib_ref.edge_probs(rng, 6 * 12).reshape(6, 12, 21), None, 200, 136)
            _SETS[name] = (s, 3, False)
        elif name == "gates":
            probs, labels = dref.gate_case(np.random.default_rng(2112))
            s.add_frames(probs, labels, 2112, 2048)
            _SETS[name] = (s, 2, True)
        elif name == "quadtrees":
            rng = np.random.default_rng(16)
            probs, depth = calib_ref.edge_probs(rng, 400), dref.random_quadtrees(rng, 400)
            depth.setflags(write=False)
            s.add(probs, depth)
            _SETS[name], _SETS["quadtree_labels"] = (s, 0, True), depth
    return _SETS[name]


@pytest.mark.parametrize("name", ["per_ctu", "frames_labelled", "frames_ragged"])
def test_counts_from_codes_equal_the_simulators_counters(pkg, name):
    s, edges, labelled = _set(name)
    cands = dref.candidates(np.random.default_rng(5), 12)
    for gates in ORDERS:
        want = s.evaluate(cands, gates)
        got = np.zeros(cands.size, ref.COUNTS)
        for i, c in enumerate(cands):
            out = dref.decide(s, c, gates)
            got[i] = pkg.ethcnn.sim_counts_from_codes(out["codes"])
            assert ref.equal(got[i], dref.counts_from_codes(out["codes"]))
        assert ref.fills_every_field(got, edges=edges, labels=labelled), name
        assert ref.equal(got, want), (name, gates)
    # a window of the set is the same rows
    whole, part = dref.decide(s, cands[0]), dref.decide(s, cands[0], first=5, n=17)
    assert all(np.array_equal(whole[k][5:22], part[k]) for k in whole)


def test_gated_sub_batches():
    s, edges, _ = _set("gates")
    cand = ref.thr(*dref.GATE_CAND)
    for gates in (ref.GATES_AI, ref.GATES_LDP):
        out = dref.decide(s, cand, gates)
        flags = out["codes"][:, 21]
        gate1 = (flags & dref.GATE1_CLOSED) != 0
        only2 = ((flags & dref.GATE2_CLOSED) != 0) & ~gate1
        assert gate1[1024:1056].all() and not gate1[:1024].any() and only2[1056 + 1024:].all() and not only2[:1056].any()
        assert ref.equal(dref.counts_from_codes(out["codes"]), s.evaluate(cand, gates)[0])
        assert not (out["codes"][gate1, 1:5] & 7 == 2).any()  # a zeroed bin is never above up
    none = dref.decide(s, cand, ref.GATES_NONE)
    assert not (none["codes"][:, 21] & (dref.GATE1_CLOSED | dref.GATE2_CLOSED)).any()
    assert not np.array_equal(none["codes"], out["codes"])


def test_bad_flag_against_reach():
    s, _, _ = _set("quadtrees")
    depth16 = _SETS["quadtree_labels"]
    seen = {"lacks": 0, "below_only": 0, "good": 0}
    for gates in ORDERS:
        for c in dref.candidates(np.random.default_rng(6), 16):
            out = dref.decide(s, c, gates)
            flags = out["codes"][:, 21]
            assert ((flags & dref.LABELLED) != 0).all()
            bad = (flags & dref.BAD) != 0
            lacks, below = dref.label_leaf_lacks(out["reach"], depth16), dref.split_only_below_label(out["codes"], depth16)
            assert not (lacks & ~bad).any()                      # the label cannot be reached => bad
            assert np.array_equal(bad, lacks | below)            # and exactly what else makes a CTU bad
            seen["lacks"] += int(lacks.sum())
            seen["below_only"] += int((below & ~lacks).sum())
            seen["good"] += int((~bad).sum())
    assert all(seen.values()), seen
    # the smallest CTU that is bad although its label is reachable: 64 x 64 BOTH, label depth 0, one 32 x 32 node SPLIT ONLY
    p = np.full((1, 21), 500 / 1024.0, np.float32)
    p[0, 1] = 900 / 1024.0
    one = ref.Set()
    one.add(p, np.zeros((1, 16), np.uint8))
    cand = ref.thr((600, 700, 800), (400, 300, 200))
    out = dref.decide(one, cand)
    assert out["codes"][0, :5].tolist() == [3, 2 | 8, 3, 3, 3] and out["codes"][0, 21] == dref.BAD | dref.LABELLED
    assert (out["reach"][0] & 1).all() and int(one.evaluate(cand)[0]["bad_ctus"]) == 1 and out["depth"][0].tolist() == [0] * 16


@pytest.mark.parametrize("name", ["per_ctu", "frames_labelled", "frames_ragged", "gates"])
def test_depth_lies_inside_reach(name):
    s, _, _ = _set(name)
    threes = 0
    for gates in ORDERS:
        for c in list(dref.candidates(np.random.default_rng(7), 8)) + [ref.thr(*dref.GATE_CAND)]:
            by_mid = []
            for mid in (0, 512, 1024):
                out = dref.decide(s, c, gates, mid)
                depth, reach = out["depth"], out["reach"]
                has = depth != 255
                assert ((reach[has].astype(np.int64) >> depth[has]) & 1).all() and depth[has].max(initial=0) <= 3
                assert not reach[~has].any()                     # no preferred depth <=> nothing reachable: outside the picture, or rejected
                by_mid.append(depth)
            both = (out["codes"][:, :21] & 7) == 3
            if both.any() and gates == ref.GATES_NONE:
                threes += 1
                assert (by_mid[0] >= by_mid[1]).all() and (by_mid[1] >= by_mid[2]).all()  # a higher mid_k never splits more
    assert threes


def test_full_search():
    full = ref.thr(*ref.FULL)
    for name in ("per_ctu", "frames_labelled", "frames_ragged"):
        s, _, _ = _set(name)
        out = dref.decide(s, full)
        code = out["codes"][:, :21]
        assert np.array_equal(code == 3, s.inside) and np.array_equal(code == 4, s.edge) and not (out["codes"][:, 21] & dref.BAD).any()
        whole = s.inside.all(axis=1)
        assert whole.any() and (out["reach"][whole] == 0b1111).all() and (out["codes"][whole, 22] == 64).all()
        assert ref.equal(dref.counts_from_codes(out["codes"]), s.evaluate(full)[0])


def test_planes_of_a_ragged_frame():
    s, _, _ = _set("frames_labelled")
    out = dref.decide(s, ref.thr((600, 700, 800), (400, 300, 200)), n=36)
    planes = dref.planes_of(out["depth"], 208, 144)
    assert planes.shape == (3, 9, 13) and planes.max() <= 3  # every block inside the picture has a depth
    ctu = 1 * 12 + 2 * 4 + 3                                   # frame 1, CTU row 2, column 3: one block column, one block row
    assert planes[1, 8, 12] == out["depth"][ctu, 0] and (out["depth"][ctu, 1:] == 255).all()


def test_header_library_and_binding_carry_every_entry(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "partition decisions" in header
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    e = pkg.ethcnn
    assert (e.SIM_FLAG_BAD, e.SIM_FLAG_LABELLED, e.SIM_FLAG_REJECTED, e.SIM_FLAG_GATE1_CLOSED, e.SIM_FLAG_GATE2_CLOSED) == (1, 2, 4, 8, 16)
    for method in ("decide", "decide_device", "decide_frames", "decide_frames_device"):
        assert callable(getattr(pkg.PartitionSim, method))


def test_counts_from_codes_error_paths(pkg):
    e = pkg.ethcnn
    lib = pkg.load_library()
    zero = e.sim_counts_from_codes(np.zeros((0, 24), np.uint8))
    assert not np.frombuffer(zero.tobytes(), np.uint64).any()
    out = np.full(23, 7, np.uint64)
    good = np.zeros((2, 24), np.uint8)
    assert lib.ethcnn_decide_counts_from_codes(None, 2, out.ctypes.data) == e.ERR_ARG
    assert lib.ethcnn_decide_counts_from_codes(good.ctypes.data, -1, out.ctypes.data) == e.ERR_ARG
    assert lib.ethcnn_decide_counts_from_codes(good.ctypes.data, 2, None) == e.ERR_ARG
    for at, value in ((0, 5), (3, 3 | 8), (20, 16), (21, 32), (22, 65), (23, 1)):
        bad = good.copy()
        bad[1, at] = value
        assert lib.ethcnn_decide_counts_from_codes(bad.ctypes.data, 2, out.ctypes.data) == e.ERR_FORMAT, (at, value)
    assert (out == 7).all()  # untouched by every failure
    with pytest.raises(ValueError):
        e.sim_counts_from_codes(np.zeros(25, np.uint8))


@pytest.mark.parametrize("args", [
    [],                                                                                             # no candidate
    ["--thr-info", "t.txt", "--order", "ai"],                                                       # no case
    ["--thr-info", "t.txt", "--case", "l", "p", "64", "64"],                                        # no order
    ["--thr-info", "t.txt", "--order", "ai", "--mid", "1.5", "--case", "l", "p", "64", "64"],
    ["--thr-info", "t.txt", "--order", "ai", "--gates", "open", "--case", "l", "p", "64", "64"],
    ["--thr-info", "t.txt", "--order", "ai", "--weights", "1", "2", "--case", "l", "p", "64", "64"],
    ["--thr-info", "t.txt", "--order", "ai", "--case", "l", "p", "64", "64"],                       # nothing to write or print
    ["--thr-info", "t.txt", "--order", "ai", "--depth-out", "d.dat", "--samples", "s.dat", "--model", "m", "--qp", "32"],  # no frames
])
def test_tool_argument_errors_exit_non_zero(args):
    r = subprocess.run([sys.executable, TOOL] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "decide_partition.py" in r.stderr, (r.returncode, r.stderr[-300:])
