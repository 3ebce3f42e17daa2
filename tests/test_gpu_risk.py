"""-m gpu: the expected wrong decisions (include/ethcnn.h "partition-search simulation: expected wrong decisions") on the GPU.  k_sim_risk
is compared with the restatement (tests/risk_ref.py) under the identity table, a random table that is not monotone and a fitted one,
and with a second witness: the per-node codes of PartitionSim.decide summed in numpy.  The ladder walk by risk is compared field for
field with the restatement's walk, every rung with the simulator's own evaluations, and a built ladder goes through the hinge: the
controller tool holds a budget with it and the All-Intra launcher builds it for the file it is about to hand to the encoder.
Probabilities are quantised to 1 / 128 so that ties happen.  Integers only: every comparison is equality.  The sets are those at which
the ladder tests find slices, partial candidate waves and ties (tests/test_gpu_ladder.py), two frame geometries with partial CTUs
and one of more than 64 CTUs a slice."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_ref as bref
import decide_ref as dref
import ladder_ref as lref
import risk_ref as rref
import sim_ref as ref
import test_gpu_ladder as tl   # the frames / small / perctu cases are those of the labelled walk, made once and never changed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
CONTROL_TOOL = os.path.join(ROOT, "tools", "control_budget.py")
BUILD_TOOL = os.path.join(ROOT, "tools", "build_ladder.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
GEOM = {"frames": (tl.W, tl.H), "odd": (200, 136), "wide": (1088, 1024)}   # 208 x 144 x 30; 200 x 136 x 7 (multiples of 8 only); 1088 x 1024 x 3
_CASES, _TABLES, _PATHS, _STATS = {}, {}, {}, {}


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _case(name):
    """-> (list of add calls, Set): an add call is ("frames", probs, labels, w, h) or ("ctus", probs, depth16 or None)"""
    if name not in _CASES:
        if name in ("frames", "small", "perctu"):
            c = tl._case(name)
            if name == "frames":
                adds = [("frames", c[0], c[1], tl.W, tl.H)]
            else:
                adds = [("ctus", c[0], c[1])] + ([("ctus", c[2], None)] if c[2].shape[0] else [])
            _CASES[name] = (adds, c[-1])
        else:
            w, h = GEOM[name]
            frames = 7 if name == "odd" else 3
            rng = np.random.default_rng(31 if name == "odd" else 32)
            per = ((w + 63) // 64) * ((h + 63) // 64)
            probs = (rng.integers(0, 129, size=(frames, per, 21)) / 128.0).astype(np.float32)
            probs.setflags(write=False)
            s = ref.Set()
            s.add_frames(probs, None, w, h)
            _CASES[name] = ([("frames", probs, None, w, h)], s)
    return _CASES[name]


def _add(sim, call):
    if call[0] == "frames":
        sim.add_frames(call[1], call[2], call[3], call[4])
    else:
        sim.add(call[1], call[2])


def _fill(sim, name):
    adds, s = _case(name)
    for call in adds:
        _add(sim, call)
    return s


def _table(pkg, which):
    """identity (None), a random table that is not monotone, a table fitted to a random histogram"""
    if which not in _TABLES:
        rng = np.random.default_rng(33)
        if which == "identity":
            _TABLES[which] = None
        elif which == "random":
            _TABLES[which] = rng.integers(0, rref.ONE + 1, size=(3, 1025)).astype(np.uint32)
        else:
            n = rng.integers(0, 300, size=(3, 1025))
            split = rng.binomial(n, 0.2 + 0.6 * np.arange(1025) / 1024.0)
            hist = np.stack([n - split, split], axis=1).astype(np.uint64)
            _TABLES[which] = pkg.ethcnn.risk_from_hist(hist)
            assert np.array_equal(_TABLES[which], rref.from_hist(hist)) and not np.array_equal(_TABLES[which], rref.identity())
    return _TABLES[which]


def _same_risk(got, want):
    split, stop = want
    assert got["exp_wrong_split"].tolist() == split and got["exp_wrong_stop"].tolist() == stop


@pytest.mark.parametrize("name", ["frames", "odd", "wide", "perctu"])
def test_eval_risk_against_the_restatement_and_the_partition_decisions(pkg, sim, name):
    s = _fill(sim, name)
    info = sim.info()
    assert (info["ctus"], info["rejected_ctus"]) == (s.ctus, s.rejected)
    if name == "perctu":
        assert info["rejected_ctus"] == 1 and info["labelled_ctus"] == 1299
    if name == "odd":
        assert info["labelled_ctus"] == 0 and info["whole_ctus"] < info["ctus"]     # partial CTUs right and below, no label anywhere
    rng = np.random.default_rng(34)
    filled = np.zeros(6, bool)
    for which in ("identity", "random", "fitted"):
        table = _table(pkg, which)
        sim.set_reliability(table)
        for k in (1, 3, 64, 65, 513):                                                # one lane, a partial wave, a full wave, one more, nine waves
            cands = dref.candidates(rng, max(k, 4))[:k]                              # (the first four are fixed: the fourth is crossed)
            assert k < 4 or (cands["down_k"] > cands["up_k"]).any()                  # crossed candidates among them
            got = sim.eval_risk(cands)
            assert got.dtype == pkg.ethcnn.SIM_RISK and got.shape == (k,)
            _same_risk(got, rref.evaluate(s, cands, table))
            filled |= np.concatenate([got["exp_wrong_split"].any(axis=0), got["exp_wrong_stop"].any(axis=0)])
            if k == 3:   # the second witness: the decisions of each candidate, node by node, summed in numpy
                for i in range(3):
                    codes = sim.decide(cands[i], "none", want=("codes",))["codes"]
                    split, stop = rref.from_codes(s, codes, table)
                    assert got[i]["exp_wrong_split"].tolist() == split and got[i]["exp_wrong_stop"].tolist() == stop
    assert filled.all()                                                              # against vacuous passes: every field is non-zero somewhere
    sim.set_reliability(None)                                                        # NULL restores the identity
    cands = dref.candidates(rng, 5)
    _same_risk(sim.eval_risk(cands), rref.evaluate(s, cands, None))
    zero = sim.eval_risk(ref.thr(*ref.FULL))[0]                                      # the full search forces nothing
    assert not zero["exp_wrong_split"].any() and not zero["exp_wrong_stop"].any()


def test_sums_do_not_depend_on_how_the_set_was_added(pkg, sim):
    probs, labels, s = tl._case("frames")
    rng = np.random.default_rng(35)
    cands = dref.candidates(rng, 70)
    sim.set_reliability(_table(pkg, "random"))
    sim.add_frames(probs, labels, tl.W, tl.H)
    whole = sim.eval_risk(cands)
    sim.reset()                                                                      # (the table belongs to the simulator: reset keeps it)
    sim.add_frames(probs[:7], labels[:7], tl.W, tl.H)
    sim.add_frames(probs[7:8], None, tl.W, tl.H)                                     # labels play no part
    sim.add_frames(probs[8:], labels[8:], tl.W, tl.H)
    pieces = sim.eval_risk(cands)
    sim.reset()
    sim.add_frames(probs[11:], None, tl.W, tl.H)                                     # another order, other sub-batches
    sim.add_frames(probs[:11], labels[:11], tl.W, tl.H)
    other = sim.eval_risk(cands)
    assert whole.tobytes() == pieces.tobytes() == other.tobytes()
    _same_risk(whole, rref.evaluate(s, cands, _table(pkg, "random")))


def test_refusals_change_nothing(pkg, sim):
    e = pkg.ethcnn
    cands = dref.candidates(np.random.default_rng(36), 4)
    assert sim.eval_risk(cands).tobytes() == np.zeros(4, e.SIM_RISK).tobytes()       # an empty set gives zeros
    assert sim.eval_risk(cands[:0]).shape == (0,)                                    # no candidate: a no-op
    s = _fill(sim, "small")
    table = _table(pkg, "random")
    sim.set_reliability(table)
    before = sim.eval_risk(cands)
    over = table.copy()
    over[2, 1024] = e.RISK_ONE + 1
    with pytest.raises(pkg.EthCnnError) as err:
        sim.set_reliability(over)
    assert err.value.code == e.ERR_ARG and "level 2, bin 1024" in str(err.value)
    assert sim.eval_risk(cands).tobytes() == before.tobytes()                        # the table in use is the one from before
    with pytest.raises(ValueError):
        sim.set_reliability(table[:2])
    out = np.full(4, 7, e.SIM_RISK)
    for up, down in (((1025, 5, 5), (0, 0, 0)), ((5, 5, -1), (0, 0, 0)), ((5, 5, 5), (0, -2, 0)), ((5, 5, 5), (0, 0, 1025))):
        bad = cands.copy()
        bad[2] = ref.thr(up, down)
        assert sim.lib.ethcnn_risk_eval(sim.h, bad.ctypes.data, 4, out.ctypes.data) == e.ERR_ARG
    assert sim.lib.ethcnn_risk_eval(sim.h, None, 4, out.ctypes.data) == e.ERR_ARG and sim.lib.ethcnn_risk_eval(sim.h, cands.ctypes.data, -1, out.ctypes.data) == e.ERR_ARG
    assert (out["exp_wrong_stop"] == 7).all()
    _same_risk(before, rref.evaluate(s, cands, table))


# --------------------------------------------------------------------------------------------------------------- the ladder ---
def _want(name, table, weights=None, grid=8, max_rungs=4096, max_risk_ppm=rref.NO_CAP):
    key = (name, table, weights, grid, max_rungs, max_risk_ppm)
    if key not in _PATHS:
        _STATS[key] = {}
        _PATHS[key] = rref.build(_case(name)[1], _TABLES[table], weights, grid, max_rungs, max_risk_ppm, _STATS[key])
    return _PATHS[key]


def _same(got, want):
    """field for field"""
    assert len(got["cost"]) == len(want)
    for name, field in (("up_k", got["thr"]["up_k"]), ("down_k", got["thr"]["down_k"]), ("checked", got["checked"]), ("exp_wrong_split", got["exp_wrong_split"]),
                        ("exp_wrong_stop", got["exp_wrong_stop"])):
        assert field.tolist() == [r[name] for r in want], name
    for name in ("coord", "value", "risk", "cost"):
        assert [int(x) for x in got[name]] == [r[name] for r in want], name
    assert got["coord"].dtype == np.int32 and got["checked"].dtype == np.uint64 and got["exp_wrong_stop"].dtype == np.uint64


def _witness(sim, got):
    """the simulator's own evaluations of every rung's thresholds give the rung's counters"""
    counts, risk = sim.eval(got["thr"], "none"), sim.eval_risk(got["thr"])
    assert np.array_equal(counts["checked"], got["checked"])
    assert np.array_equal(risk["exp_wrong_split"], got["exp_wrong_split"]) and np.array_equal(risk["exp_wrong_stop"], got["exp_wrong_stop"])


def _promises(got, grid):
    tl._promises(got, grid)                                                          # costs fall strictly, one coordinate moves per rung, ...
    assert int(got["risk"][0]) == 0                                                  # the full search forces nothing


@pytest.mark.parametrize("grid,max_rungs", [(8, 40), (1, 9)])
def test_the_walk_on_frames_with_edge_ctus(pkg, sim, grid, max_rungs):
    """(the restatement evaluates every candidate of every step in numpy: the paths are cut at 40 and 9 rungs to keep it to seconds; the
    whole grid-64 path is walked below, the whole grid-8 path on the small set)"""
    _fill(sim, "frames")
    _table(pkg, "identity")
    want = _want("frames", "identity", None, grid, max_rungs)
    got = sim.build_ladder_risk(grid=grid, max_rungs=max_rungs)
    _same(got, want)
    _witness(sim, got)
    _promises(got, grid)
    assert len(want) == max_rungs and len({r["coord"] for r in want[1:]}) >= 2


@pytest.mark.parametrize("table", ["identity", "fitted", "random"])
def test_the_whole_path_under_each_table(pkg, sim, table):
    _fill(sim, "frames")
    sim.set_reliability(_table(pkg, table))
    want = _want("frames", table, None, 64)
    got = sim.build_ladder_risk(grid=64)
    _same(got, want)
    _witness(sim, got)
    _promises(got, 64)
    assert len(want) > 5
    if table == "identity":
        assert len(want) > 30 and len({r["coord"] for r in want[1:]}) == 6            # a long path on which every threshold moves


def test_the_small_set_whole_path_and_short_ladders(pkg, sim):
    _fill(sim, "small")
    _table(pkg, "identity")
    want = _want("small", "identity", None, 8)
    got = sim.build_ladder_risk(grid=8)
    _same(got, want)
    _witness(sim, got)
    _promises(got, 8)
    assert len(want) > 65                                                            # more than one batch of steps
    for max_rungs in (1, 2):
        got = sim.build_ladder_risk(grid=8, max_rungs=max_rungs)
        _same(got, _want("small", "identity", None, 8, max_rungs))
        assert len(got["cost"]) == max_rungs
    again = sim.build_ladder_risk(grid=8)                                            # a second build gives the same bytes
    first = sim.build_ladder_risk(grid=8)
    for k in ("thr", "coord", "value", "checked", "exp_wrong_split", "exp_wrong_stop"):
        assert first[k].tobytes() == again[k].tobytes(), k
    weights = (2 ** 32 - 1,) * 4                                                     # cross products that need more than 64 bits
    _same(sim.build_ladder_risk(weights, grid=64), _want("small", "identity", weights, 64))


def test_both_walks_back_to_back_on_one_simulator_share_no_state(pkg, sim):
    """The two builds run through one host walk.  Same weights, grid 8 and 65 rungs (one past a batch of 64 steps, so each build looks at
    the state block twice): the labelled ladder, the ladder by risk and the labelled one again on one simulator.  Anything one walk left
    behind for the other -- state words, table rows of the other width, rungs of the other size -- would change a rung."""
    _fill(sim, "frames")
    _table(pkg, "identity")
    first = sim.build_ladder(grid=8, max_rungs=65)
    by_risk = sim.build_ladder_risk(grid=8, max_rungs=65)
    again = sim.build_ladder(grid=8, max_rungs=65)
    for k in ("thr", "coord", "value", "checked", "bad_ctus"):
        assert first[k].tobytes() == again[k].tobytes(), k
    assert [int(x) for x in first["cost"]] == [int(x) for x in again["cost"]]
    tl._same(first, tl._want("frames", None, 8, 65))
    tl._same(again, tl._want("frames", None, 8, 65))
    _same(by_risk, _want("frames", "identity", None, 8, 65))
    assert len(first["cost"]) == len(by_risk["cost"]) == 65                          # both paths are longer: the cut is the second batch's


def test_the_cap_takes_moves_away(pkg, sim):
    s = _fill(sim, "frames")
    _table(pkg, "identity")
    free = _want("frames", "identity", None, 64)
    counted = s.ctus - s.rejected
    cap = free[len(free) // 2]["risk"] * 10 ** 6 // (counted * rref.ONE)            # expected wrong nodes per million CTUs at the middle of the free path
    capped = _want("frames", "identity", None, 64, 4096, cap)
    got = sim.build_ladder_risk(grid=64, max_risk_ppm=cap)
    _same(got, capped)
    _witness(sim, got)
    assert 1 < len(capped) < len(free) and _STATS["frames", "identity", None, 64, 4096, cap]["capped"] > 0
    assert all(int(r) * 10 ** 6 <= cap * counted * rref.ONE for r in got["risk"])
    got = sim.build_ladder_risk(grid=64, max_risk_ppm=0)                             # the full search has no risk: rung 0 is always there
    _same(got, _want("frames", "identity", None, 64, 4096, 0))
    assert len(got["cost"]) >= 1 and not any(int(r) for r in got["risk"])


def test_sets_without_labels_build_and_the_per_ctu_layout(pkg, sim):
    e = pkg.ethcnn
    _fill(sim, "odd")
    _table(pkg, "identity")
    with pytest.raises(pkg.EthCnnError) as err:                                      # the labelled walk still refuses such a set
        sim.build_ladder(grid=128)
    assert err.value.code == e.ERR_ARG and "labelled" in str(err.value)
    got = sim.build_ladder_risk(grid=128)
    _same(got, _want("odd", "identity", None, 128))
    _witness(sim, got)
    _promises(got, 128)
    assert len(got["cost"]) > 5
    sim.reset()
    _fill(sim, "perctu")                                                             # labelled, plain and one rejected CTU: all but the last count
    got = sim.build_ladder_risk(grid=128)
    _same(got, _want("perctu", "identity", None, 128))
    _witness(sim, got)


def test_build_refusals_leave_the_outputs_untouched(pkg, sim):
    e = pkg.ethcnn
    rungs, n = np.full(4, 7, e.LADDER_RUNG_RISK), ctypes.c_int64(-5)
    call = lambda w, grid, max_rungs, ppm: sim.lib.ethcnn_risk_ladder_build(sim.h, w, grid, max_rungs, ppm, rungs.ctypes.data, ctypes.byref(n))
    w = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
    assert call(w, 64, 4, 5) == e.ERR_ARG                                            # an empty set
    bad = np.full((3, 21), np.nan, np.float32)
    sim.add(bad)
    assert call(w, 64, 4, 5) == e.ERR_ARG and "valid probabilities" in sim.ctx.lib.ethcnn_last_error(sim.ctx.h).decode()   # rejected CTUs only
    _fill(sim, "small")
    wbig = (ctypes.c_uint64 * 4)(64, 16, 4, 2 ** 32)
    for args in ((w, 3, 4, 5), (w, 0, 4, 5), (w, 2048, 4, 5), (w, 64, 0, 5), (w, 64, 4097, 5), (wbig, 64, 4, 5)):
        assert call(*args) == e.ERR_ARG, args[1:]
    assert sim.lib.ethcnn_risk_ladder_build(sim.h, w, 64, 4, 5, None, ctypes.byref(n)) == e.ERR_ARG
    assert n.value == -5 and (rungs["coord"] == 7).all() and (rungs["exp_wrong_stop"] == 7).all()
    assert call(None, 64, 4, 2 ** 64 - 1) == 0 and 1 <= n.value <= 4 and (rungs["coord"][n.value:] == 7).all()   # NULL weight: 64 16 4 1
    for bad in (dict(grid=3), dict(max_rungs=0), dict(max_rungs=4097), dict(max_risk_ppm=-1), dict(max_risk_ppm=2 ** 64), dict(weights=(1, 2, 3, 2 ** 32))):
        with pytest.raises(pkg.EthCnnError) as err:
            sim.build_ladder_risk(**bad)
        assert err.value.code == e.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the hinge ---
def test_tools_build_without_labels_and_the_controller_holds_its_budget(pkg, tmp_path):
    frames = 6
    pp, lp, s = tl._write_case(tmp_path, frames)
    e = pkg.ethcnn
    table = _table(pkg, "fitted")
    e.risk_write(str(tmp_path / "rel.txt"), table)
    nolabels = ["--case", "-", pp, str(tl.W), str(tl.H)]
    r = subprocess.run([sys.executable, BUILD_TOOL, "--no-labels", "--reliability", "rel.txt", "--grid", "64", "--rungs", "9", "--out", "ladder.txt", "--order",
                        "ai", "--csv", "ladder.csv"] + nolabels, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = ref.Set()
    plain.add_frames(tl._case("frames")[0][:frames], None, tl.W, tl.H)
    path = rref.build(plain, table, None, 64)
    keep = lref.thin([x["cost"] for x in path], 9)
    up, down = [path[i]["up_k"] for i in keep], [path[i]["down_k"] for i in keep]
    assert len(path) > 9 and open(str(tmp_path / "ladder.txt")).read() == lref.ladder_lines(up, down, "ai")
    rows = [line.split(",") for line in open(str(tmp_path / "ladder.csv")).read().strip().splitlines()]
    assert rows[0] == ("up0,up1,up2,down0,down1,down2,cost,share,exp_wrong_split0,exp_wrong_split1,exp_wrong_split2,exp_wrong_stop0,exp_wrong_stop1,"
                       "exp_wrong_stop2,moved").split(",") and len(rows) == 1 + len(keep)
    for row, i in zip(rows[1:], keep):
        x = path[i]
        assert [int(v) for v in row[:7]] == x["up_k"] + x["down_k"] + [x["cost"]] and row[7] == "%.6f" % (x["cost"] / path[0]["cost"])
        assert row[8:14] == ["%.3f" % (v / float(rref.ONE)) for v in x["exp_wrong_split"] + x["exp_wrong_stop"]]
        assert row[14] == ("-" if x["coord"] < 0 else ref.COORDS[x["coord"]])
    assert "%d rungs built" % len(path) in r.stderr and "without labels" in r.stderr and "rel.txt" in r.stderr
    # the controller reads that file and holds a budget with it
    r = subprocess.run([sys.executable, CONTROL_TOOL, "--budget", "0.5", "--mode", "carry", "--ladder", "ladder.txt", "--order", "ai", "--out", "cu_depth.dat",
                        "--case", lp, pp, str(tl.W), str(tl.H)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ladder = ref.thr(up, down)
    rung, over, cost, full = bref.choose(bref.cost(s, ladder, 0, tl.PER, frames), bref.WEIGHTS, 500000, bref.CARRY)
    assert open(str(tmp_path / "cu_depth.dat"), "rb").read() == bref.bake(s, ladder, rung, 0, tl.PER, frames).tobytes()
    assert "%.6f of the full search over %d frames, %d over budget" % (sum(cost) / sum(full), frames, sum(over)) in r.stderr and max(rung) > 0
    assert sum(cost) * 2 <= sum(full) or sum(over) > 0                               # the budget is held wherever the ladder reaches that low
    # the simulator tool prints the expected counts beside the check counts, with labels or without
    (tmp_path / "thr.txt").write_text("0.6 0.4 0.7 0.3 0.8 0.2\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "simulate_thresholds.py"), "--thr-info", "thr.txt", "--order", "ai", "--gates", "none",
                        "--reliability", "rel.txt"] + nolabels, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cand = ref.thr((614, 717, 819), (410, 307, 205))                                 # round(v * 1024)
    split, stop = rref.evaluate(plain, cand, table)
    for d, size in enumerate(("64x64", "32x32", "16x16")):
        assert "%-5s  expected wrongly split %.3f  expected wrongly stopped %.3f" % (size, split[0][d] / float(rref.ONE), stop[0][d] / float(rref.ONE)) in r.stdout
    assert "table: rel.txt" in r.stdout and "bad CTUs" not in r.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]


def test_the_calibrator_tool_writes_the_table_of_its_histogram(pkg, tmp_path):
    pp, lp, s = tl._write_case(tmp_path, 6)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "calibrate_thresholds.py"), "--hist", "hist.dat", "--reliability-out", "rel.txt", "--case", lp, pp,
                        str(tl.W), str(tl.H)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    hist = np.fromfile(str(tmp_path / "hist.dat"), "<u8").reshape(3, 2, 1025)
    assert hist.sum() > 0 and open(str(tmp_path / "rel.txt")).read() == rref.table_text(rref.from_hist(hist))


def test_launcher_builds_the_ladder_of_the_file_it_predicts(pkg, tmp_path):
    w, h, frames, qp, seed, gain = 208, 144, 3, 32, 9, 8.0
    rng = np.random.default_rng(5)
    yuv = rng.integers(0, 256, size=(frames, w * h * 3 // 2), dtype=np.uint8)
    yuv[1, :w * h] = (yuv[1, :w * h] // 32 + 90).astype(np.uint8)   # a smoother frame
    yuv.tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text("0.75 0.25 0.75 0.25 0.75 0.25\n")
    table = _table(pkg, "fitted")
    pkg.ethcnn.risk_write(str(tmp_path / "rel.txt"), table)
    base = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET") and k != "ETHCNN_DEVICES"}
    base.update(ETHCNN_SYNTHETIC_SEED=str(seed), ETHCNN_HEAD_GAIN=str(gain), ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="auto")
    baked = {}
    for which, extra in (("identity", {}), ("fitted", {"ETHCNN_SEARCH_BUDGET_RELIABILITY": "rel.txt"})):
        r = subprocess.run([sys.executable, LAUNCHER, "seq.yuv", str(w), str(h), str(qp)], cwd=str(tmp_path), env=dict(base, **extra), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0 and "search budget 0.4 (frame)" in r.stderr and "rungs built from the predictions of 3 frames" in r.stderr, r.stderr
        baked[which] = (tmp_path / "cu_depth.dat").read_bytes()
        os.remove(str(tmp_path / "cu_depth.dat"))
    with pkg.EthCnn(device=0) as own:   # predict with open gates, then build_ladder_risk, then budget_control
        own.load_synthetic(seed, gain)
        own.set_thresholds(0.0, 0.0)
        own.predict_yuv_file(str(tmp_path / "seq.yuv"), w, h, qp, str(tmp_path / "open.dat"))
        probs = np.fromfile(str(tmp_path / "open.dat"), dtype="<f4")
        with pkg.PartitionSim(own) as s:
            s.add_frames(probs, None, w, h)
            for which, rel in (("identity", None), ("fitted", table)):
                s.set_reliability(rel)
                ladder = s.build_ladder_risk(None, 8, 4096)["thr"]
                assert len(ladder) > 1
                assert baked[which] == s.budget_control(0.4, "frame", ladder, width=w, height=h)["probs"].tobytes(), which
    assert sorted(os.listdir(str(tmp_path))) == ["Thr_info.txt", "open.dat", "rel.txt", "seq.yuv"]


@pytest.mark.parametrize("which", ["python", "native"])
def test_both_daemons_refuse_auto(pkg, tmp_path, which):
    cmd = ([sys.executable, os.path.join(ROOT, "resi_to_cu_depth_LDP.py"), "--python"] if which == "python" else [os.path.join(BIN, "resi_to_cu_depth_ldp"), "--quiet"])
    (tmp_path / "Thr_info.txt").write_text("0.25 0.75 0.25 0.75 0.25 0.75\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    env.update(ETHCNN_SYNTHETIC_SEED="1", ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="auto")
    r = subprocess.run(cmd + ["--max-frames", "0", "--idle-timeout", "0"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ETHCNN_SEARCH_BUDGET_LADDER='auto'" in r.stderr and "cannot see the sequence in advance" in r.stderr, r.stderr[-300:]
    assert os.listdir(str(tmp_path)) == ["Thr_info.txt"]
