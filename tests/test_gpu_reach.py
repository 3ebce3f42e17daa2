"""-m gpu: the threshold calibration on reached nodes (include/ethcnn.h "threshold calibration on reached nodes") on the GPU.
k_reach_hist is compared with the restatement (tests/reach_ref.py) on sets at which slices, partial waves, unlabelled and rejected CTUs,
frame edges and closed batch gates occur, with the simulator's own evaluation through the identities of the header, and with a second
witness: the per-node codes of PartitionSim.decide histogrammed in numpy.  The top-down choice is compared field by field with the
restatement's, and the tool's files with both.  Integers only: every comparison is equality."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import decide_ref as dref
import reach_ref as rr
import risk_ref as rref
import sim_ref as ref
import test_gpu_ladder as tl   # the frames / small / perctu cases are those of the labelled walk, made once and never changed
import test_reach_cpu as rc    # the candidates and the identities of the CPU tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "calibrate_thresholds.py")
GATE_W, GATE_H = 2112, 2048
GATES = (("none", ref.GATES_NONE), ("ai", ref.GATES_AI), ("ldp", ref.GATES_LDP))
FULL = ref.thr(*ref.FULL)
_CASES = {}


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _case(name):
    """-> (list of add calls, Set), made once and never changed: an add call is ("frames", probs, labels, w, h) or ("ctus", probs, depth16
    or None)"""
    if name not in _CASES:
        if name == "frames":
            c = tl._case(name)
            adds = [("frames", c[0], c[1], tl.W, tl.H)]
        elif name in ("small", "perctu"):
            c = tl._case(name)
            adds = [("ctus", c[0], c[1])] + ([("ctus", c[2], None)] if c[2].shape[0] else [])
        elif name == "gates":
            probs, labels = dref.gate_case(np.random.default_rng(2112))
            adds = [("frames", probs, labels, GATE_W, GATE_H)]
        elif name == "tiny":     # fewer CTUs than a wave, in several adds, the last one without labels
            rng = np.random.default_rng(51)
            adds = [("ctus", calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)) for n in (17, 1, 19)] + [("ctus", calib_ref.edge_probs(rng, 5), None)]
        elif name == "wave65":   # one CTU past a wave
            rng = np.random.default_rng(52)
            adds = [("ctus", calib_ref.edge_probs(rng, 65), calib_ref.random_depths(rng, 65))]
        elif name == "saturated":   # every probability 0 or 1: all adds of a level and truth land in two words
            rng = np.random.default_rng(53)
            adds = [("ctus", rng.integers(0, 2, size=(4096, 21)).astype(np.float32), calib_ref.random_depths(rng, 4096))]
        elif name == "grid":     # grid values k / 1024 and their fp32 neighbours
            rng = np.random.default_rng(54)
            adds = [("ctus", calib_ref.edge_probs(rng, 1000), calib_ref.random_depths(rng, 1000))]
        s = ref.Set()
        for call in adds:
            if call[0] == "frames":
                s.add_frames(call[1], call[2], call[3], call[4])
            else:
                s.add(call[1], call[2])
        _CASES[name] = (adds, s)
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


def _cands():
    """69 candidates for calls of 1, 3 and 65: the full search, crossed ones and the ends of the ranges among them; two that close gates
    over nodes whose sub-CUs are still visited (tests/test_reach_cpu.py)"""
    c = rc._cands(55, 69)
    c[7] = ref.thr((600, 700, 800), (300, 300, 200))
    c[8] = ref.thr((400, 650, 800), (500, 300, 200))
    return c


def _hist_in_three_calls(sim, cands, gates):
    got = np.concatenate([sim.reach_hist(cands[:1], gates), sim.reach_hist(cands[1:4], gates), sim.reach_hist(cands[4:], gates)])
    assert got.dtype == np.uint64 and got.shape == (cands.size, 3, 2, 1025)
    return got


@pytest.mark.parametrize("name", ["tiny", "perctu", "small", "frames", "wave65", "gates", "saturated", "grid"])
def test_reach_hist_against_the_restatement_and_the_evaluation(sim, name):
    s = _fill(sim, name)
    info = sim.info()
    assert (info["ctus"], info["labelled_ctus"], info["rejected_ctus"]) == (s.ctus, int(s.labelled.sum()), s.rejected)
    if name == "frames":
        assert info["labelled_ctus"] * 2 == info["ctus"]                                       # half the CTUs are partial and carry no label
    cands = _cands()
    seen = {}
    for gates, g in GATES:
        got = _hist_in_three_calls(sim, cands, gates)
        assert np.array_equal(got, rr.reach_hist(s, cands, g)), gates
        rc.check_identities(s, cands, g, got, sim.eval(cands, gates))                          # the wrong decisions of k_sim_eval are sums over it
        assert int(got[1].sum()) == 21 * info["labelled_ctus"]                                 # candidate 1, the full search, reaches every node
        seen[gates] = got
    if name == "gates":                                                                        # closed gates moved bins to 0
        assert not np.array_equal(seen["ldp"][7], seen["none"][7]) and not np.array_equal(seen["ai"][8], seen["none"][8])
    elif name != "frames":                                                                     # the per-CTU layout is never gated
        assert seen["ai"].tobytes() == seen["none"].tobytes() == seen["ldp"].tobytes()
    if name == "saturated":
        assert seen["none"][:, :, :, 1:1024].sum() == 0 and seen["none"][1, 2, :, 0].min() > 1000


def test_second_witness_the_partition_decisions_histogrammed_in_numpy(sim):
    probs, depth = tl._case("perctu")[:2]
    _fill(sim, "perctu")
    d = depth.astype(np.int64)
    truth = np.zeros((d.shape[0], 21), bool)
    truth[:, 0], truth[:, 1:5], truth[:, 5:] = d.sum(axis=1) > 8, d[:, calib_ref.IDX32].sum(axis=2) > 6, d == 3
    bins = calib_ref.bins_of(probs)[0]
    cands = _cands()[[0, 1, 3, 9, 10]]
    got = sim.reach_hist(cands, "none")
    for i in range(cands.size):
        codes = sim.decide(cands[i], "none", want=("codes",))["codes"][:d.shape[0]]            # (the rows behind them carry no label)
        decided = np.isin(codes[:, :21] & 7, (1, 2, 3)) & ((codes[:, 21:22] & 2) != 0)         # current / split / both, on labelled CTUs
        for l, (a, b) in enumerate(rr.SPANS):
            for t in (0, 1):
                pick = decided[:, a:b] & (truth[:, a:b] == bool(t))
                assert np.array_equal(got[i, l, t], np.bincount(bins[:, a:b][pick], minlength=1025).astype(np.uint64)), (i, l, t)
    assert got[0].sum() < got[1].sum() == 21 * 1299


def test_counts_do_not_depend_on_how_the_set_was_added(sim):
    probs, labels, s = tl._case("frames")
    cands = _cands()[:12]
    sim.add_frames(probs, labels, tl.W, tl.H)
    whole = {g: sim.reach_hist(cands, g) for g, _ in GATES}
    sim.reset()
    for f in range(probs.shape[0]):                                                            # frame by frame
        sim.add_frames(probs[f:f + 1], labels[f:f + 1], tl.W, tl.H)
    assert all(sim.reach_hist(cands, g).tobytes() == whole[g].tobytes() for g, _ in GATES)
    sim.reset()
    sim.add_frames(probs[11:], labels[11:], tl.W, tl.H)                                        # another order, other sub-batch numbers
    sim.add_frames(probs[:11], labels[:11], tl.W, tl.H)
    assert all(sim.reach_hist(cands, g).tobytes() == whole[g].tobytes() for g, _ in GATES)
    assert np.array_equal(whole["ldp"], rr.reach_hist(s, cands, ref.GATES_LDP))
    sim.reset()
    p, d, plain, s2 = tl._case("perctu")
    for a, b in ((700, 1300), (0, 64), (64, 700)):                                             # per-CTU pieces, shuffled, the plain CTUs in between
        sim.add(p[a:b], d[a:b])
        sim.add(plain[a:b])
    assert np.array_equal(sim.reach_hist(cands), rr.reach_hist(s2, cands))


def test_a_second_call_after_reset_and_refill_gives_the_same_bytes(sim):
    _fill(sim, "gates")
    cands = _cands()
    first = sim.reach_hist(cands, "ldp")
    rep1, thr1, counts1 = sim.calibrate_reached(20000, 20000, "ldp")
    sim.reset()
    _fill(sim, "small")
    other = sim.reach_hist(cands, "ldp")
    sim.reset()
    _fill(sim, "gates")
    assert sim.reach_hist(cands, "ldp").tobytes() == first.tobytes() != other.tobytes()
    rep2, thr2, counts2 = sim.calibrate_reached(20000, 20000, "ldp")
    assert bytes(rep1) == bytes(rep2) and thr1.tobytes() == thr2.tobytes() and counts1.tobytes() == counts2.tobytes()


def test_empty_inputs(pkg, sim):
    e = pkg.ethcnn
    cands = _cands()[:5]
    assert not sim.reach_hist(cands).any()                                                     # an empty set
    sim.add(tl._case("perctu")[2])                                                             # CTUs, but no label on any
    sim.add_frames(tl._case("frames")[0], None, tl.W, tl.H)
    out = np.full((5, 3, 2, 1025), 7, np.uint64)
    assert sim.lib.ethcnn_reach_hist(sim.h, cands.ctypes.data, 5, 0, out.ctypes.data) == 0 and not out.any()
    out[:] = 7
    assert sim.lib.ethcnn_reach_hist(sim.h, cands.ctypes.data, 0, 0, out.ctypes.data) == 0 and (out == 7).all()   # no candidate: a no-op
    assert sim.lib.ethcnn_reach_hist(sim.h, None, 0, 0, None) == 0 and sim.reach_hist(cands[:0]).shape == (0, 3, 2, 1025)
    rep, thr, counts = e.CalibReport(), np.full(1, 7, e.SIM_THR), np.full(1, 7, e.SIM_COUNTS)
    eps = (ctypes.c_uint32 * 3)(50000, 50000, 50000)
    assert sim.lib.ethcnn_reach_calibrate(sim.h, eps, eps, 0, ctypes.byref(rep), thr.ctypes.data, counts.ctypes.data) == e.ERR_ARG   # no labelled CTU
    assert "labelled" in sim.ctx.lib.ethcnn_last_error(sim.ctx.h).decode()
    assert (thr["up_k"] == 7).all() and (counts["checked"] == 7).all() and rep.level[1].n0 == 0


@pytest.mark.parametrize("name", ["frames", "gates"])
def test_calibrate_reached_field_by_field(pkg, sim, name):
    s = _fill(sim, name)
    crossed = 0
    for gates, g in GATES:
        for eps_down, eps_up in ((0, 0), (20000, 20000), (10 ** 6, 10 ** 6), ((0, 50000, 300000), (100000, 0, 20000))):
            rep, thr, counts = sim.calibrate_reached(eps_down, eps_up, gates)
            as3 = lambda x: x if isinstance(x, tuple) else (x,) * 3
            levels, want_thr, want_counts = rr.calibrate_reached(s, as3(eps_down), as3(eps_up), g)
            assert rep.as_dicts() == levels, (gates, eps_down, eps_up)
            assert thr.tobytes() == np.asarray(want_thr).tobytes() and ref.equal(counts, want_counts)
            for l, lv in enumerate(rep.level):
                assert (int(counts["wrong_stop"][l]), int(counts["wrong_split"][l])) == (lv.miss, lv.fsplit)
                crossed += lv.crossed
            assert ref.equal(sim.eval(thr, gates)[0], counts)
    assert crossed > 0                                                                         # crossed levels are among them (budgets of 10^6)


def test_refusals_write_nothing(pkg, sim):
    e = pkg.ethcnn
    _fill(sim, "small")
    cands = np.repeat(FULL.reshape(1), 257)
    out = np.full((257, 3, 2, 1025), 7, np.uint64)
    hist = lambda c, n, g, o: sim.lib.ethcnn_reach_hist(sim.h, None if c is None else c.ctypes.data, n, g, None if o is None else o.ctypes.data)
    assert hist(cands, 257, 0, out) == e.ERR_ARG and "257" in sim.ctx.lib.ethcnn_last_error(sim.ctx.h).decode()
    assert hist(cands, -1, 0, out) == e.ERR_ARG and hist(cands, 4, 3, out) == e.ERR_ARG and hist(cands, 4, -1, out) == e.ERR_ARG
    assert hist(cands, 4, 0, None) == e.ERR_ARG and hist(None, 4, 0, out) == e.ERR_ARG
    for up, down in (((1025, 5, 5), (0, 0, 0)), ((5, 5, -1), (0, 0, 0)), ((5, 5, 5), (0, -2, 0)), ((5, 5, 5), (0, 0, 1025))):
        bad = cands[:4].copy()
        bad[2] = ref.thr(up, down)
        assert hist(bad, 4, 0, out) == e.ERR_ARG
    assert (out == 7).all()
    assert hist(cands, 256, 0, out) == 0 and (out[:256] == out[0]).all() and (out[256] == 7).all() and out[0].sum() == 21 * 60   # the cap itself is served
    with pytest.raises(pkg.EthCnnError) as err:
        sim.reach_hist(cands)
    assert err.value.code == e.ERR_ARG
    rep, thr, counts = e.CalibReport(), np.full(1, 7, e.SIM_THR), np.full(1, 7, e.SIM_COUNTS)
    ok, over = (ctypes.c_uint32 * 3)(50000, 50000, 50000), (ctypes.c_uint32 * 3)(50000, 10 ** 6 + 1, 50000)
    cal = lambda dn, up, g, r, t: sim.lib.ethcnn_reach_calibrate(sim.h, dn, up, g, r, t, counts.ctypes.data)
    assert cal(over, ok, 0, ctypes.byref(rep), thr.ctypes.data) == e.ERR_ARG and cal(ok, over, 0, ctypes.byref(rep), thr.ctypes.data) == e.ERR_ARG
    assert cal(ok, ok, 3, ctypes.byref(rep), thr.ctypes.data) == e.ERR_ARG and cal(ok, ok, 0, None, thr.ctypes.data) == e.ERR_ARG
    assert cal(ok, ok, 0, ctypes.byref(rep), None) == e.ERR_ARG and cal(None, ok, 0, ctypes.byref(rep), thr.ctypes.data) == e.ERR_ARG
    assert (thr["down_k"] == 7).all() and (counts["bad_ctus"] == 7).all() and rep.level[0].n1 == 0
    assert sim.lib.ethcnn_reach_calibrate(sim.h, ok, ok, 0, ctypes.byref(rep), thr.ctypes.data, None) == 0 and rep.level[0].n0 + rep.level[0].n1 == 60   # counts_out may be NULL
    with pytest.raises(ValueError):
        sim.calibrate_reached(10 ** 6 + 1, 0)


def test_the_fitted_table_goes_into_the_expected_wrong_decisions(pkg, sim):
    """the chain the histogram exists for: the table fitted to the full-search reach histogram, installed, prices forced decisions"""
    s = _fill(sim, "frames")
    hist = sim.reach_hist(FULL, "none")[0]
    table = pkg.ethcnn.risk_from_hist(hist)
    assert np.array_equal(table, rref.from_hist(rr.reach_hist(s, FULL)[0])) and not np.array_equal(table, rref.identity())
    teacher = calib_ref.histogram_frames(tl._case("frames")[0], tl._case("frames")[1], tl.W, tl.H)[0]
    assert not np.array_equal(table[1:], rref.from_hist(teacher)[1:])                          # not the table of the teacher-forced populations
    sim.set_reliability(table)
    cands = _cands()[:20]
    split, stop = rref.evaluate(s, cands, table)
    got = sim.eval_risk(cands)
    assert got["exp_wrong_split"].tolist() == split and got["exp_wrong_stop"].tolist() == stop


def test_tool_reached_and_the_unchanged_default(pkg, sim, tmp_path):
    frames = 6
    pp, lp, s = tl._write_case(tmp_path, frames)
    case = ["--case", lp, pp, str(tl.W), str(tl.H)]
    e = pkg.ethcnn
    r = subprocess.run([sys.executable, TOOL, "--reached", "--out", "T.txt", "--order", "ldp", "--reliability-out", "R.txt", "--hist", "H.dat", "--json"] + case,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    eps = (50000,) * 3
    levels, thr, counts = rr.calibrate_reached(s, eps, eps, ref.GATES_LDP)                     # --gates defaults to --order's value
    assert open(str(tmp_path / "T.txt")).read() == calib_ref.thr_info_line(levels, "ldp")
    full = rr.reach_hist(s, FULL)[0]
    assert np.array_equal(np.fromfile(str(tmp_path / "H.dat"), "<u8").reshape(3, 2, 1025), full)
    assert np.array_equal(e.risk_read(str(tmp_path / "R.txt")), e.risk_from_hist(full))
    got = json.loads(r.stdout)
    sim.add_frames(tl._case("frames")[0][:frames], tl._case("frames")[1][:frames], tl.W, tl.H)
    ev = sim.eval(thr, "ldp")[0]
    assert got["reached"] is True and got["gates"] == "ldp" and got["levels"] == levels
    assert got["thr"] == {"up_k": [int(x) for x in thr["up_k"]], "down_k": [int(x) for x in thr["down_k"]]}
    assert got["counts"] == {f: [int(x) for x in np.atleast_1d(ev[f])] for f in ref.FIELDS} and ref.equal(ev, counts)
    # the text form: the reached populations, the checks per CU size and their weighted share
    r = subprocess.run([sys.executable, TOOL, "--reached", "--gates", "none"] + case, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    levels, thr, counts = rr.calibrate_reached(s, eps, eps, ref.GATES_NONE)
    fullc = s.evaluate(FULL)[0]
    cost = lambda c: sum(w * int(x) for w, x in zip((64, 16, 4, 1), c["checked"]))
    assert "32x32  reached unsplit %d  reached split %d" % (levels[1]["n0"], levels[1]["n1"]) in r.stdout
    assert "16x16  checked %d of %d\n" % (int(counts["checked"][2]), int(fullc["checked"][2])) in r.stdout
    assert "%.6f of the full search (weights 64 16 4 1)" % (cost(counts) / cost(fullc)) in r.stdout
    # without --reached: what the tool gave before, the calibrator's teacher-forced choice
    for f in ("T.txt", "R.txt", "H.dat"):
        os.remove(str(tmp_path / f))
    r = subprocess.run([sys.executable, TOOL, "--out", "T.txt", "--order", "ldp", "--hist", "H.dat", "--json"] + case, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    hist, rejected, skipped = calib_ref.histogram_frames(tl._case("frames")[0][:frames], tl._case("frames")[1][:frames], tl.W, tl.H)
    forced = calib_ref.choose(hist, eps, eps)
    assert json.loads(r.stdout) == {"levels": forced, "rejected": [int(x) for x in rejected], "skipped_partial": skipped, "eps_down_ppm": list(eps),
                                    "eps_up_ppm": list(eps), "out": "T.txt", "order": "ldp"}
    assert open(str(tmp_path / "T.txt")).read() == calib_ref.thr_info_line(forced, "ldp")
    assert np.array_equal(np.fromfile(str(tmp_path / "H.dat"), "<u8").reshape(3, 2, 1025), hist)
    with pkg.Calibrator(sim.ctx) as cal:
        cal.add_frames(tl._case("frames")[0][:frames], tl._case("frames")[1][:frames], tl.W, tl.H)
        assert np.array_equal(cal.histogram(), hist) and cal.choose(eps, eps).as_dicts() == forced
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
