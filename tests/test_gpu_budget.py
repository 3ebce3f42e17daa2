"""-m gpu: the search budget (include/ethcnn.h "search budget") on the GPU.  The two kernels against the numpy restatement
(tests/budget_ref.py) byte for byte, against the existing decisions kernel as a second witness, and through "the hinge": the baked rows,
read back under the companion thresholds, make ethcnn_decide reproduce the decisions of every frame's own rung.  Probabilities are
synthetic, on the k / 1024 grid, with values exactly at up and down of several rungs and a spread that differs from frame to frame, so
that the chosen rungs differ.  Integers and three constants only: every comparison is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_ref as bref
import decide_ref as dref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "control_budget.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
COMPANION = ref.thr(*bref.COMPANION)
MODES = {"frame": bref.FRAME, "carry": bref.CARRY}
# name: width, height, frames, label frames skipped (None: no labels), CTU that carries a NaN (None: none)
SHAPES = {"labelled": (208, 144, 30, 1, 3 * 12 + 5),  # 4 x 3 CTUs, partial right and bottom; a 256-lane block spans 21 frames and starts mid-frame
          "ragged": (200, 136, 7, None, None),         # 16 x 16 edge nodes with a single 8 x 8 inside
          "wide": (1088, 1024, 3, None, None),         # 272 CTUs: a frame crosses a block
          "nan": (64, 64, 1, None, 0)}                 # one CTU, rejected
_CASES, _LADDERS, _COSTS = {}, {}, {}


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _case(name):
    """(probs [F, per, 21], labels or None, skip, sim_ref.Set) made once and never changed"""
    if name not in _CASES:
        w, h, frames, skip, nan_at = SHAPES[name]
        per = ((w + 63) // 64) * ((h + 63) // 64)
        rng = np.random.default_rng(sum(map(ord, name)))
        k = rng.integers(0, 1025, size=(frames, per, 21))
        spread = np.linspace(0.05, 1.0, frames)[rng.permutation(frames)]           # frames near 0.5 are dear, spread-out frames cheap
        k = 512 + np.rint((k - 512) * spread[:, None, None]).astype(np.int64)
        at_rung = rng.choice(np.array([1024 - 100, 99, 1024 - 300, 299, 512, 511, 1024, 0, 768, 256]), size=k.shape)
        k = np.where(rng.integers(0, 6, size=k.shape) == 0, at_rung, k)             # exactly at up / down of rungs 100, 300, 512, 0
        probs = (k / 1024.0).astype(np.float32)
        if nan_at is not None:
            probs.reshape(-1, 21)[nan_at, 7] = np.nan
        labels = None
        if skip is not None:
            labels = rng.integers(0, 4, size=(frames + skip, h // 16, w // 16)).astype(np.uint8)
        s = ref.Set()
        s.add_frames(probs, labels, w, h, skip or 0)
        probs.setflags(write=False)
        _CASES[name] = (probs, labels, skip or 0, s)
    return _CASES[name]


def _fill(sim, name, lead=0):
    """the case in a simulator, behind `lead` CTUs in the per-CTU layout -> (Set, first CTU, per)"""
    probs, labels, skip, s = _case(name)
    w, h = SHAPES[name][:2]
    if lead:
        sim.add(np.full((lead, 21), 0.5, np.float32))
    sim.add_frames(probs, labels, w, h, skip_label_frames=skip)
    return s, lead, probs.shape[1]


def _ladder(k):
    if k not in _LADDERS:
        _LADDERS[k] = bref.default_ladder() if k == 513 else dref.candidates(np.random.default_rng(k), max(k, 4))[:k].copy()
    return _LADDERS[k]


def _cost(name, k):
    if (name, k) not in _COSTS:
        probs, _, _, s = _case(name)
        _COSTS[name, k] = bref.cost(s, _ladder(k), 0, probs.shape[1], probs.shape[0])
    return _COSTS[name, k]


@pytest.mark.parametrize("name,k", [("labelled", 1), ("labelled", 3), ("labelled", 64), ("labelled", 65), ("labelled", 513), ("ragged", 513),
                                    ("wide", 513), ("wide", 65), ("nan", 513)])
def test_cost_per_frame_and_rung(pkg, ctx, sim, name, k):
    w, h, frames = SHAPES[name][:3]
    lead = 63 if name == "labelled" else 0     # the frames do not start the set
    s, first, per = _fill(sim, name, lead)
    ladder, want = _ladder(k), _cost(name, k)
    got = sim.budget_cost(ladder if k != 513 else None, first, w, h, frames)
    assert got.dtype == np.uint32 and got.shape == (frames, k + 1, 4) and np.array_equal(got, want)
    assert got[:, :, 3].any() or name == "nan"
    # the existing decisions kernel as a second witness, on a sample of (frame, rung)
    rng = np.random.default_rng(k)
    for f, r in {(0, 0), (frames - 1, k - 1)} | {(int(rng.integers(frames)), int(rng.integers(k))) for _ in range(4)}:
        codes = sim.decide(ladder[r], "none", 512, first + f * per, per, want=("codes",))["codes"]
        assert pkg.ethcnn.sim_counts_from_codes(codes)["checked"].tolist() == got[f, r].tolist(), (f, r)
    # column K is the full search: rung 0 of the default ladder
    full = sim.budget_cost(None, first, w, h, frames)[:, 0] if k != 513 else got[:, 0]
    assert np.array_equal(got[:, k], full)
    # a window of frames, and the device form: the same bytes
    assert np.array_equal(sim.budget_cost(ladder, first + per * (frames // 2), w, h, frames - frames // 2), want[frames // 2:])
    buf = ctx.alloc(want.nbytes + 32)
    try:
        buf.upload(np.full(want.nbytes + 32, 0xAB, np.uint8))
        sim.budget_cost_device(ladder, first, w, h, frames, buf.ptr + 16)
        raw = buf.download(np.uint8, want.nbytes + 32)
    finally:
        buf.free()
    assert (raw[:16] == 0xAB).all() and (raw[-16:] == 0xAB).all() and raw[16:-16].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["labelled", "ragged", "wide", "nan"])
def test_bake_rows_guards_and_pieces(pkg, ctx, sim, name):
    w, h, frames = SHAPES[name][:3]
    lead = 63 if name == "labelled" else 0
    s, first, per = _fill(sim, name, lead)
    for k in (513, 3):
        ladder = _ladder(k)
        rung = np.random.default_rng(frames + k).integers(0, k, size=frames).astype(np.int32)
        rung[0], rung[-1] = k - 1, 0
        want = bref.bake(s, ladder, rung, 0, per, frames)
        got = sim.budget_bake(ladder, rung, first, w, h, frames)
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
        assert set(np.unique(got).tolist()) <= {0.0, 0.5, 1.0}
        # guard floats before and after a device buffer stay untouched
        n = frames * per * 21
        buf = ctx.alloc((n + 16) * 4)
        try:
            buf.upload(np.full(n + 16, 7.25, np.float32))
            sim.budget_bake_device(ladder, rung, first, w, h, frames, buf.ptr + 32)
            raw = buf.download(np.float32, n + 16)
        finally:
            buf.free()
        assert (raw[:8] == 7.25).all() and (raw[-8:] == 7.25).all() and raw[8:-8].tobytes() == want.tobytes()
        # staged in pieces that start inside a frame, and a window of frames
        sim.set_decide_piece(7 * per // 3 + 1)
        try:
            assert sim.budget_bake(ladder, rung, first, w, h, frames).tobytes() == want.tobytes()
            assert sim.budget_bake(ladder, rung[1:], first + per, w, h, frames - 1).tobytes() == want[per:].tobytes()
        finally:
            sim.set_decide_piece(0)
    if SHAPES[name][4] is not None:
        assert (got[SHAPES[name][4]] == 0.5).all()   # the rejected CTU gets the full search


@pytest.mark.parametrize("mode", ["frame", "carry"])
def test_the_hinge_an_unchanged_decision_rule_carries_out_every_frames_rung(pkg, sim, mode):
    name = "labelled"
    w, h, frames, skip, nan_at = SHAPES[name]
    probs, labels, _, s = _case(name)
    _, first, per = _fill(sim, name)
    ladder = bref.default_ladder()
    out = sim.budget_control(0.4, mode, width=w, height=h)
    assert len(set(out["rung"].tolist())) > 3 and out["rung"].max() > 0   # frames of different spread take different rungs
    baked = out["probs"]
    assert (baked[nan_at] == 0.5).all()
    with pkg.PartitionSim(sim.ctx) as again:
        again.add_frames(baked, labels, w, h, skip_label_frames=skip)
        got = again.decide(COMPANION, "none")["codes"]
    kept = np.ones(frames * per, bool)
    kept[nan_at] = False
    for f in range(frames):
        sl = slice(f * per, (f + 1) * per)
        want = sim.decide(ladder[out["rung"][f]], "none", 512, first + f * per, per, want=("codes",))["codes"]
        assert np.array_equal(want, dref.decide(s, ladder[out["rung"][f]], first=f * per, n=per)["codes"])
        assert np.array_equal(got[sl][kept[sl], :23], want[kept[sl], :23]), f
    # so the baked file's checks under the companion thresholds are the chosen rungs' costs
    counts = [pkg.ethcnn.sim_counts_from_codes(got[f * per:(f + 1) * per][kept[f * per:(f + 1) * per]])["checked"] for f in range(frames)]
    costs = [sum(wt * int(x) for wt, x in zip(bref.WEIGHTS, c)) for c in counts]
    assert costs == [int(x) for x in out["cost"]]
    if mode == "frame":
        assert all(c * 10 ** 6 <= 400000 * int(fl) for c, fl, o in zip(costs, out["full"], out["over"]) if not o)


@pytest.mark.parametrize("name,k,weights", [("labelled", 513, None), ("ragged", 65, (7, 5, 3, 2)), ("nan", 513, None)])
def test_control_is_cost_then_choose_then_bake(pkg, sim, name, k, weights):
    w, h, frames = SHAPES[name][:3]
    s, first, per = _fill(sim, name)
    ladder = _ladder(k)
    checked = sim.budget_cost(ladder, first, w, h, frames)
    seen_over = 0
    for mode in ("frame", "carry"):
        for share in (0.0, 0.25, 0.4, 0.7):
            got = sim.budget_control(share, mode, None if k == 513 else ladder, weights, first, w, h, frames)
            step = pkg.ethcnn.budget_choose(checked, weights, int(round(share * 1e6)), mode)
            want = bref.choose(_cost(name, k), weights or bref.WEIGHTS, int(round(share * 1e6)), MODES[mode])
            for key, ref_list in zip(("rung", "over", "cost", "full"), want):
                assert [int(x) for x in got[key]] == [int(x) for x in step[key]] == ref_list, (mode, share, key)
            assert got["probs"].tobytes() == sim.budget_bake(ladder, got["rung"], first, w, h, frames).tobytes()
            assert got["probs"].tobytes() == bref.bake(s, ladder, got["rung"], 0, per, frames).tobytes()
            seen_over += int(got["over"].sum())
            without = sim.budget_control(share, mode, None if k == 513 else ladder, weights, first, w, h, frames, probs=False)
            assert "probs" not in without and np.array_equal(without["rung"], got["rung"])
    assert seen_over or name == "nan"
    if k == 513:  # the whole budget: rung 0 everywhere, every decided node is left to "both"
        full = sim.budget_control(1.0, "frame", width=w, height=h, first=first, nframes=frames)
        assert not full["rung"].any() and not full["over"].any() and np.array_equal(full["cost"], full["full"])
        live = (s.inside[:, 0] | s.edge[:, 0])[:, None]
        assert np.array_equal(full["probs"] == 0.5, s.inside | ~live) and np.array_equal(full["probs"] == 1.0, s.edge)


def test_bad_arguments_leave_the_outputs_untouched(pkg, ctx, sim):
    e = pkg.ethcnn
    name = "labelled"
    w, h, frames = SHAPES[name][:3]
    _, first, per = _fill(sim, name, 63)
    lib, lad = sim.lib, np.ascontiguousarray(_ladder(3))
    bad_lad = lad.copy()
    bad_lad["up_k"][1, 2] = 1025
    rung, bad_rung, neg_rung = np.zeros(frames, np.int32), np.zeros(frames, np.int32), np.zeros(frames, np.int32)
    bad_rung[7], neg_rung[0] = 3, -1
    host = np.full(frames * per * 21, 3.5, np.float32)
    counts = np.full(frames * 4 * 4, 0xEEEEEEEE, np.uint32)
    dev = ctx.alloc(host.nbytes + 64)
    dev.upload(np.full(host.nbytes + 64, 0xEE, np.uint8))
    p = lambda a: a.ctypes.data
    try:
        # ladder, K, first, width, height, frames
        windows = [(lad, 0, first, w, h, frames), (lad, 4097, first, w, h, frames), (bad_lad, 3, first, w, h, frames), (lad, 3, first + 1, w, h, frames),
                   (lad, 3, first, w, h, frames + 1), (lad, 3, 0, w, h, 1), (lad, 3, first, h, w, 1), (lad, 3, first, 204, h, 1), (lad, 3, first, w, h, -1),
                   (lad, 3, -12, w, h, 1)]
        for l, k, f0, ww, hh, nf in windows:
            assert lib.ethcnn_budget_cost(sim.h, p(l), k, f0, ww, hh, nf, p(counts)) == e.ERR_ARG, (k, f0, ww, hh, nf)
            assert lib.ethcnn_budget_cost_device(sim.h, p(l), k, f0, ww, hh, nf, dev.ptr) == e.ERR_ARG
            assert lib.ethcnn_budget_bake(sim.h, p(l), k, p(rung), f0, ww, hh, nf, p(host)) == e.ERR_ARG
            assert lib.ethcnn_budget_bake_device(sim.h, p(l), k, p(rung), f0, ww, hh, nf, dev.ptr) == e.ERR_ARG
            assert lib.ethcnn_budget_control(sim.h, p(l), k, None, 400000, 0, f0, ww, hh, nf, p(host), None, None, None, None) == e.ERR_ARG
        for r in (bad_rung, neg_rung, None):
            assert lib.ethcnn_budget_bake(sim.h, p(lad), 3, None if r is None else p(r), first, w, h, frames, p(host)) == e.ERR_ARG
            assert lib.ethcnn_budget_bake_device(sim.h, p(lad), 3, None if r is None else p(r), first, w, h, frames, dev.ptr) == e.ERR_ARG
        assert lib.ethcnn_budget_cost(sim.h, None, 3, first, w, h, frames, p(counts)) == e.ERR_ARG
        assert lib.ethcnn_budget_cost_device(sim.h, p(lad), 3, first, w, h, frames, dev.ptr + 2) == e.ERR_ARG      # not 4-byte aligned
        assert lib.ethcnn_budget_bake_device(sim.h, p(lad), 3, p(rung), first, w, h, frames, dev.ptr + 2) == e.ERR_ARG
        wbig = (np.array([64, 16, 4, 2 ** 32], np.uint64))
        for ppm, mode, wt in ((1000001, 0, None), (400000, 2, None), (400000, 0, p(wbig))):
            assert lib.ethcnn_budget_control(sim.h, None, 0, wt, ppm, mode, first, w, h, frames, p(host), None, None, None, None) == e.ERR_ARG
        assert lib.ethcnn_budget_cost(sim.h, p(lad), 3, first + frames * per, w, h, 0, None) == 0                 # no frames: a no-op
        assert (host == 3.5).all() and (counts == 0xEEEEEEEE).all() and (dev.download(np.uint8, host.nbytes + 64) == 0xEE).all()
        with pytest.raises(pkg.EthCnnError) as err:
            sim.budget_bake(lad, bad_rung, first, w, h, frames)
        assert err.value.code == e.ERR_ARG and "rung" in str(err.value)
        with pytest.raises(ValueError):
            sim.budget_control(1.5, width=w, height=h, first=first)
    finally:
        dev.free()


def test_tool_reproduces_the_restatement_on_a_tiny_file_pair(pkg, tmp_path):
    name = "labelled"
    w, h, _, skip, _ = SHAPES[name]
    probs, labels, _, _ = _case(name)
    frames = 5
    per = probs.shape[1]
    probs, labels = probs[:frames], labels[:frames + skip]
    pp, lp = str(tmp_path / "cu_depth_in.dat"), str(tmp_path / "Info_CUDepth.dat")
    probs.tofile(pp)
    labels.tofile(lp)
    s = ref.Set()
    s.add_frames(probs, labels, w, h, skip)
    lines = ["0 1 0 1 0 1", "0.1 0.9 0.2 0.8 0.3 0.7", "0.4 0.6 0.4 0.6 0.4 0.6", "0.5 0.5 0.5 0.5 0.5 0.5"]   # LDP order: down up ...
    (tmp_path / "ladder.txt").write_text("\n".join(lines) + "\n")
    tok = np.array([[int(round(float(t) * 1024)) for t in line.split()] for line in lines])
    ladder = ref.thr(tok[:, 1::2], tok[:, 0::2])
    out, thr = str(tmp_path / "cu_depth.dat"), str(tmp_path / "Thr_info.txt")
    r = subprocess.run([sys.executable, TOOL, "--budget", "0.55", "--mode", "carry", "--ladder", "ladder.txt", "--order", "ldp", "--weights", "60", "20", "5", "1",
                        "--out", out, "--thr-out", thr, "--per-frame", "--case", lp, pp, str(w), str(h), "--skip-label-frames", str(skip)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    weights = (60, 20, 5, 1)
    rung, over, cost, full = bref.choose(bref.cost(s, ladder, 0, per, frames), weights, 550000, bref.CARRY)
    assert open(out, "rb").read() == bref.bake(s, ladder, rung, 0, per, frames).tobytes()
    assert [float(t) for t in open(thr).read().split()] == [0.25, 0.75] * 3
    rows = [line.split(",") for line in r.stdout.strip().splitlines()]
    assert rows[0] == "case,frame,rung,up0,up1,up2,down0,down1,down2,cost,full,share,over_budget,bad_ctus,labelled_ctus".split(",") and len(rows) == 1 + frames
    for f, row in enumerate(rows[1:]):
        codes = dref.decide(s, ladder[rung[f]], first=f * per, n=per)["codes"]
        want = [0, f, rung[f]] + ladder[rung[f]]["up_k"].tolist() + ladder[rung[f]]["down_k"].tolist() + [cost[f], full[f]]
        assert [int(x) for x in row[:11]] == want and row[11] == "%.6f" % (cost[f] / full[f]) and int(row[12]) == over[f]
        assert [int(row[13]), int(row[14])] == [int(((codes[:, 21] & bit) != 0).sum()) for bit in (dref.BAD, dref.LABELLED)]
    assert "%.6f of the full search over %d frames, %d over budget" % (sum(cost) / sum(full), frames, sum(over)) in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]


def test_launcher_under_a_budget_and_without(pkg, tmp_path):
    w, h, frames, qp, seed, gain = 208, 144, 3, 32, 9, 8.0
    rng = np.random.default_rng(5)
    yuv = rng.integers(0, 256, size=(frames, w * h * 3 // 2), dtype=np.uint8)
    yuv[1, :w * h] = (yuv[1, :w * h] // 32 + 90).astype(np.uint8)   # a smoother frame
    yuv.tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text("0.75 0.25 0.75 0.25 0.75 0.25\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET") and k != "ETHCNN_DEVICES"}
    env.update(ETHCNN_SYNTHETIC_SEED=str(seed), ETHCNN_HEAD_GAIN=str(gain))
    run = lambda **more: subprocess.run([sys.executable, LAUNCHER, "seq.yuv", str(w), str(h), str(qp)], cwd=str(tmp_path), env=dict(env, **more),
                                        capture_output=True, text=True, timeout=300)
    r = run(ETHCNN_SEARCH_BUDGET="0.4")
    assert r.returncode == 0 and "search budget 0.4 (frame)" in r.stderr, r.stderr
    baked = np.fromfile(str(tmp_path / "cu_depth.dat"), dtype="<f4").reshape(-1, 21)
    assert baked.shape == (frames * 12, 21) and set(np.unique(baked).tolist()) <= {0.0, 0.5, 1.0}
    r = run(ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_MODE="carry", ETHCNN_SEARCH_BUDGET_WEIGHTS="8 4 2 1")
    assert r.returncode == 0, r.stderr
    carried = np.fromfile(str(tmp_path / "cu_depth.dat"), dtype="<f4").reshape(-1, 21)
    r = run()
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "cu_depth.dat").read_bytes()
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    with pkg.EthCnn(device=0) as own:
        own.load_synthetic(seed, gain)
        own.load_thresholds(str(tmp_path / "Thr_info.txt"))
        own.predict_yuv_file(str(tmp_path / "seq.yuv"), w, h, qp, str(tmp_path / "direct.dat"))
        assert plain == (tmp_path / "direct.dat").read_bytes()        # the variable unset: the code the launcher always ran
        own.set_thresholds(0.0, 0.0)
        own.predict_yuv_file(str(tmp_path / "seq.yuv"), w, h, qp, str(tmp_path / "open.dat"))
        probs = np.fromfile(str(tmp_path / "open.dat"), dtype="<f4")
        with pkg.PartitionSim(own) as s:
            s.add_frames(probs, None, w, h)
            assert baked.tobytes() == s.budget_control(0.4, "frame", width=w, height=h)["probs"].tobytes()
            assert carried.tobytes() == s.budget_control(0.4, "carry", weights=(8, 4, 2, 1), width=w, height=h)["probs"].tobytes()
