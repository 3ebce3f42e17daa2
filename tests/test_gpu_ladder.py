"""-m gpu: the ladder search (include/ethcnn.h "search budget: building a ladder") on the GPU.  Every path k_ladder_step builds is compared
field for field with the restatement (tests/ladder_ref.py: Python integers on top of sim_ref.Set.evaluate), every rung's counters with
the simulator's own evaluation as a second witness, and a built ladder goes through "the hinge": the offline controller, the pacer, the
tools and the launchers hold a budget with it.  Probabilities are a noisy teacher of the labels, quantised to 1 / 128 so that ties
happen.  Integers only: every comparison is equality.  The shapes are the smallest at which slices, partial candidate waves, ties and
the cap all occur; the restatement evaluates only the grid's candidates per step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_ref as bref
import ladder_ref as lref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
BUILD_TOOL = os.path.join(ROOT, "tools", "build_ladder.py")
CONTROL_TOOL = os.path.join(ROOT, "tools", "control_budget.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
W, H, FRAMES, PER = 208, 144, 30, 12      # 4 x 3 CTUs, partial right and bottom: 6 of a frame's 12 CTUs are whole, so 180 of 360 carry labels
_CASES, _PATHS, _STATS = {}, {}, {}


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _teacher(rng, truth, labelled):
    """probabilities that lean towards the label, with noise; CTUs without labels get uniform ones; all on the grid k / 128"""
    p = np.where(truth, 0.72, 0.28) + rng.normal(0.0, 0.22, size=truth.shape)
    p = np.where(labelled[:, None], p, rng.uniform(0.0, 1.0, size=truth.shape))
    return (np.clip(np.rint(p * 128), 0, 128) / 128.0).astype(np.float32)


def _case(name):
    """made once and never changed.  frames / more: (probs [F, 12, 21], labels, Set); small / perctu: (probs, depth16, unlabelled probs, Set)"""
    if name not in _CASES:
        if name in ("frames", "more"):
            frames = FRAMES if name == "frames" else 4
            rng = np.random.default_rng(3 if name == "frames" else 4)
            labels = rng.integers(0, 4, size=(frames, H // 16, W // 16)).astype(np.uint8)
            t = ref.Set()
            t.add_frames(np.zeros((frames, PER, 21), np.float32), labels, W, H)
            probs = _teacher(rng, t.truth, t.labelled).reshape(frames, PER, 21)
            s = ref.Set()
            s.add_frames(probs, labels, W, H)
            _CASES[name] = (probs, labels, s)
        else:
            n, n_plain, nan_at, seed = {"small": (60, 0, None, 5), "perctu": (1300, 1300, 77, 6)}[name]
            rng = np.random.default_rng(seed)
            depth = rng.integers(0, 4, size=(n, 16)).astype(np.uint8)
            t = ref.Set()
            t.add(np.zeros((n, 21), np.float32), depth)
            probs = _teacher(rng, t.truth, t.labelled)
            if nan_at is not None:
                probs[nan_at, 9] = np.nan
            plain = (rng.integers(0, 129, size=(n_plain, 21)) / 128.0).astype(np.float32)
            s = ref.Set()
            s.add(probs, depth)
            if n_plain:
                s.add(plain)
            _CASES[name] = (probs, depth, plain, s)
        for a in _CASES[name][:2]:
            a.setflags(write=False)
    return _CASES[name]


def _fill(sim, name):
    c = _case(name)
    if name in ("frames", "more"):
        sim.add_frames(c[0], c[1], W, H)
    else:
        sim.add(c[0], c[1])
        if c[2].shape[0]:
            sim.add(c[2])
    return c[-1]


def _want(name, weights=None, grid=8, max_rungs=4096, max_bad_ppm=10 ** 6):
    key = (name, weights, grid, max_rungs, max_bad_ppm)
    if key not in _PATHS:
        _STATS[key] = {}
        _PATHS[key] = lref.build(_case(name)[-1], weights, grid, max_rungs, max_bad_ppm, _STATS[key])
    return _PATHS[key]


def _same(got, want):
    """field for field"""
    assert len(got["cost"]) == len(want)
    for name, field in (("up_k", got["thr"]["up_k"]), ("down_k", got["thr"]["down_k"]), ("checked", got["checked"])):
        assert field.tolist() == [r[name] for r in want], name
    for name in ("coord", "value", "bad_ctus", "cost"):
        assert [int(x) for x in got[name]] == [r[name] for r in want], name
    assert got["thr"].dtype.names == ("up_k", "down_k") and got["coord"].dtype == np.int32 and got["checked"].dtype == np.uint64


def _witness(sim, got):
    """the simulator's own evaluation of every rung's thresholds gives the rung's counters"""
    counts = sim.eval(got["thr"], "none")
    assert np.array_equal(counts["checked"], got["checked"]) and np.array_equal(counts["bad_ctus"], got["bad_ctus"])


def _promises(got, grid):
    cost = [int(x) for x in got["cost"]]
    assert all(b < a for a, b in zip(cost, cost[1:]))                         # costs fall strictly
    assert got["thr"][0]["up_k"].tolist() == [1024] * 3 and got["thr"][0]["down_k"].tolist() == [-1] * 3 and (got["coord"][0], got["value"][0]) == (-1, 0)
    assert (got["thr"]["down_k"] <= got["thr"]["up_k"]).all()
    assert (got["value"][1:] % grid == 0).all() and ((got["coord"][1:] >= 0) & (got["coord"][1:] < 6)).all()
    flat = np.stack([got["thr"]["down_k"], got["thr"]["up_k"]], axis=2).reshape(len(cost), 6)   # sweep order: down0 up0 down1 up1 down2 up2
    for i in range(1, len(cost)):                                             # one coordinate moves per rung, to `value`
        moved = np.nonzero(flat[i] != flat[i - 1])[0].tolist()
        assert moved == [int(got["coord"][i])] and flat[i, moved[0]] == got["value"][i]


def test_the_full_path_on_frames_with_edge_ctus(sim):
    s = _fill(sim, "frames")
    assert sim.info()["labelled_ctus"] == 180 == int(s.labelled.sum()) and sim.info()["ctus"] == 360
    want = _want("frames", None, 64)
    got = sim.build_ladder(grid=64)
    _same(got, want)
    _witness(sim, got)
    _promises(got, 64)
    assert len(want) > 30 and len({r["coord"] for r in want[1:]}) >= 4         # a long path on which ups and downs of several levels move
    assert any(b["bad_ctus"] < a["bad_ctus"] for a, b in zip(want, want[1:]))  # a negative numerator in the choice
    assert _STATS["frames", None, 64, 4096, 10 ** 6]["ties"] > 0               # steps at which two moves share the smallest ratio


def test_the_fine_grid_has_partial_candidate_waves(sim):
    _fill(sim, "small")
    got = sim.build_ladder(grid=1, max_rungs=7)     # 1025 values a coordinate: 17 candidate waves each, the last one partial
    _same(got, _want("small", None, 1, 7))
    _witness(sim, got)
    _promises(got, 1)
    assert len(got["cost"]) == 7


def test_the_per_ctu_layout_with_unlabelled_and_rejected_ctus(sim):
    s = _fill(sim, "perctu")
    info = sim.info()
    assert (info["ctus"], info["labelled_ctus"], info["rejected_ctus"]) == (2600, 1299, 1) == (s.ctus, int(s.labelled.sum()), s.rejected)
    got = sim.build_ladder(grid=128)
    _same(got, _want("perctu", None, 128))
    _witness(sim, got)
    _promises(got, 128)


def test_the_cap_on_bad_ctus_ends_the_path(sim):
    _fill(sim, "frames")
    free, capped = _want("frames", None, 64), _want("frames", None, 64, 4096, 20000)
    got = sim.build_ladder(grid=64, max_bad_ppm=20000)
    _same(got, capped)
    _witness(sim, got)
    assert 1 < len(capped) < len(free)                                         # the path ends early ...
    assert _STATS["frames", None, 64, 4096, 20000]["capped"] > 0               # ... because the cap took moves away
    assert all(int(b) * 10 ** 6 <= 20000 * 180 for b in got["bad_ctus"][1:])     # ... and every move stayed within the cap
    got = sim.build_ladder(grid=64, max_bad_ppm=0)   # the full search has no bad CTU: rung 0 is always there
    _same(got, _want("frames", None, 64, 4096, 0))
    assert len(got["cost"]) >= 1 and not got["bad_ctus"].any()


@pytest.mark.parametrize("weights", [(1, 0, 0, 0), (2 ** 32 - 1,) * 4])
def test_weights(sim, weights):
    _fill(sim, "frames")
    want = _want("frames", weights, 64)
    got = sim.build_ladder(weights, grid=64)
    _same(got, want)
    _promises(got, 64)
    if weights[0] > 1:
        assert want[0]["cost"] > 2 ** 44 and len(want) > 30   # numerators and savings whose cross products need more than 64 bits
    else:
        assert all(r["coord"] in (0, 1) for r in want[1:])   # only level 0 changes the number of 64 x 64 checks


@pytest.mark.parametrize("max_rungs", [1, 64, 65])
def test_batch_boundaries(sim, max_rungs):
    _fill(sim, "small")
    want = _want("small", None, 8, max_rungs)
    assert len(want) == max_rungs                     # (the whole path has more than 65 rungs)
    got = sim.build_ladder(grid=8, max_rungs=max_rungs)
    _same(got, want)
    _witness(sim, got)


def test_the_state_is_clean_between_builds_and_follows_the_set(sim):
    _fill(sim, "frames")
    first = sim.build_ladder(grid=64)
    other = sim.build_ladder(grid=8, max_rungs=10)    # another table shape in between
    again = sim.build_ladder(grid=64)
    for k in ("thr", "coord", "value", "checked", "bad_ctus"):
        assert first[k].tobytes() == again[k].tobytes(), k
    assert len(other["cost"]) == 10
    more = _case("more")
    sim.add_frames(more[0], more[1], W, H)
    both = ref.Set()
    both.add_frames(_case("frames")[0], _case("frames")[1], W, H)
    both.add_frames(more[0], more[1], W, H)
    got = sim.build_ladder(grid=64)
    _same(got, lref.build(both, None, 64))
    assert got["thr"].tobytes() != first["thr"].tobytes()


def test_refusals_leave_the_outputs_untouched(pkg, sim):
    e = pkg.ethcnn
    import ctypes
    lib = sim.lib
    rungs, n = np.full(4, 7, e.LADDER_RUNG), ctypes.c_int64(-5)
    call = lambda w, grid, max_rungs, ppm: lib.ethcnn_ladder_build(sim.h, w, grid, max_rungs, ppm, rungs.ctypes.data, ctypes.byref(n))
    w = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
    assert call(w, 64, 4, 5) == e.ERR_ARG and "labelled" in sim.ctx.lib.ethcnn_last_error(sim.ctx.h).decode()    # an empty set
    sim.add(_case("perctu")[2])                                                                                   # CTUs, but no labels
    assert call(w, 64, 4, 5) == e.ERR_ARG
    _fill(sim, "small")
    wbig = (ctypes.c_uint64 * 4)(64, 16, 4, 2 ** 32)
    for args in ((w, 3, 4, 5), (w, 0, 4, 5), (w, 2048, 4, 5), (w, 64, 0, 5), (w, 64, 4097, 5), (w, 64, 4, 10 ** 6 + 1), (wbig, 64, 4, 5)):
        assert call(*args) == e.ERR_ARG, args[1:]
    assert lib.ethcnn_ladder_build(sim.h, w, 64, 4, 5, None, ctypes.byref(n)) == e.ERR_ARG and lib.ethcnn_ladder_build(sim.h, w, 64, 4, 5, rungs.ctypes.data, None) == e.ERR_ARG
    assert n.value == -5 and (rungs["coord"] == 7).all() and (rungs["bad_ctus"] == 7).all()
    assert call(None, 64, 4, 10 ** 6) == 0 and 1 <= n.value <= 4 and (rungs["coord"][n.value:] == 7).all()        # NULL weight: 64 16 4 1
    for bad in (dict(grid=3), dict(max_rungs=0), dict(max_rungs=4097), dict(max_bad_ppm=10 ** 6 + 1), dict(weights=(1, 2, 3, 2 ** 32))):
        with pytest.raises(pkg.EthCnnError) as err:
            sim.build_ladder(**bad)
        assert err.value.code == e.ERR_ARG


@pytest.mark.parametrize("mode", ["frame", "carry"])
def test_the_hinge_a_built_ladder_holds_a_budget_offline_and_online(pkg, ctx, sim, mode):
    s = _fill(sim, "frames")
    got = sim.build_ladder(grid=64)
    ladder, frames = got["thr"], 8
    assert np.array_equal(ladder, ref.thr([r["up_k"] for r in _want("frames", None, 64)], [r["down_k"] for r in _want("frames", None, 64)]))
    rung, over, cost, full = bref.choose(bref.cost(s, ladder, 0, PER, frames), bref.WEIGHTS, 450000, {"frame": bref.FRAME, "carry": bref.CARRY}[mode])
    baked = bref.bake(s, ladder, rung, 0, PER, frames)
    off = sim.budget_control(0.45, mode, ladder, width=W, height=H, nframes=frames)
    assert off["rung"].tolist() == rung and off["over"].astype(int).tolist() == over and [int(x) for x in off["cost"]] == cost
    assert off["probs"].tobytes() == baked.tobytes()
    assert len(set(rung)) > 1 and max(rung) > 0                                    # the frames take different rungs of the built ladder
    probs = _case("frames")[0]
    with pkg.Pacer(ctx, 0.45, mode, ladder) as pacer:
        for f in range(frames):
            rows, res = pacer.frame(probs[f], W, H)
            assert (int(res["rung"]), int(res["over"]), int(res["cost"]), int(res["full"])) == (rung[f], over[f], cost[f], full[f]), f
            assert rows.tobytes() == baked[f * PER:(f + 1) * PER].tobytes()


def _write_case(tmp_path, frames):
    probs, labels, _ = _case("frames")
    pp, lp = str(tmp_path / "cu_depth_in.dat"), str(tmp_path / "Info_CUDepth.dat")
    probs[:frames].tofile(pp)
    labels[:frames].tofile(lp)
    s = ref.Set()
    s.add_frames(probs[:frames], labels[:frames], W, H)
    return pp, lp, s


def test_tools_end_to_end_a_built_file_drives_the_controller(pkg, tmp_path):
    frames = 6
    pp, lp, s = _write_case(tmp_path, frames)
    case = ["--case", lp, pp, str(W), str(H)]
    r = subprocess.run([sys.executable, BUILD_TOOL, "--grid", "64", "--rungs", "9", "--weights", "60", "20", "5", "1", "--out", "ladder.txt", "--order", "ldp",
                        "--csv", "ladder.csv"] + case, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    weights = (60, 20, 5, 1)
    path = lref.build(s, weights, 64)
    keep = lref.thin([x["cost"] for x in path], 9)
    up, down = [path[i]["up_k"] for i in keep], [path[i]["down_k"] for i in keep]
    assert len(path) > 9 and open(str(tmp_path / "ladder.txt")).read() == lref.ladder_lines(up, down, "ldp")
    rows = [line.split(",") for line in open(str(tmp_path / "ladder.csv")).read().strip().splitlines()]
    assert rows[0] == "up0,up1,up2,down0,down1,down2,cost,share,bad_ppm,moved".split(",") and len(rows) == 1 + len(keep)
    labelled = int(s.labelled.sum())
    for row, i in zip(rows[1:], keep):
        x = path[i]
        assert [int(v) for v in row[:7]] == x["up_k"] + x["down_k"] + [x["cost"]] and row[7] == "%.6f" % (x["cost"] / path[0]["cost"])
        assert row[8] == "%.1f" % (x["bad_ctus"] * 10 ** 6 / labelled) and row[9] == ("-" if x["coord"] < 0 else ref.COORDS[x["coord"]])
    assert "%d rungs built" % len(path) in r.stderr and "%d kept" % len(keep) in r.stderr
    # the controller reads that file and holds a budget with it
    r = subprocess.run([sys.executable, CONTROL_TOOL, "--budget", "0.5", "--mode", "carry", "--ladder", "ladder.txt", "--order", "ldp", "--out", "cu_depth.dat"]
                       + case, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ladder = ref.thr(up, down)
    rung, over, cost, full = bref.choose(bref.cost(s, ladder, 0, PER, frames), bref.WEIGHTS, 500000, bref.CARRY)
    assert open(str(tmp_path / "cu_depth.dat"), "rb").read() == bref.bake(s, ladder, rung, 0, PER, frames).tobytes()
    assert "%.6f of the full search over %d frames, %d over budget" % (sum(cost) / sum(full), frames, sum(over)) in r.stderr and max(rung) > 0
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    # without labels the tool stops before a GPU is touched
    r = subprocess.run([sys.executable, BUILD_TOOL, "--case", "-", pp, str(W), str(H)], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "labels" in r.stderr


def test_launcher_under_a_ladder_file(pkg, sim, tmp_path):
    w, h, frames, qp, seed, gain = 208, 144, 3, 32, 9, 8.0
    _fill(sim, "frames")
    ladder = sim.build_ladder(grid=64)["thr"]
    pkg.ethcnn.ladder_write(str(tmp_path / "ladder.txt"), ladder, "ai")
    rng = np.random.default_rng(5)
    yuv = rng.integers(0, 256, size=(frames, w * h * 3 // 2), dtype=np.uint8)
    yuv[1, :w * h] = (yuv[1, :w * h] // 32 + 90).astype(np.uint8)   # a smoother frame
    yuv.tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text("0.75 0.25 0.75 0.25 0.75 0.25\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET") and k != "ETHCNN_DEVICES"}
    env.update(ETHCNN_SYNTHETIC_SEED=str(seed), ETHCNN_HEAD_GAIN=str(gain), ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="ladder.txt")
    r = subprocess.run([sys.executable, LAUNCHER, "seq.yuv", str(w), str(h), str(qp)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "search budget 0.4 (frame)" in r.stderr, r.stderr
    baked = (tmp_path / "cu_depth.dat").read_bytes()
    with pkg.EthCnn(device=0) as own:
        own.load_synthetic(seed, gain)
        own.set_thresholds(0.0, 0.0)
        own.predict_yuv_file(str(tmp_path / "seq.yuv"), w, h, qp, str(tmp_path / "open.dat"))
        probs = np.fromfile(str(tmp_path / "open.dat"), dtype="<f4")
        with pkg.PartitionSim(own) as s:
            s.add_frames(probs, None, w, h)
            assert baked == s.budget_control(0.4, "frame", ladder, width=w, height=h)["probs"].tobytes()


def test_both_daemons_under_a_ladder_file_stay_byte_identical(pkg, sim, tmp_path):
    import test_gpu_pacer as tp   # the encoder's side of the handshake and the frames are those of the pacer's daemon test
    _fill(sim, "frames")
    ladder = sim.build_ladder(grid=64)["thr"]
    thr = str(tmp_path / "Thr_info.txt")
    pkg.ethcnn.sim_write_thr_info(thr, pkg.ethcnn.budget_companion_thr(), "ldp")
    pkg.ethcnn.ladder_write(str(tmp_path / "ladder.txt"), ladder, "ldp")
    resi = tp._daemon_frames()
    with pkg.EthCnn(device=0) as own:
        own.load_synthetic(tp.DAEMON_SEED, tp.DAEMON_GAIN)
        own.load_lstm_synthetic(tp.DAEMON_SEED, tp.DAEMON_GAIN)
        own.set_thresholds(0.0, 0.0)
        with pkg.Pacer(own, 0.4, "carry", ladder) as pacer:
            want = [pacer.frame(own.ldp_step(resi[f], tp.DAEMON_W, tp.DAEMON_H, tp.DAEMON_QP, f + 1), tp.DAEMON_W, tp.DAEMON_H)[0].tobytes()
                    for f in range(tp.DAEMON_FRAMES)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    env.update(ETHCNN_SYNTHETIC_SEED=str(tp.DAEMON_SEED), ETHCNN_HEAD_GAIN=str(tp.DAEMON_GAIN), ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_MODE="carry",
               ETHCNN_SEARCH_BUDGET_LADDER=str(tmp_path / "ladder.txt"))
    outs = {}
    for which, cmd in (("native", [os.path.join(BIN, "resi_to_cu_depth_ldp"), "--quiet"]),
                       ("python", [sys.executable, os.path.join(ROOT, "resi_to_cu_depth_LDP.py"), "--python"])):
        work = str(tmp_path / which)
        os.makedirs(work)
        open(os.path.join(work, "Thr_info.txt"), "w").write(open(thr).read())
        outs[which], stderr = tp._drive(cmd + ["--max-frames", str(tp.DAEMON_FRAMES), "--idle-timeout", "60"], work, env)
        assert outs[which] == want, which
        assert "search budget 0.4 (carry)" in stderr
    assert outs["native"] == outs["python"]
