"""-m gpu: the online search budget (include/ethcnn.h "search budget, online") on the GPU.  A pacer fed one frame at a time against the
numpy restatement (tests/budget_ref.py: cost -> choose -> bake, Python integers) AND against the offline controller
(PartitionSim.budget_control) on the same frames, field by field and byte by byte; queued back to back; in place and staged; across a
change of geometry; through "the hinge"; and inside both Low-Delay-P daemons.  Inputs are built as in tests/test_gpu_budget.py:
synthetic probabilities on the k / 1024 grid, values exactly at up / down of several rungs, a spread that differs per frame so that the
picked rungs differ.  Integers and three float constants only: every comparison is equality."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import budget_ref as bref
import decide_ref as dref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
COMPANION = ref.thr(*bref.COMPANION)
MODES = {"frame": bref.FRAME, "carry": bref.CARRY}
M = 10 ** 6
# name: width, height, frames, CTU that carries a NaN (None: none)
SHAPES = {"small": (208, 144, 30, 3 * 12 + 5),  # 4 x 3 CTUs, partial right and bottom
          "ragged": (200, 136, 7, None),        # 16 x 16 edge nodes with a single 8 x 8 inside
          "wide": (1088, 1024, 3, None),        # 272 CTUs: five slices, so the ticket counts several blocks
          "nan": (64, 64, 1, 0)}                # one CTU, rejected
_CASES, _LADDERS, _COSTS = {}, {}, {}


def _case(name):
    """(probs [F, per, 21], sim_ref.Set) made once and never changed"""
    if name not in _CASES:
        w, h, frames, nan_at = SHAPES[name]
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
        s = ref.Set()
        s.add_frames(probs, None, w, h, 0)
        probs.setflags(write=False)
        _CASES[name] = (probs, s)
    return _CASES[name]


def _ladder(k):
    if k not in _LADDERS:
        # (2: the full search and the cheapest rung of the default ladder, so that a frame leaves a large remainder)
        _LADDERS[k] = bref.default_ladder() if k == 513 else bref.default_ladder()[[0, 512]].copy() if k == 2 else dref.candidates(np.random.default_rng(k), max(k, 4))[:k].copy()
    return _LADDERS[k]


def _cost(name, k):
    if (name, k) not in _COSTS:
        probs, s = _case(name)
        _COSTS[name, k] = bref.cost(s, _ladder(k), 0, probs.shape[1], probs.shape[0])
    return _COSTS[name, k]


def _expect(checked, ladder, weights, ppm, mode):
    """the choice rule over checked [F, K + 1, 4] -> one dict per frame with every field of ethcnn_pacer_result (Python integers)"""
    rung, over, cost, full = bref.choose(checked, weights, ppm, MODES[mode])
    out, carry = [], 0
    for f in range(len(rung)):
        allow = ppm * full[f] + carry
        carry = allow - cost[f] * M if mode == "carry" and not over[f] else 0
        out.append({"frame": f, "rung": rung[f], "over": over[f], "cost": cost[f], "full": full[f], "carry": carry,
                    "up_k": ladder[rung[f]]["up_k"].tolist(), "down_k": ladder[rung[f]]["down_k"].tolist()})
    return out


def _fields(res):
    return {"frame": int(res["frame"]), "rung": int(res["rung"]), "over": int(res["over"]), "cost": int(res["cost"]), "full": int(res["full"]),
            "carry": int(res["carry_lo"]) | int(res["carry_hi"]) << 64, "up_k": res["up_k"].tolist(), "down_k": res["down_k"].tolist()}


def _offline(pkg, ctx, name, k, weights, share, mode):
    probs, _ = _case(name)
    w, h = SHAPES[name][:2]
    with pkg.PartitionSim(ctx) as sim:
        sim.add_frames(probs, None, w, h)
        return sim.budget_control(share, mode, None if k == 513 else _ladder(k), weights, 0, w, h, probs.shape[0])


def _one_by_one(pkg, ctx, name, k, weights, share, mode):
    """the case through a pacer, frame by frame -> (results, baked [F * per, 21])"""
    probs, _ = _case(name)
    w, h = SHAPES[name][:2]
    got, rows = [], []
    with pkg.Pacer(ctx, share, mode, None if k == 513 else _ladder(k), weights) as pacer:
        for f in range(probs.shape[0]):
            baked, res = pacer.frame(probs[f], w, h)
            got.append(_fields(res))
            rows.append(baked)
    return got, np.concatenate(rows)


def _same_as_both(pkg, ctx, name, k, weights, share, mode):
    probs, s = _case(name)
    frames, per = probs.shape[:2]
    ladder = _ladder(k)
    want = _expect(_cost(name, k), ladder, weights or bref.WEIGHTS, int(round(share * 1e6)), mode)
    got, baked = _one_by_one(pkg, ctx, name, k, weights, share, mode)
    assert got == want, (name, k, share, mode)
    rung = [x["rung"] for x in want]
    assert baked.tobytes() == bref.bake(s, ladder, rung, 0, per, frames).tobytes(), (name, k, share, mode)
    off = _offline(pkg, ctx, name, k, weights, share, mode)
    for key in ("rung", "over", "cost", "full"):
        assert [int(x) for x in off[key]] == [x[key] for x in got], (name, k, share, mode, key)
    assert baked.tobytes() == off["probs"].tobytes()
    return want, baked


@pytest.mark.parametrize("k", [1, 64, 65, 513, 4096])
def test_one_by_one_equals_the_restatement_and_the_offline_controller(pkg, ctx, k):
    seen = {"over": 0, "deep": 0, "carry": 0}
    for mode in ("frame", "carry"):
        for share in (0.4, 0.0):
            want, baked = _same_as_both(pkg, ctx, "small", k, None, share, mode)
            assert set(np.unique(baked).tolist()) <= {0.0, 0.5, 1.0}
            seen["over"] += sum(x["over"] for x in want)
            seen["deep"] += sum(x["rung"] > 0 for x in want)
            seen["carry"] += sum(x["carry"] > 0 for x in want)
            if share == 0.0:
                assert all(x["over"] or x["cost"] == 0 for x in want) and not any(x["carry"] for x in want)
            elif k == 513:
                assert len({x["rung"] for x in want}) > 3   # frames of different spread take different rungs
    assert seen["over"] and (k == 1 or (seen["deep"] and seen["carry"]))


@pytest.mark.parametrize("name", ["ragged", "wide", "nan"])
def test_geometry_corners(pkg, ctx, name):
    for mode in ("frame", "carry"):
        want, baked = _same_as_both(pkg, ctx, name, 513, None, 0.4, mode)
    if name == "nan":
        assert (want[0]["full"], want[0]["rung"], want[0]["over"]) == (0, 0, 0) and (baked == 0.5).all()
    else:
        assert all(x["full"] > 0 for x in want)


def test_frames_queued_back_to_back(pkg, ctx):
    """all frames queued with frame_device and per-frame result slots, one synchronise at the end: table and ticket are zero again for
    every frame and the carry is ordered by the stream"""
    name, k = "small", 513
    probs, s = _case(name)
    w, h, frames = SHAPES[name][:3]
    per = probs.shape[1]
    want = _expect(_cost(name, k), _ladder(k), bref.WEIGHTS, 400000, "carry")
    size = pkg.ethcnn.PACER_RESULT.itemsize
    d_probs, d_baked, d_res = ctx.alloc(probs.nbytes), ctx.alloc(probs.nbytes + 64), ctx.alloc(frames * size + 16)
    try:
        d_probs.upload(probs)
        d_baked.upload(np.full(probs.nbytes + 64, 0xAB, np.uint8))
        d_res.upload(np.full(frames * size + 16, 0xCD, np.uint8))
        with pkg.Pacer(ctx, 0.4, "carry") as pacer:
            for f in range(frames):
                pacer.frame_device(d_probs.ptr + f * per * 84, w, h, d_baked.ptr + 32 + f * per * 84, d_res.ptr + 8 + f * size)
            ctx.synchronize()
            last = pacer.last()
        raw, res = d_baked.download(np.uint8, probs.nbytes + 64), d_res.download(np.uint8, frames * size + 16)
        assert d_probs.download(np.uint8, probs.nbytes).tobytes() == probs.tobytes()
    finally:
        for b in (d_probs, d_baked, d_res):
            b.free()
    assert (raw[:32] == 0xAB).all() and (raw[-32:] == 0xAB).all() and (res[:8] == 0xCD).all() and (res[-8:] == 0xCD).all()
    got = [_fields(r) for r in res[8:-8].view(pkg.ethcnn.PACER_RESULT)]
    assert got == want and _fields(last) == want[-1]
    assert raw[32:-32].tobytes() == bref.bake(s, _ladder(k), [x["rung"] for x in want], 0, per, frames).tobytes()


def test_the_128_bit_path(pkg, ctx):
    weights = (2 ** 32 - 1,) * 4
    want, _ = _same_as_both(pkg, ctx, "wide", 513, weights, 0.4, "carry")
    assert max(x["cost"] for x in want) * M >= 2 ** 64
    want, _ = _same_as_both(pkg, ctx, "wide", 2, weights, 0.9, "carry")      # a coarse ladder: the remainder itself passes 2^64
    assert max(x["carry"] for x in want) >= 2 ** 64 and {x["rung"] for x in want} == {0, 1}


def test_in_place_and_staged_routes_give_the_same_bytes(pkg):
    with pkg.EthCnn(device=0) as own:   # (a context of its own: its page-locked buffer goes with it)
        _routes(pkg, own)


def _routes(pkg, ctx):
    name, k = "ragged", 513
    probs, s = _case(name)
    w, h, frames = SHAPES[name][:3]
    per = probs.shape[1]
    want = _expect(_cost(name, k), _ladder(k), bref.WEIGHTS, 400000, "carry")
    rows = bref.bake(s, _ladder(k), [x["rung"] for x in want], 0, per, frames).reshape(frames, per, 21)
    pinned = ctx.host_buffer(2 * per * 84 + 64).view(np.float32)
    pin_a, pin_b = pinned[4:4 + per * 21].reshape(per, 21), pinned[8 + per * 21:8 + 2 * per * 21].reshape(per, 21)
    dev = ctx.alloc(per * 84)
    routes = {"pageable": [], "pageable in place": [], "pinned in place": [], "pinned to pinned": [], "pinned to pageable": [], "device in place": []}
    try:
        pacers = {r: pkg.Pacer(ctx, 0.4, "carry") for r in routes}
        for f in range(frames):
            src = probs[f].copy()
            baked, res = pacers["pageable"].frame(src, w, h)
            assert src.tobytes() == probs[f].tobytes()                      # not in place: the probabilities stay as they were
            routes["pageable"].append((baked.copy(), _fields(res)))
            baked, res = pacers["pageable in place"].frame(src, w, h, out=src)
            routes["pageable in place"].append((src.copy(), _fields(res)))
            pin_a[:] = probs[f]
            baked, res = pacers["pinned in place"].frame(pin_a, w, h, out=pin_a)
            routes["pinned in place"].append((pin_a.copy(), _fields(res)))
            pin_a[:] = probs[f]
            pinned[:4], pinned[4 + per * 21:8 + per * 21], pinned[8 + 2 * per * 21:] = 7.25, 7.25, 7.25
            baked, res = pacers["pinned to pinned"].frame(pin_a, w, h, out=pin_b)
            assert pin_a.tobytes() == probs[f].tobytes() and (pinned[:4] == 7.25).all() and (pinned[4 + per * 21:8 + per * 21] == 7.25).all()
            assert (pinned[8 + 2 * per * 21:] == 7.25).all()
            routes["pinned to pinned"].append((pin_b.copy(), _fields(res)))
            baked, res = pacers["pinned to pageable"].frame(pin_a, w, h)
            routes["pinned to pageable"].append((baked.copy(), _fields(res)))
            dev.upload(probs[f])
            pacers["device in place"].frame_device(dev, w, h, dev)
            routes["device in place"].append((dev.download(np.float32, per * 21).reshape(per, 21), _fields(pacers["device in place"].last())))
        for r, got in routes.items():
            assert [g[1] for g in got] == want, r
            assert all(g[0].tobytes() == rows[f].tobytes() for f, g in enumerate(got)), r
    finally:
        for p in pacers.values():
            p.close()
        dev.free()


def test_geometry_change_with_carry_then_reset_and_last(pkg, ctx):
    k, weights, nf = 65, (7, 5, 3, 2), 5
    ladder = _ladder(k)
    parts = [("small", nf), ("ragged", nf), ("wide", 2)]
    checked = np.concatenate([_cost(n, k)[:c] for n, c in parts])
    want = _expect(checked, ladder, weights, 550000, "carry")
    assert any(x["carry"] for x in want[nf - 1:nf + 1])    # something is carried across the change of geometry
    with pkg.Pacer(ctx, 0.55, "carry", ladder, weights) as pacer:
        with pytest.raises(pkg.EthCnnError) as err:
            pacer.last()
        assert err.value.code == pkg.ethcnn.ERR_ARG
        got = []
        for name, count in parts:
            probs, s = _case(name)
            w, h = SHAPES[name][:2]
            for f in range(count):
                baked, res = pacer.frame(probs[f], w, h)
                got.append(_fields(res))
                assert _fields(pacer.last()) == got[-1]
                assert baked.tobytes() == bref.bake(s, ladder, [got[-1]["rung"]], f * probs.shape[1], probs.shape[1], 1).tobytes()
        assert got == want
        # after reset the first frames equal a fresh pacer's
        pacer.reset()
        with pytest.raises(pkg.EthCnnError):
            pacer.last()
        probs, _ = _case("ragged")
        fresh = _expect(_cost("ragged", k)[:3], ladder, weights, 550000, "carry")
        assert [_fields(pacer.frame(probs[f], 200, 136)[1]) for f in range(3)] == fresh


def test_bad_arguments_leave_outputs_carry_and_frame_count_untouched(pkg, ctx):
    e = pkg.ethcnn
    name, k = "small", 513
    probs, _ = _case(name)
    w, h = SHAPES[name][:2]
    per = probs.shape[1]
    want = _expect(_cost(name, k), _ladder(k), bref.WEIGHTS, 400000, "carry")
    lib = ctx.lib
    host = np.full(per * 21 + 1, 3.5, np.float32)
    res = np.full(72, 0xEE, np.uint8)
    dev = ctx.alloc(per * 84 + 64)
    dev.upload(np.full(per * 84 + 64, 0xEE, np.uint8))
    src = np.ascontiguousarray(probs[0])
    p = lambda a: a.ctypes.data
    with pytest.raises(ValueError):
        pkg.Pacer(ctx, 1.5)
    with pytest.raises(ValueError):
        pkg.Pacer(ctx, 0.4, "both")
    for bad in (dict(ladder=np.resize(bref.default_ladder(), 4097)), dict(weights=(1, 2, 3, 2 ** 32))):
        with pytest.raises(pkg.EthCnnError) as err:
            pkg.Pacer(ctx, 0.4, "frame", **bad)
        assert err.value.code == e.ERR_ARG
    pacer = pkg.Pacer(ctx, 0.4, "carry")
    try:
        got = [_fields(pacer.frame(probs[f], w, h)[1]) for f in range(2)]
        for ww, hh in ((204, h), (w, 140), (0, h), (w, -8), (65544, h)):
            assert lib.ethcnn_pacer_frame(pacer.h, p(src), ww, hh, p(host), p(res)) == e.ERR_ARG, (ww, hh)
            assert lib.ethcnn_pacer_frame_device(pacer.h, dev.ptr, ww, hh, dev.ptr, dev.ptr + 32) == e.ERR_ARG, (ww, hh)
        assert lib.ethcnn_pacer_frame(pacer.h, None, w, h, p(host), p(res)) == e.ERR_ARG
        assert lib.ethcnn_pacer_frame(pacer.h, p(src), w, h, None, p(res)) == e.ERR_ARG
        assert lib.ethcnn_pacer_frame(pacer.h, p(src), w, h, p(host) + 2, p(res)) == e.ERR_ARG
        assert lib.ethcnn_pacer_frame_device(pacer.h, None, w, h, dev.ptr, None) == e.ERR_ARG
        assert lib.ethcnn_pacer_frame_device(pacer.h, dev.ptr, w, h, None, None) == e.ERR_ARG
        for a, b, c in ((2, 0, 0), (0, 2, 0), (0, 0, 2)):   # not 4-byte aligned
            assert lib.ethcnn_pacer_frame_device(pacer.h, dev.ptr + a, w, h, dev.ptr + b, dev.ptr + 32 + c) == e.ERR_ARG
        assert lib.ethcnn_pacer_last(pacer.h, None) == e.ERR_ARG
        assert (host == 3.5).all() and (res == 0xEE).all() and (dev.download(np.uint8, per * 84 + 64) == 0xEE).all()
        assert _fields(pacer.last()) == got[-1]
        # the next good frames give what they would have given
        got += [_fields(pacer.frame(probs[f], w, h)[1]) for f in range(2, 5)]
        assert got == want[:5]
    finally:
        pacer.close()
        dev.free()
    with pytest.raises(ValueError):
        pacer.frame(probs[0], w, h)        # a closed pacer
    with pytest.raises(ValueError):
        pkg.Pacer(ctx, 0.4).frame(probs[0], 64, 64)   # 12 rows are not a 64 x 64 frame
    # a pacer goes before its context: closing the context closes it
    own = pkg.EthCnn(device=0)
    mine = pkg.Pacer(own, 0.4)
    own.close()
    assert mine.h is None


@pytest.mark.parametrize("mode", ["frame", "carry"])
def test_the_hinge_online(pkg, ctx, mode):
    """ethcnn_decide over a pacer's baked frames under the companion thresholds, gates none, gives each CTU the codes bytes 0..22 it has
    on the original frame under that frame's rung"""
    name = "small"
    w, h, frames, nan_at = SHAPES[name]
    probs, s = _case(name)
    per = probs.shape[1]
    ladder = bref.default_ladder()
    got, baked = _one_by_one(pkg, ctx, name, 513, None, 0.4, mode)
    assert (baked[nan_at] == 0.5).all()
    with pkg.PartitionSim(ctx) as again:
        again.add_frames(baked, None, w, h)
        codes = again.decide(COMPANION, "none")["codes"]
    kept = np.ones(frames * per, bool)
    kept[nan_at] = False
    for f in range(frames):
        sl = slice(f * per, (f + 1) * per)
        want = dref.decide(s, ladder[got[f]["rung"]], first=f * per, n=per)["codes"]
        assert np.array_equal(codes[sl][kept[sl], :23], want[kept[sl], :23]), f
    counts = [pkg.ethcnn.sim_counts_from_codes(codes[f * per:(f + 1) * per][kept[f * per:(f + 1) * per]])["checked"] for f in range(frames)]
    assert [sum(wt * int(x) for wt, x in zip(bref.WEIGHTS, c)) for c in counts] == [x["cost"] for x in got]


# ------------------------------------------------------------------------------------------------------------------ daemons ---
DAEMON_W, DAEMON_H, DAEMON_FRAMES, DAEMON_QP, DAEMON_SEED, DAEMON_GAIN = 416, 240, 5, 32, 21, 8.0
_DAEMON = {}


def _daemon_frames():
    if "resi" not in _DAEMON:
        rng = np.random.default_rng(11)
        resi = np.clip(np.rint(128 + rng.laplace(0.0, 6.0, size=(DAEMON_FRAMES, DAEMON_H, DAEMON_W))), 0, 255).astype(np.uint8)
        resi[2] = 128 + (resi[2].astype(np.int64) - 128) // 4     # a calmer frame
        resi.setflags(write=False)
        _DAEMON["resi"] = resi
    return _DAEMON["resi"]


def _in_process(pkg, thr, budget):
    """what the daemons must write: ldp_step frame by frame (open gates and a pacer under a budget, else the gates of Thr_info.txt)"""
    key = (budget,)
    if key not in _DAEMON:
        resi = _daemon_frames()
        with pkg.EthCnn(device=0) as own:
            own.load_synthetic(DAEMON_SEED, DAEMON_GAIN)
            own.load_lstm_synthetic(DAEMON_SEED, DAEMON_GAIN)
            own.load_thresholds(thr)
            pacer = None
            if budget is not None:
                own.set_thresholds(0.0, 0.0)
                pacer = pkg.Pacer(own, 0.4, budget)
            out = []
            for f in range(DAEMON_FRAMES):
                probs = own.ldp_step(resi[f], DAEMON_W, DAEMON_H, DAEMON_QP, f + 1)
                out.append((pacer.frame(probs, DAEMON_W, DAEMON_H)[0] if pacer else probs).tobytes())
        _DAEMON[key] = out
    return _DAEMON[key]


def _drive(cmd, work, env):
    """the encoder's side of the file handshake, one frame at a time -> the cu_depth.dat of every frame"""
    resi = _daemon_frames()
    p = lambda n: os.path.join(work, n)
    d = subprocess.Popen(cmd, cwd=work, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    out = []
    try:
        for f in range(DAEMON_FRAMES):
            resi[f].tofile(p("resi.yuv"))
            open(p("command.dat"), "w").write("%d %d %d %d [end]" % (f + 1, DAEMON_W, DAEMON_H, DAEMON_QP))
            open(p("pred_start.sig"), "w").close()
            deadline = time.time() + 120
            while not os.path.exists(p("pred_end.sig")):
                assert d.poll() is None and time.time() < deadline, d.stderr.read()[-800:]
                time.sleep(0.002)
            os.remove(p("pred_end.sig"))
            out.append(open(p("cu_depth.dat"), "rb").read())
        assert d.wait(timeout=60) == 0
        return out, d.stderr.read()
    finally:
        if d.poll() is None:
            d.kill()


@pytest.mark.parametrize("budget", ["frame", "carry", None])
def test_daemons_pace_every_frame_inside_the_handshake(pkg, tmp_path, budget):
    thr = str(tmp_path / "Thr_info.txt")
    pkg.ethcnn.sim_write_thr_info(thr, pkg.ethcnn.budget_companion_thr(), "ldp")
    want = _in_process(pkg, thr, budget)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    env.update(ETHCNN_SYNTHETIC_SEED=str(DAEMON_SEED), ETHCNN_HEAD_GAIN=str(DAEMON_GAIN))
    if budget is not None:
        env.update(ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_MODE=budget)
    for which, cmd in (("native", [os.path.join(BIN, "resi_to_cu_depth_ldp"), "--quiet"]),
                       ("python", [sys.executable, os.path.join(ROOT, "resi_to_cu_depth_LDP.py"), "--python"])):
        work = str(tmp_path / which)
        os.makedirs(work)
        open(os.path.join(work, "Thr_info.txt"), "w").write(open(thr).read())
        got, stderr = _drive(cmd + ["--max-frames", str(DAEMON_FRAMES), "--idle-timeout", "60"], work, env)
        assert got == want, (which, budget)
        assert ("search budget 0.4 (%s)" % budget in stderr and "over %d frames" % DAEMON_FRAMES in stderr) if budget else "search budget" not in stderr
    if budget is not None:
        baked = np.frombuffer(b"".join(want), "<f4")
        assert set(np.unique(baked).tolist()) <= {0.0, 0.5, 1.0} and want != _in_process(pkg, thr, None)
