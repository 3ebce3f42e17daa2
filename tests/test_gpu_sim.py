"""-m gpu: the partition-search simulator (include/ethcnn.h "partition-search simulation") on the GPU against its numpy restatement
(tests/sim_ref.py): both layouts, host and device entries, with and without labels, partial CTUs, the three gate orders, accumulation /
reset / the error paths, sweep and search, and the command-line tool end to end.  Counters are integers: every comparison is
array_equal.  Against vacuous passes every comparison first asserts that the reference fills every counter that the set can fill (a
set without partial CTUs has no edge_split, one without labels no wrong_* / bad_ctus) for at least one candidate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "simulate_thresholds.py")
GATES = {"none": ref.GATES_NONE, "ai": ref.GATES_AI, "ldp": ref.GATES_LDP}

_CASES = {}


def _candidates():
    """1026 candidates; the first is the one that fills every counter, then the corners: full search, up = down, crossed, down = -1,
    up = 0, up = 1024; the rest random, a third of them crossed somewhere"""
    if "cands" not in _CASES:
        rng = np.random.default_rng(77)
        up, down = rng.integers(0, 1025, size=(1026, 3)), rng.integers(-1, 1025, size=(1026, 3))
        keep = rng.integers(0, 3, size=1026) > 0
        lo, hi = np.minimum(up, down), np.maximum(up, down)
        up, down = np.where(keep[:, None], hi, up), np.where(keep[:, None], lo, down)
        up[:8] = [(600, 700, 800), (1024, 1024, 1024), (512, 512, 512), (300, 400, 500), (600, 700, 800), (0, 0, 0), (1024, 1024, 1024), (0, 1024, 0)]
        down[:8] = [(400, 300, 200), (-1, -1, -1), (512, 512, 512), (700, 800, 900), (-1, -1, -1), (0, 0, 0), (1024, 1024, 1024), (-1, 1024, 1024)]
        up[up < 0] = 0
        c = ref.thr(up, down)
        c.setflags(write=False)
        _CASES["cands"] = c
    return _CASES["cands"]


def _per_ctu_case(n):
    """(probs, depth, reference counters with labels, without) of n CTUs over all 1026 candidates, made once; with n > 1 the last CTU
    carries a NaN, a -0.5 and a 1.5 and is rejected"""
    if n not in _CASES:
        rng = np.random.default_rng(200 + n)
        probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
        if n > 1:
            probs[-1, 0], probs[-1, 3], probs[-1, 20] = np.nan, -0.5, 1.5
        sets = ref.Set(), ref.Set()
        sets[0].add(probs, depth)
        sets[1].add(probs)
        want = [s.evaluate(_candidates()) for s in sets]
        assert sets[0].info()["rejected_ctus"] == (1 if n > 1 else 0)
        for a in (probs, depth) + tuple(want):
            a.setflags(write=False)
        _CASES[n] = (probs, depth, want[0], want[1], sets[0].info(), sets[1].info())
    return _CASES[n]


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _not_vacuous(want, n, **kw):
    if n >= 63:
        assert ref.fills_every_field(want, **kw)
    else:
        assert all(want[f].any() for f in ("checked", "split_only", "current_only", "both"))


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 1026])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_per_ctu_layout_host_and_device(ctx, sim, n, k):
    probs, depth, want_l, want_u, info_l, info_u = _per_ctu_case(n)
    cands = _candidates()[:k]
    _not_vacuous(want_l[:max(k, 8)], n, edges=0)
    _not_vacuous(want_u[:max(k, 8)], n, edges=0, labels=False)
    sim.add(probs, depth)
    assert sim.info() == info_l and ref.equal(sim.eval(cands), want_l[:k])
    sim.reset()
    sim.add(probs)
    assert sim.info() == info_u and ref.equal(sim.eval(cands), want_u[:k])
    sim.reset()
    dp, dd = ctx.alloc(probs.nbytes), ctx.alloc(depth.nbytes)
    try:
        dp.upload(probs)
        dd.upload(depth)
        sim.add_device(dp, dd, n)
        got_l = sim.eval(cands, "ldp")  # per-CTU layout: never gated
        sim.reset()
        sim.add_device(dp, None, n)
        got_u = sim.eval(cands, "ai")
    finally:
        dp.free()
        dd.free()
    assert ref.equal(got_l, want_l[:k]) and ref.equal(got_u, want_u[:k])
    if n > 1:
        assert sim.info()["rejected_ctus"] == 1


def _frame_case(rng, w, h, frames, skip, labelled):
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    probs = calib_ref.edge_probs(rng, frames * nctu).reshape(frames, nctu, 21)
    labels = None
    if labelled:
        labels = rng.integers(0, 4, size=(frames + skip, h // 16, w // 16)).astype(np.uint8)
        labels[skip:, :4, :4] = np.array([3, 0, 2])[:frames, None, None] if frames == 3 else 3
    return probs, labels


@pytest.mark.parametrize("w,h,frames,skip,labelled", [(64, 64, 3, 0, True), (208, 144, 3, 1, True), (200, 136, 2, 0, False)])
def test_frame_layout(ctx, sim, w, h, frames, skip, labelled):
    rng = np.random.default_rng(w)
    probs, labels = _frame_case(rng, w, h, frames, skip, labelled)
    cands = _candidates()[:130]
    s = ref.Set()
    s.add_frames(probs, labels, w, h, skip)
    want = {g: s.evaluate(cands, GATES[g]) for g in GATES}
    if w == 64:
        assert all(want["none"][f].any() for f in ref.FIELDS if f != "edge_split")
    else:
        assert ref.fills_every_field(want["none"], edges=3 if w % 16 else 2, labels=labelled)
        assert s.info()["whole_ctus"] == frames * (w // 64) * (h // 64) < s.info()["ctus"]
    sim.add_frames(probs, labels, w, h, skip_label_frames=skip)
    assert sim.info() == s.info()
    for g in GATES:
        assert ref.equal(sim.eval(cands, g), want[g]), g
    sim.reset()
    dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes if labelled else 16)
    try:
        dp.upload(probs)
        if labelled:
            dl.upload(labels)
        sim.add_frames_device(dp, dl if labelled else None, w, h, frames, skip_label_frames=skip)
        assert sim.info() == s.info()
        for g in GATES:
            assert ref.equal(sim.eval(cands, g), want[g]), g
    finally:
        dp.free()
        dl.free()


def test_gates_over_two_sub_batches_a_frame(sim):
    rng = np.random.default_rng(11)
    w, h, frames = 2560, 1920, 2  # 1200 CTUs a frame: sub-batches of 1024 and 176
    probs = calib_ref.edge_probs(rng, frames * 1200).reshape(frames, 1200, 21)
    # the second sub-batch's p64 / p32 are capped: its gate 1 / gate 2 close for some candidates and not for others
    probs[:, 1024:, 0] = np.minimum(probs[:, 1024:, 0], np.float32(500 / 1024.0))
    probs[:, 1024:, 1:5] = np.minimum(probs[:, 1024:, 1:5], np.float32(600 / 1024.0))
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16)).astype(np.uint8)
    # down_k <= up_k everywhere (the condition under which the AI-order gates change nothing); candidates 1 and 2: down_k[1] = -1
    cands = ref.thr([(600, 700, 800), (400, 700, 800), (400, 500, 800), (450, 650, 800), (1024, 1024, 1024), (500, 600, 700), (499, 599, 700)],
                    [(400, 300, 200), (300, -1, 200), (300, -1, 200), (400, 300, 200), (-1, -1, -1), (500, 600, 700), (100, 599, 3)])
    s = ref.Set()
    s.add_frames(probs, labels, w, h)
    want = {g: s.evaluate(cands, GATES[g]) for g in GATES}
    assert s.info()["sub_batches"] == 4 and ref.fills_every_field(want["none"], edges=0)
    assert ref.equal(want["ai"], want["none"])
    assert [not ref.equal(want["ldp"][i], want["none"][i]) for i in range(cands.size)] == [True, True, False, True, False, False, False]
    sim.add_frames(probs, labels, w, h)
    assert sim.info() == s.info()
    got = {g: sim.eval(cands, g) for g in GATES}
    for g in GATES:
        assert ref.equal(got[g], want[g]), g
    assert ref.equal(got["ai"], got["none"]) and not ref.equal(got["ldp"], got["none"])


def test_accumulation_reset_and_errors(pkg, sim):
    probs, depth, want, _, info, _ = _per_ctu_case(1000)
    cands = _candidates()[:65]
    assert ref.fills_every_field(want[:65], edges=0)
    assert not sim.eval(cands).view(np.uint64).any() and sim.info()["ctus"] == 0  # an empty set: zeroed output
    assert sim.eval(cands[:0]).size == 0
    for a, b in ((0, 1), (1, 300), (300, 1000)):
        sim.add(probs[a:b], depth[a:b])
    sim.add(probs[:0], depth[:0])  # n == 0: a no-op
    assert sim.info() == info and ref.equal(sim.eval(cands), want[:65])
    # a bad depth byte fails and adds nothing; later calls still work
    bad = depth.copy()
    bad[200, 7] = 4
    with pytest.raises(pkg.EthCnnError) as e:
        sim.add(probs, bad)
    assert e.value.code == pkg.ethcnn.ERR_FORMAT and "above 3" in str(e.value)
    assert sim.info() == info and ref.equal(sim.eval(cands), want[:65])
    # mixed layouts: the per-CTU set and two frame sets, against the restatement fed the same way
    rng = np.random.default_rng(4)
    fp, fl = _frame_case(rng, 208, 144, 3, 1, True)
    gp, _ = _frame_case(rng, 200, 136, 2, 0, False)
    s = ref.Set()
    s.add(probs, depth)
    s.add_frames(fp, fl, 208, 144, 1)
    s.add_frames(gp, None, 200, 136)
    mixed = {g: s.evaluate(cands, GATES[g]) for g in GATES}
    assert ref.fills_every_field(mixed["none"])  # (the 200 x 136 set has 16 x 16 CUs that cross the edge)
    sim.add_frames(fp, fl, 208, 144, skip_label_frames=1)
    sim.add_frames(gp, None, 200, 136)
    assert sim.info() == s.info() and s.info()["sub_batches"] == 5
    for g in GATES:
        assert ref.equal(sim.eval(cands, g), mixed[g]), g
    badl = fl.copy()
    badl[1, 2, 2] = 200
    with pytest.raises(pkg.EthCnnError) as e:
        sim.add_frames(fp, badl, 208, 144, skip_label_frames=1)
    assert e.value.code == pkg.ethcnn.ERR_FORMAT and sim.info() == s.info()
    for args in ((fp, fl, 200, 136), (gp, None, 196, 136)):  # labels need multiples of 16, pictures multiples of 8
        with pytest.raises(pkg.EthCnnError) as e:
            sim.add_frames(*args, nframes=1)
        assert e.value.code == pkg.ethcnn.ERR_ARG
    for up, down in (((0, 0, 1025), (0, 0, 0)), ((0, 0, 0), (-2, 0, 0)), ((-1, 0, 0), (0, 0, 0))):
        with pytest.raises(pkg.EthCnnError) as e:
            sim.eval(ref.thr(up, down))
        assert e.value.code == pkg.ethcnn.ERR_ARG
    assert ref.equal(sim.eval(cands, "ldp"), mixed["ldp"])
    sim.reset()
    assert sim.info() == {"ctus": 0, "whole_ctus": 0, "labelled_ctus": 0, "rejected_ctus": 0, "sub_batches": 0}
    sim.add(probs, depth)  # the same set again gives the same counters
    assert ref.equal(sim.eval(cands), want[:65])


def _leaning_case(n, seed):
    """probabilities that lean towards the truth, so that pruning is possible at all"""
    rng = np.random.default_rng(seed)
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    t, d = np.zeros((n, 21), bool), depth.astype(np.int64)
    t[:, 0], t[:, 1:5], t[:, 5:] = d.sum(axis=1) > 8, d[:, calib_ref.IDX32].sum(axis=2) > 6, d == 3
    return np.where(t, np.float32(0.5) + probs / 2, probs / 2).astype(np.float32), depth


def test_sweep_and_search(pkg, sim):
    probs, depth = _per_ctu_case(65)[:2]
    s = ref.Set()
    s.add(probs, depth)
    sim.add(probs, depth)
    base = ref.thr((600, 700, 800), (400, 300, 200))
    for coord in range(6):
        values, cands = s.sweep_candidates(base, coord)
        got_values, got = sim.sweep(base, ref.COORDS[coord])
        assert values.size == (1025 if coord & 1 else 1026) and np.array_equal(got_values, values)
        want = s.evaluate(cands)
        assert ref.fills_every_field(want, edges=0)
        assert ref.equal(got, want) and ref.equal(got, sim.eval(cands))
    n, weights = 64, (64, 16, 4, 1)
    probs, depth = _leaning_case(n, 8)
    s.reset()
    s.add(probs, depth)
    sim.reset()
    sim.add(probs, depth)
    full = ref.thr(*ref.FULL)
    for ppm, rounds in ((100000, 8), (300000, 1), (0, 0)):
        want_thr, want_counts, want_rounds = s.search(full, ref.GATES_NONE, weights, ppm, rounds)
        thr, counts, ran = sim.search(full, "none", weights, ppm, rounds)
        assert thr == want_thr and ref.equal(counts, want_counts) and ran == want_rounds, (ppm, rounds, thr, want_thr)
        assert int(counts["bad_ctus"]) * 10 ** 6 <= ppm * n
    assert want_rounds == 0 and thr == full[()] and counts["checked"].tolist() == [n, 4 * n, 16 * n, 64 * n]
    assert sim.search(full, "none", weights, 100000, 8)[0] != full[()]  # and the search did prune
    for start, ppm, rounds in ((ref.thr((0, 0, 0), (1024, 1024, 1024)), 0, 8), (full, 1000001, 8), (full, 1000, -1)):
        with pytest.raises(pkg.EthCnnError) as e:
            sim.search(start, "none", weights, ppm, rounds)
        assert e.value.code == pkg.ethcnn.ERR_ARG
    sim.reset()
    sim.add(probs)
    with pytest.raises(pkg.EthCnnError) as e:  # no labelled CTU
        sim.search(full, "none", weights, 1000, 8)
    assert e.value.code == pkg.ethcnn.ERR_ARG


def test_tool_end_to_end_on_a_predicted_all_intra_sequence(pkg, oracle, tmp_path):
    from test_gpu_calib import _textured_sequence
    from test_gpu_score import _labels_from_texture
    w, h, frames, qp = 256, 192, 2, 32
    luma = _textured_sequence(32, w, h, frames)
    lab = _labels_from_texture(luma)
    yuv, labels, models = str(tmp_path / "seq.yuv"), str(tmp_path / "Info_test_256x192_qp32_nf2_CUDepth.dat"), str(tmp_path / "models")
    with open(yuv, "wb") as f:
        for k in range(frames):
            f.write(luma[k].tobytes())
            f.write(bytes([128]) * (w * h // 2))
    lab.tofile(labels)
    os.mkdir(models)
    prefix = os.path.join(models, pkg.ethcnn.model_name_for_qp(qp))
    pkg.ethcnn.write_ckpt_blob(prefix, oracle.synth_blob(1, 8.0))
    thr_file, out = str(tmp_path / "candidate.txt"), str(tmp_path / "Thr_info.txt")
    cand = ref.thr((600, 700, 800), (400, 300, 200))
    pkg.ethcnn.sim_write_thr_info(thr_file, cand, "ai")
    source = ["--yuv", yuv, str(w), str(h), str(qp), "--labels", labels, "--model-dir", models]
    r = subprocess.run([sys.executable, TOOL, "--thr-info", thr_file, "--order", "ai", "--json"] + source, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    # the same prediction, gates open, evaluated here and by the restatement
    c = pkg.EthCnn(device=0)
    c.load_checkpoint(prefix)
    c.set_thresholds(0.0, 0.0)
    dat = str(tmp_path / "cu_depth.dat")
    assert c.predict_yuv_file(yuv, w, h, qp, dat) == frames
    probs = np.fromfile(dat, "<f4")
    s = ref.Set()
    s.add_frames(probs, lab, w, h)
    with pkg.PartitionSim(c) as sim:
        sim.add_frames(probs, lab, w, h)
        got, full = sim.eval(cand, "ai")[0], sim.eval(ref.thr(*ref.FULL))[0]
        assert sim.info() == s.info() == rep["info"] and rep["info"]["labelled_ctus"] == frames * 12
    c.close()
    assert ref.equal(got, s.evaluate(cand, ref.GATES_AI)[0]) and got["checked"].any()
    assert rep["gates"] == "ai" and rep["up_k"] == [600, 700, 800] and rep["down_k"] == [400, 300, 200]
    for f in ref.FIELDS:
        assert rep[f] == (int(got[f]) if f == "bad_ctus" else got[f].tolist()), f
    assert rep["full_checked"] == full["checked"].tolist() == [frames * 12 * x for x in (1, 4, 16, 64)]
    assert rep["cost"] == sum(wt * int(x) for wt, x in zip((64, 16, 4, 1), got["checked"])) and rep["full_cost"] == frames * 12 * 4 * 64
    # the joint search writes a file that the library's parser reads back to the same grid values
    r = subprocess.run([sys.executable, TOOL, "--search", "--max-bad-ppm", "250000", "--out", out, "--order", "ai", "--json"] + source,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    want_thr, want_counts, want_rounds = s.search(ref.thr(*ref.FULL), ref.GATES_AI, (64, 16, 4, 1), 250000, 16)
    assert rep["up_k"] == want_thr["up_k"].tolist() and rep["down_k"] == want_thr["down_k"].tolist() and rep["rounds"] == want_rounds
    assert rep["checked"] == want_counts["checked"].tolist() and rep["bad_ctus"] == int(want_counts["bad_ctus"])
    assert rep["bad_ctus"] * 10 ** 6 <= 250000 * rep["info"]["labelled_ctus"]
    assert open(out).read() == calib_ref.thr_info_line([{"down_k": d, "up_k": u} for d, u in zip(rep["down_k"], rep["up_k"])], "ai")
    t1, t3 = pkg.ethcnn.parse_thresholds(out)  # tokens [1] and [3]: down1, down2 in the AI order
    assert (np.float32(t1), np.float32(t3)) == (np.float32(rep["down_k"][0] / 1024.0), np.float32(rep["down_k"][1] / 1024.0))
