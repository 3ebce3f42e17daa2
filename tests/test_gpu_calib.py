"""-m gpu: the threshold calibrator (include/ethcnn.h "threshold calibration") on the GPU against its numpy restatement
(tests/calib_ref.py): both label layouts, host and device entries, accumulation / reset, the error paths, and its three sources end to
end: the command-line tool over an All-Intra sequence (checked with tools/score_cu_depth.py), the device-resident output of the LDP
sequence call, and a trainer's evaluation of a sample file.  Counts are integers: every comparison is array_equal."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import calib_ref as ref
import train_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "calibrate_thresholds.py")
SCORER = os.path.join(ROOT, "tools", "score_cu_depth.py")

_CASES = {}


def _per_ctu_case(n):
    """(probs, depth, reference hist, reference rejected) of n CTUs, made once; CTU 0 is fully split and carries one NaN, one -0.5 and
    one 1.5 (one per level), so all three are counted as rejected"""
    if n not in _CASES:
        rng = np.random.default_rng(100 + n)
        probs, depth = ref.edge_probs(rng, n), ref.random_depths(rng, n)
        depth[0] = 3
        probs[0, 0], probs[0, 2], probs[0, 9] = np.nan, -0.5, 1.5
        hist, rej = ref.histogram(probs, depth)
        assert rej.tolist() == [1, 1, 1]
        for a in (probs, depth, hist, rej):
            a.setflags(write=False)
        _CASES[n] = (probs, depth, hist, rej)
    return _CASES[n]


@pytest.fixture
def cal(pkg, ctx):
    k = pkg.Calibrator(ctx)
    yield k
    k.close()


def _state(cal):
    hist, rej, skipped = cal.get()
    return hist, rej, skipped


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_per_ctu_layout_host_and_device(ctx, cal, n):
    probs, depth, want_hist, want_rej = _per_ctu_case(n)
    cal.add(probs, depth)
    hist, rej, skipped = _state(cal)
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej) and skipped == 0
    assert int(hist[0].sum()) + int(rej[0]) == n  # every CTU is a level-0 sample
    cal.reset()
    dp, dd = ctx.alloc(probs.nbytes), ctx.alloc(depth.nbytes)
    try:
        dp.upload(probs)
        dd.upload(depth)
        cal.add_device(dp, dd, n)
        hist_d, rej_d, skipped_d = _state(cal)
    finally:
        dp.free()
        dd.free()
    assert np.array_equal(hist_d, hist) and np.array_equal(rej_d, rej) and skipped_d == 0


@pytest.mark.parametrize("w,h,frames,skip,partial", [(128, 128, 2, 0, 0), (208, 144, 3, 1, 12)])
def test_frame_layout(ctx, cal, w, h, frames, skip, partial):
    rng = np.random.default_rng(w)
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    scored = frames - skip
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16)).astype(np.uint8)
    labels[skip, :4, :4] = 3  # the first CTU of the first scored frame is fully split
    probs = ref.edge_probs(rng, scored * nctu).reshape(scored, nctu, 21)
    probs[0, 0, 1] = np.nan
    want_hist, want_rej, want_skipped = ref.histogram_frames(probs, labels, w, h, skip)
    assert want_skipped == partial and int(want_rej.sum()) == 1
    cal.add_frames(probs, labels, w, h, skip_label_frames=skip)
    hist, rej, skipped = _state(cal)
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej) and skipped == partial
    cal.reset()
    dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes)
    try:
        dp.upload(probs)
        dl.upload(labels)
        cal.add_frames_device(dp, dl, w, h, scored, skip_label_frames=skip)
        hist_d, rej_d, skipped_d = _state(cal)
    finally:
        dp.free()
        dl.free()
    assert np.array_equal(hist_d, hist) and np.array_equal(rej_d, rej) and skipped_d == partial


def test_accumulation_reset_and_repeatability(cal):
    probs, depth, want_hist, want_rej = _per_ctu_case(5000)
    for a, b in ((0, 1), (1, 1300), (1300, 5000)):
        cal.add(probs[a:b], depth[a:b])
    cal.add(probs[:0], depth[:0])  # n == 0: a no-op
    hist, rej, _ = _state(cal)
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej)
    cal.reset()
    hist, rej, skipped = _state(cal)
    assert not hist.any() and not rej.any() and skipped == 0
    cal.add(probs, depth)
    first = _state(cal)
    cal.reset()
    cal.add(probs, depth)
    second = _state(cal)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    cal.add(probs, depth)  # and twice the set is twice the counts
    assert np.array_equal(_state(cal)[0], 2 * want_hist)


def test_errors_leave_the_accumulator_alone(pkg, cal):
    probs, depth, want_hist, want_rej = _per_ctu_case(257)
    cal.add(probs, depth)
    bad = depth.copy()
    bad[200, 7] = 4
    with pytest.raises(pkg.EthCnnError) as e:
        cal.add(probs, bad)
    assert e.value.code == pkg.ethcnn.ERR_FORMAT and "above 3" in str(e.value)
    hist, rej, _ = _state(cal)
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 4, size=(1, 8, 8)).astype(np.uint8)
    labels[0, 5, 6] = 200
    fprobs = ref.edge_probs(rng, 4)
    with pytest.raises(pkg.EthCnnError) as e:
        cal.add_frames(fprobs, labels, 128, 128)
    assert e.value.code == pkg.ethcnn.ERR_FORMAT
    assert np.array_equal(_state(cal)[0], want_hist)
    with pytest.raises(pkg.EthCnnError) as e:
        cal.add_frames(fprobs, labels, 120, 128, nframes=1)
    assert e.value.code == pkg.ethcnn.ERR_ARG
    with pytest.raises(pkg.EthCnnError) as e:
        cal.add_frames_device(8, 8, 128, 72, 1)
    assert e.value.code == pkg.ethcnn.ERR_ARG
    cal.add(probs, depth)  # the next valid call works
    assert np.array_equal(_state(cal)[0], 2 * want_hist)


# ---------------------------------------------------------------------------------------------------------- All-Intra end to end ---
def _textured_sequence(seed, w, h, frames):
    """luma whose 16x16 blocks have the local range of a random depth quadtree (train_data.depth_map), so that the texture labels of
    tests/test_gpu_score.py put both classes on all three levels"""
    rng = np.random.default_rng(seed)
    lo_hi = ((100, 110), (100, 150), (60, 200), (0, 256))  # ranges below 24, in [24, 96), in [96, 200), above 200
    luma = np.empty((frames, h, w), np.uint8)
    for f in range(frames):
        for cy in range(h // 64):
            for cx in range(w // 64):
                d = train_data.depth_map(rng)
                for by in range(4):
                    for bx in range(4):
                        lo, hi = lo_hi[int(d[by, bx])]
                        y, x = cy * 64 + by * 16, cx * 64 + bx * 16
                        luma[f, y:y + 16, x:x + 16] = rng.integers(lo, hi, size=(16, 16))
    return luma


def _score(labels, dat, w, h, thr):
    r = subprocess.run([sys.executable, SCORER, labels, dat, str(w), str(h)] + [repr(t) for t in thr], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [[int(x) for x in re.findall(r"\d+", line.split("=")[1].split("accuracy")[0])] for line in r.stdout.strip().splitlines()]


def test_all_intra_end_to_end_with_the_tool_and_the_scorer(pkg, oracle, tmp_path):
    from test_gpu_score import _labels_from_texture
    w, h, frames, qp, eps = 768, 512, 3, 32, 50000
    luma = _textured_sequence(31, w, h, frames)
    lab = _labels_from_texture(luma)
    # before the GPU is touched: both classes on all three levels (the probabilities play no part in the class sizes)
    sizes = ref.histogram_frames(np.full((frames, 96, 21), 0.5, np.float32), lab, w, h)[0].sum(axis=2)
    assert (sizes > 0).all(), sizes
    yuv, labels, models = str(tmp_path / "seq.yuv"), str(tmp_path / "Info_test_768x512_qp32_nf3_CUDepth.dat"), str(tmp_path / "models")
    with open(yuv, "wb") as f:
        for k in range(frames):
            f.write(luma[k].tobytes())
            f.write(bytes([128]) * (w * h // 2))
    lab.tofile(labels)
    os.mkdir(models)
    blob = oracle.synth_blob(1, 8.0)
    prefix = os.path.join(models, pkg.ethcnn.model_name_for_qp(qp))
    pkg.ethcnn.write_ckpt_blob(prefix, blob)
    out = str(tmp_path / "Thr_info.txt")
    r = subprocess.run([sys.executable, TOOL, "--eps-down", str(eps), str(eps), str(eps), "--eps-up", str(eps), str(eps), str(eps), "--out", out,
                        "--order", "ai", "--json", "--yuv", yuv, str(w), str(h), str(qp), "--labels", labels, "--model-dir", models],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    lv = rep["levels"]
    assert [[l["n0"], l["n1"]] for l in lv] == sizes.tolist() and rep["skipped_partial"] == 0 and rep["rejected"] == [0, 0, 0]
    # the same prediction, gates open, as a file for the scorer
    c = pkg.EthCnn(device=0)
    c.load_checkpoint(prefix)
    c.set_thresholds(0.0, 0.0)
    dat = str(tmp_path / "cu_depth.dat")
    assert c.predict_yuv_file(yuv, w, h, qp, dat) == frames
    c.close()
    at_down = _score(labels, dat, w, h, [l["down_k"] / 1024.0 for l in lv])  # [n00, n01, n10, n11] per level
    at_up = _score(labels, dat, w, h, [l["up_k"] / 1024.0 for l in lv])
    for l in range(3):
        assert at_down[l][2] == lv[l]["miss"] and at_up[l][1] == lv[l]["fsplit"], (l, at_down, at_up, lv)
        assert lv[l]["miss"] * 10 ** 6 <= eps * lv[l]["n1"] and lv[l]["fsplit"] * 10 ** 6 <= eps * lv[l]["n0"]
    # the ai order puts down1 / down2 where the predictors read their gates' thresholds: tokens [1] and [3]
    t1, t3 = pkg.ethcnn.parse_thresholds(out)
    assert (np.float32(t1), np.float32(t3)) == (np.float32(lv[0]["down_k"] / 1024.0), np.float32(lv[1]["down_k"] / 1024.0))
    assert open(out).read() == ref.thr_info_line(lv, "ai")
    # and the restatement on the same file agrees with the whole report
    want = ref.choose(ref.histogram_frames(np.fromfile(dat, "<f4"), lab, w, h)[0], [eps] * 3, [eps] * 3)
    assert [{k: l[k] for k in ("down_k", "up_k", "miss", "fsplit", "uncertain", "crossed")} for l in lv] == \
           [{k: l[k] for k in ("down_k", "up_k", "miss", "fsplit", "uncertain", "crossed")} for l in want]


# --------------------------------------------------------------------------------------------------------- device-resident LDP ---
def test_ldp_sequence_output_left_in_hbm(pkg, oracle):
    import ethcnn_lstm_np
    ctx = pkg.EthCnn(device=0)  # (a context of its own: the weights and the open gates stay out of the session's)
    cal = pkg.Calibrator(ctx)
    w, h, nf, qp = 416, 240, 3, 32
    nctu = pkg.ethcnn.ctus_per_frame(w, h)
    rng = np.random.default_rng(41)
    luma = rng.integers(0, 256, size=(nf, h, w), dtype=np.uint8)
    luma[:, : h // 2] = (luma[:, : h // 2] // 16 + 120).astype(np.uint8)
    labels = rng.integers(0, 4, size=(nf + 1, h // 16, w // 16)).astype(np.uint8)  # POC 0 first: one label frame is passed over
    ctx.load_blob(oracle.synth_blob(21, 1.0))
    ctx.load_lstm_blob(ethcnn_lstm_np.synth_lstm_blob(22, 3.0))
    ctx.set_thresholds(0.0, 0.0)  # open gates
    dl, dp, dlab = ctx.alloc(luma.nbytes), ctx.alloc(nf * nctu * 21 * 4), ctx.alloc(labels.nbytes)
    try:
        dl.upload(luma)
        dlab.upload(labels)
        ctx.ldp_sequence_device(dl, w, h, nf, qp, 1, dp)
        cal.add_frames_device(dp, dlab, w, h, nf, skip_label_frames=1)  # the probabilities never left HBM
        got = _state(cal)
        probs = dp.download(np.float32, nf * nctu * 21)
    finally:
        for b in (dl, dp, dlab):
            b.free()
    cal.reset()
    cal.add_frames(probs, labels, w, h, skip_label_frames=1)
    back = _state(cal)
    assert np.array_equal(got[0], back[0]) and np.array_equal(got[1], back[1]) and got[2] == back[2] == nf * (28 - 18)
    want = ref.histogram_frames(probs, labels, w, h, 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert int(got[0][0].sum()) == nf * 18 and int(got[0][2].sum()) > 0
    ctx.close()


# -------------------------------------------------------------------------------------------------------------------- samples ---
def test_tool_over_a_sample_file_equals_trainer_evaluate(pkg, ctx, cal, tmp_path):
    n, qp = 200, 32
    data = train_data.make_records(n, seed=13)
    path, prefix, hist_path = str(tmp_path / "AI_valid.dat"), str(tmp_path / "model.dat"), str(tmp_path / "hist.bin")
    with open(path, "wb") as f:
        f.write(data)
    with pkg.Trainer(ctx, batch=8, dropout=False, seed=2) as t:
        t.init_weights(5)
        blob = t.get_blob()
        t.set_samples(pkg.ethcnn.SET_VALID, data)
        probs = t.evaluate(pkg.ethcnn.SET_VALID, qp, n=n, want_probs=True)[2]
    pkg.ethcnn.write_ckpt_blob(prefix, blob)
    rec = np.frombuffer(data, np.uint8).reshape(n, train_data.REC)
    depth = rec[:, 4160 + 16 * qp: 4176 + 16 * qp]
    cal.add(probs, depth)
    hist, rej, _ = _state(cal)
    assert np.array_equal(hist, ref.histogram(probs, depth)[0])
    r = subprocess.run([sys.executable, TOOL, "--json", "--hist", hist_path, "--eps-down", "100000", "100000", "100000", "--samples", path,
                        "--model", prefix, "--qp", str(qp), "--net", "ai"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    assert np.array_equal(np.fromfile(hist_path, "<u8").reshape(3, 2, ref.BINS), hist) and rep["rejected"] == [int(x) for x in rej]
    want = cal.choose([100000] * 3, [50000] * 3).as_dicts()
    assert [{k: l[k] for k in l if k in want[0]} for l in rep["levels"]] == want
