"""GPU: the Low-Delay-P residual ETH-CNN trainer (include/ethcnn.h "training", net = ETHCNN_TRAIN_NET_LDP) against the float64
torch restatement of ETH-CNN_Training_LDP/net_CTU64.py:94-209 (tests/train_ref_ldp.py), the tuning modes, and its checkpoint
through LDP inference and both LDP daemons.  Data: seeded synthetic 16516-byte records (tests/train_data_ldp.py)."""
import os
import shutil
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import train_data_ldp
import train_ref
import train_ref_ldp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM32 = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
NATIVE = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "resi_to_cu_depth_ldp")
QPS = [22, 27, 32, 37]
NREC = 600
DATA = train_data_ldp.make_records(NREC, seed=11)
VALID = train_data_ldp.make_records(3000, seed=12)
OFFS = {n: (o // 4, int(np.prod(s))) for n, s, o in train_ref.ethcnn_np.TENSORS}


def _trainer(pkg, ctx, batch, dropout=False, seed=5, **kw):
    t = pkg.Trainer(ctx, batch=batch, dropout=dropout, seed=seed, net="ldp", **kw)
    t.set_samples(0, DATA)
    return t


def _close(g, gref, names=None, rel=1e-4, floor=1e-7):
    for name, (off, n) in OFFS.items():
        if names is not None and name not in names:
            continue
        a, b = g[off: off + n], gref[off: off + n]
        tol = rel * np.abs(b).max() + floor
        err = np.abs(a - b).max()
        assert err <= tol, "%s: max |g - g_ref| = %g > %g" % (name, err, tol)


@pytest.mark.parametrize("batch", [64, 7, 200])
def test_gradients_of_one_step(pkg, ctx, batch):
    t = _trainer(pkg, ctx, batch)
    t.init_weights(3)
    w0 = t.get_blob()
    rng = np.random.default_rng(batch)
    idx = rng.integers(0, NREC, batch)
    qps = rng.choice(QPS, batch)
    l3, a3 = t.step_indices(1, idx, qps)
    luma, lab = train_ref_ldp.parse_records(DATA, idx, qps)
    ref, gref = train_ref_ldp.loss_and_grad(w0, luma, lab, qps)
    np.testing.assert_allclose(l3, ref["loss_list"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(a3, ref["accuracy_list"], rtol=0, atol=1e-5)
    _close(t.debug_fetch(pkg.ethcnn.TDBG_GRADS), gref)
    np.testing.assert_allclose(t.debug_fetch(pkg.ethcnn.TDBG_PROBS).reshape(batch, 21), ref["probs"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(t.debug_fetch(pkg.ethcnn.TDBG_H1).reshape(batch, 448), ref["H1"], rtol=1e-5, atol=1e-5)
    t.close()


def test_init_weights_draw_the_biases(pkg, ctx):
    """LDP bias_variable is truncated normal too (net_CTU64.py:38-40); All-Intra keeps tf.constant(0.01)"""
    t = _trainer(pkg, ctx, 8)
    t.init_weights(3)
    w = t.get_blob()
    t.close()
    u = pkg.Trainer(ctx, batch=8)
    u.init_weights(3)
    v = u.get_blob()
    u.close()
    for name in ("h_fc1__64__b", "Variable_1", "y_conv_flat__16__b"):
        off, n = OFFS[name]
        assert (v[off: off + n] == np.float32(0.01)).all()
        b = w[off: off + n]
        assert np.abs(b).max() <= 0.2 and len(np.unique(b)) == n
    off, n = OFFS["h_fc1__64__w"]
    assert np.array_equal(w[off: off + n], v[off: off + n])  # the weights: the same generator, the same draws


def test_dropout_masks_device_batches_and_gradients(pkg, ctx):
    batch, seed, step = 32, 77, 9
    t = _trainer(pkg, ctx, batch, dropout=True, seed=seed)
    t.init_weights(4)
    w0 = t.get_blob()
    t.run(step, 1)  # device-drawn: index and slot QP
    got = t.debug_fetch(pkg.ethcnn.TDBG_INDICES).reshape(batch, 2)
    idx, qp = train_ref.batch_of(seed, step, batch, NREC, QPS)
    assert np.array_equal(got[:, 0], idx) and np.array_equal(got[:, 1], qp) and len(set(qp)) == 4
    m1 = t.debug_fetch(pkg.ethcnn.TDBG_MASK_FC1).reshape(batch, 448)
    m2 = t.debug_fetch(pkg.ethcnn.TDBG_MASK_FC2).reshape(batch, 336)
    r1, r2 = train_ref.dropout_masks(seed, step, batch)
    assert np.array_equal(m1, r1) and np.array_equal(m2, r2)
    luma, lab = train_ref_ldp.parse_records(DATA, idx, qp)
    _, gref = train_ref_ldp.loss_and_grad(w0, luma, lab, qp, r1, r2)
    _close(t.debug_fetch(pkg.ethcnn.TDBG_GRADS), gref)
    t.close()


@pytest.mark.parametrize("tune", [1, 2, 3])
def test_tuning_modes(pkg, ctx, tune):
    tag = train_ref_ldp.TUNE_TAGS[tune]
    mask = train_ref_ldp.tune_mask(tune)
    rng = np.random.default_rng(tune)
    # 20 device-drawn steps from non-zero accumulators: every frozen tensor and its accumulator bit-identical
    t = _trainer(pkg, ctx, 64, dropout=True, seed=3, tune=tune)
    t.init_weights(7)
    w0 = t.get_blob()
    a0 = (rng.standard_normal(w0.size) * 1e-3).astype(np.float32)
    t.set_blob(w0, a0)
    t.run(1, 20)
    w1, a1 = t.get_blob(with_accum=True)
    t.close()
    assert np.array_equal(w1[~mask].view(np.uint32), w0[~mask].view(np.uint32))
    assert np.array_equal(a1[~mask].view(np.uint32), a0[~mask].view(np.uint32))
    for name, (off, n) in OFFS.items():
        assert (tag in name) == (not np.array_equal(w1[off: off + n], w0[off: off + n])), name
    # the tuned head follows the restatement's masked update (3 explicit steps, mixed slots)
    t = _trainer(pkg, ctx, 16, tune=tune, lr=0.05)
    t.init_weights(8)
    w = t.get_blob().astype(np.float64)
    acc = np.zeros_like(w)
    for step in range(1, 4):
        idx, qps = rng.integers(0, NREC, 16), rng.choice(QPS, 16)
        luma, lab = train_ref_ldp.parse_records(DATA, idx, qps)
        _, g = train_ref_ldp.loss_and_grad(w, luma, lab, qps)
        w, acc = train_ref_ldp.masked_momentum_update(w, acc, g, train_ref.lr_at(step, 0.05), tune)
        t.step_indices(step, idx, qps)
    gw, gacc = t.get_blob(with_accum=True)
    t.close()
    assert np.abs(gw - w).max() <= 1e-5 * np.abs(w).max()
    assert np.abs(gacc - acc).max() <= 1e-5 * np.abs(acc).max()
    assert not gacc[~mask].any()


def test_determinism_and_exact_resume(pkg, ctx):
    blobs = []
    for seed in (9, 9):
        t = _trainer(pkg, ctx, 64, dropout=True, seed=seed)
        t.init_weights(2)
        t.run(1, 500)
        blobs.append(t.get_blob())
        t.close()
    assert np.array_equal(blobs[0].view(np.uint32), blobs[1].view(np.uint32)) and np.isfinite(blobs[0]).all()
    t = _trainer(pkg, ctx, 32, dropout=True, seed=4)
    t.init_weights(5)
    w_init = t.get_blob()
    t.run(1, 200)
    straight = t.get_blob()
    t.set_blob(w_init)
    t.run(1, 100)
    w, acc = t.get_blob(with_accum=True)
    t.close()
    u = _trainer(pkg, ctx, 32, dropout=True, seed=4)
    u.set_blob(w, acc)
    u.run(101, 100)
    resumed = u.get_blob()
    u.close()
    assert np.array_equal(straight.view(np.uint32), resumed.view(np.uint32))


def test_evaluation_is_one_batch(pkg, ctx):
    t = _trainer(pkg, ctx, 64, seed=17)
    t.set_samples(1, VALID)
    t.init_weights(8)
    w0 = t.get_blob()
    n = 3000
    slots = pkg.ethcnn.mixed_eval_slots(17, n)
    assert slots.tolist() == [(train_ref.draw(17, 2, 0, i, 0) >> 32) * 4 >> 32 for i in range(n)]
    for qp, qps in ((32, np.full(n, 32)), (-1, np.array(QPS)[slots])):
        l3, a3, probs = t.evaluate(1, qp, n=n, want_probs=True)
        luma, lab = train_ref_ldp.parse_records(VALID, np.arange(n), qps)
        out, _ = train_ref_ldp.loss_and_grad(w0, luma, lab, qps)
        np.testing.assert_allclose(l3, out["loss_list"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(probs, out["probs"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(a3, train_ref.accuracy(probs, lab), rtol=0, atol=1e-6)
        chunks = [train_ref_ldp.loss_and_grad(w0, luma[i:i + 1024], lab[i:i + 1024], qps[i:i + 1024])[0]["loss_list"]
                  for i in range(0, n, 1024)]
        assert np.abs(np.mean(chunks, axis=0) - out["loss_list"]).max() > 1e-5
    t.close()


def test_learning_on_synthetic_data(pkg, ctx):
    """Calibration: train_ref_ldp (float64, CPU), batch 64, lr 0.01, momentum 0.9, no dropout, the documented device batches of
    seed 31 over the four slots, its own truncated-normal init: mixed-slot validation loss_list (64, 32, 16) 0.689 0.728 0.770 ->
    0.012 0.177 0.405 after 100 steps and 0.00001 0.0025 0.011 after 300; accuracy_list 0.630 0.574 0.555 -> 1.000 0.966 0.846 at step
    100.  The thresholds sit well inside that: the summed loss below 0.8x its start, the 64x64 accuracy at least 0.85."""
    t = _trainer(pkg, ctx, 64, seed=31)
    t.set_samples(1, VALID)
    t.init_weights(12)
    l0, a0 = t.evaluate(1, -1, n=2000)
    t.run(1, 300)
    l1, a1 = t.evaluate(1, -1, n=2000)
    assert l1.sum() < 0.8 * l0.sum(), (l0, l1)
    assert a1[0] >= 0.85 and a1[0] > a0[0], (a0, a1)
    t.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _drive(work, frames, w, h, qp, alive):
    """HM's side of the file handshake (TEncGOP.cpp:1463-1503), played from the test: -> the cu_depth.dat bytes of each frame"""
    out = []
    for poc, luma in enumerate(frames, 1):
        with open(os.path.join(work, "resi.yuv"), "wb") as f:
            f.write(luma.tobytes())
            f.write(bytes(w * h // 2))
        with open(os.path.join(work, "command.dat"), "w") as f:
            f.write("%d %d %d %d [end]" % (poc, w, h, qp))
        open(os.path.join(work, "pred_start.sig"), "w").close()
        t0 = time.time()
        while not os.path.exists(os.path.join(work, "pred_end.sig")):
            assert time.time() - t0 < 90 and alive(), "daemon did not answer frame %d" % poc
            time.sleep(0.001)
        os.remove(os.path.join(work, "pred_end.sig"))
        out.append(open(os.path.join(work, "cu_depth.dat"), "rb").read())
    return out


def test_checkpoint_into_ldp_inference_and_daemons(pkg, ctx, oracle, tmp_path, monkeypatch):
    import ethcnn_lstm_np as lstm
    t = _trainer(pkg, ctx, 40, seed=2)
    t.init_weights(13)
    t.run(1, 50)
    blob = t.get_blob()
    idx, qps = np.arange(40) * 7, np.full(40, 32)
    t.step_indices(51, idx, qps)  # dropout-free: DBG_H1 = the FC1 vectors of `blob`
    h1 = t.debug_fetch(pkg.ethcnn.TDBG_H1).reshape(40, 448)
    t.close()
    export = tmp_path / "export"
    export.mkdir()
    prefix = str(export / "model_LDP_2000000_qp22~37.dat")
    pkg.ethcnn.write_ckpt_blob(prefix, blob)
    # the same 40 residual CTUs tiled into a 512 x 320 frame (8 x 5 CTUs, raster order)
    resi, _ = train_ref_ldp.parse_records(DATA, idx, qps)
    frame = np.ascontiguousarray(resi.reshape(5, 8, 64, 64).transpose(0, 2, 1, 3).reshape(320, 512))
    e = pkg.EthCnn(device=0)
    e.load_checkpoint(prefix)
    assert np.array_equal(e.get_blob().view(np.uint32), blob.view(np.uint32))
    np.testing.assert_allclose(e.resi_vectors(frame, 512, 320), h1, rtol=1e-5, atol=1e-5)
    e.close()
    # the Python daemon: exported CNN + the reference's trained QP-32 LSTM, no synthetic seed
    monkeypatch.delenv("ETHCNN_SYNTHETIC_SEED", raising=False)
    w, h, qp = 416, 240, 32
    rng = np.random.default_rng(8)
    frames = [np.ascontiguousarray(frame[:h, :w])] + [rng.integers(96, 160, size=(h, w), dtype=np.uint8) for _ in range(2)]
    works = {}
    for kind in ("python", "native"):
        work = tmp_path / kind
        work.mkdir()
        for ext in (".index", ".data-00000-of-00001"):
            shutil.copy(prefix + ext, work / ("model_LDP_2000000_qp22~37.dat" + ext))
            shutil.copy(LSTM32 + ext, work / ("model_LDP_200000_qp32.dat" + ext))
        (work / "Thr_info.txt").write_text("0.4 0.6 0.3 0.7 0.2 0.8")
        works[kind] = str(work)
    d = pkg.resi_to_cu_depth_LDP
    result = {}
    th = threading.Thread(target=lambda: result.setdefault("n", d.serve(works["python"], max_frames=3, idle_timeout=60.0,
                                                                       verbose=False)))
    th.start()
    try:
        got = _drive(works["python"], frames, w, h, qp, th.is_alive)
    finally:
        th.join(timeout=90)
    assert result.get("n") == 3
    lblob = np.fromfile(LSTM32 + ".data-00000-of-00001", dtype=np.float32)
    state = None
    n = ((w + 63) // 64) * ((h + 63) // 64)
    for poc, (luma, raw) in enumerate(zip(frames, got), 1):
        want, state = lstm.lstm_step(lblob, oracle.resi_vectors(blob, luma, w, h), state, qp, poc, 0.6, 0.7, mode=0)
        assert np.array_equal(_bits(np.frombuffer(raw, np.float32).reshape(n, 21)), _bits(want)), poc
    if os.path.exists(NATIVE):  # the native daemon: the same bytes on the same frames
        env = {k: v for k, v in os.environ.items() if k != "ETHCNN_SYNTHETIC_SEED"}
        p = subprocess.Popen([NATIVE, "--max-frames", "3", "--idle-timeout", "60", "--quiet"], cwd=works["native"], env=env,
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        try:
            nat = _drive(works["native"], frames, w, h, qp, lambda: p.poll() is None)
        finally:
            _, err = p.communicate(timeout=90)
        assert p.returncode == 0, err
        assert nat == got


def test_bad_arguments(pkg, ctx):
    E = pkg.EthCnnError
    for kw in ({"net": 2}, {"tune": 4}, {"tune": -1}):
        with pytest.raises(E) as ei:
            pkg.Trainer(ctx, batch=8, **kw)
        assert ei.value.code == -1
    t = pkg.Trainer(ctx, batch=8, net="ldp")
    with pytest.raises(E) as ei:
        t.set_qps([32])  # no training set yet: no slot QPs
    assert ei.value.code == -1
    with pytest.raises(E) as ei:
        t.set_samples(0, DATA[:-1])
    assert ei.value.code == -3
    with pytest.raises(E) as ei:
        t.set_samples(0, bytes(4992 * 331))  # 4992-byte records are not 16516-byte ones
    assert ei.value.code == -3
    mixed = np.frombuffer(DATA, np.uint8).reshape(NREC, -1).copy()
    mixed[417, 64 + 4113 * 2] = 33  # record 417's third slot at QP 33
    with pytest.raises(E) as ei:
        t.set_samples(0, mixed.tobytes())
    assert ei.value.code == -3 and "record 417" in str(ei.value)
    mixed[417, 64 + 4113 * 2] = 32
    mixed[0, 64 + 4113] = 22  # record 0: two slots at QP 22
    with pytest.raises(E) as ei:
        t.set_samples(0, mixed.tobytes())
    assert ei.value.code == -3
    t.set_samples(0, DATA)
    for qps in ([30], [22, 52], []):
        with pytest.raises(E) as ei:
            t.set_qps(qps)
        assert ei.value.code == -1
    t.set_qps([27])  # a subset: single-QP training
    t.init_weights(1)
    t.run(1, 1)
    assert set(t.debug_fetch(pkg.ethcnn.TDBG_INDICES).reshape(8, 2)[:, 1]) == {27}
    with pytest.raises(E) as ei:
        t.step_indices(1, [0] * 8, 30)
    assert ei.value.code == -1
    t.set_samples(1, DATA)
    for qp in (30, -2, 52):
        with pytest.raises(E) as ei:
            t.evaluate(1, qp, n=10)
        assert ei.value.code == -1
    t.close()
    a = pkg.Trainer(ctx, batch=8)
    a.set_samples(1, train_data_ldp.make_records(1, 1)[:4992 * 3])
    with pytest.raises(E) as ei:
        a.evaluate(1, -1, n=3)  # qp = -1 is LDP only
    assert ei.value.code == -1
    a.close()


def test_driver_train_reload_export(pkg, tmp_path):
    """train_resi_CNN_CTU64.py: the reference's log format and checkpoints, --reload continues the log, --export-ldp"""
    (tmp_path / "train.dat").write_bytes(DATA)
    (tmp_path / "valid.dat").write_bytes(VALID[: 300 * 16516])
    drv = os.path.join(ROOT, "hevc-complexity-reduction_amd", "train_resi_CNN_CTU64.py")
    base = [sys.executable, drv, "--train", "train.dat", "--valid", "valid.dat", "--batch", "16"]
    r = subprocess.run(base + ["--iters", "1000", "--export-ldp", "."], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "step 1000: loss=[[" in r.stdout and "tendency = [[" in r.stdout
    lines = (tmp_path / "Models" / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
    assert lines[0] == "1000" and lines[-1] == ""
    assert [len(ln.split("  ")) for ln in lines[1:-1]] == [19, 19] and lines[2].startswith("1000  ")
    blob = pkg.ethcnn.read_ckpt_blob(str(tmp_path / "Models" / "model.dat"))
    exported = pkg.ethcnn.read_ckpt_blob(str(tmp_path / "model_LDP_2000000_qp22~37.dat"))
    assert np.array_equal(exported.view(np.uint32), blob.view(np.uint32))
    r = subprocess.run(base + ["--iters", "1000", "--reload", "--partly-tuning-mode", "3"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "iter_times_last = 1000" in r.stdout
    lines = (tmp_path / "Models" / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
    assert lines[0] == "2000" and len(lines) == 5 and lines[3].startswith("2000  ")
    assert any(f.startswith("model_") and f.endswith("_2000_qp22~37.dat.index") for f in os.listdir(str(tmp_path / "Models")))
    tuned = pkg.ethcnn.read_ckpt_blob(str(tmp_path / "Models" / "model.dat"))
    mask = train_ref_ldp.tune_mask(3)
    assert np.array_equal(tuned[~mask].view(np.uint32), blob[~mask].view(np.uint32)) and not np.array_equal(tuned[mask], blob[mask])
