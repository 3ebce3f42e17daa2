"""GPU: the ETH-LSTM driver and sample builder end to end.  train_LSTM_CTU64.py --export-lstm in a subprocess, the exported bundle
through load_lstm_checkpoint, twenty chained lstm_step calls against the trainer's evaluation (qp_scale 0.18: the deployed feature),
bit-exact inference against the oracle chain, ldp_step and both LDP daemons; get_LSTM_input.py against a numpy transcription fed
with resi_vectors.  Tolerance trainer vs lstm_step: atol 1e-5 on states and probabilities (tests/test_gpu_train_lstm.py)."""
import importlib
import os
import shutil
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import train_data_ldp
import train_data_lstm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "resi_to_cu_depth_ldp")
REC = 37264


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _drive(work, frames, w, h, qp, alive):
    """HM's side of the LDP file handshake, played from the test -> the cu_depth.dat bytes of each frame"""
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


@pytest.fixture(scope="module")
def exported(pkg, tmp_path_factory):
    """driver: 1000 steps at QP 32, qp_scale 0.18, --export-lstm; then --reload for 1000 more"""
    tmp = tmp_path_factory.mktemp("lstm_driver")
    (tmp / "train.dat").write_bytes(train_data_lstm.make_samples(400, seed=31))
    (tmp / "valid.dat").write_bytes(train_data_lstm.make_samples(200, seed=32))
    drv = os.path.join(ROOT, "hevc-complexity-reduction_amd", "train_LSTM_CTU64.py")
    base = [sys.executable, drv, "--train", "train.dat", "--valid", "valid.dat", "--batch", "16", "--qp", "32", "--qp-scale", "0.18"]
    r = subprocess.run(base + ["--iters", "1000", "--export-lstm", "."], cwd=str(tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return tmp, base, r.stdout


def test_driver_log_checkpoints_reload_and_export(pkg, exported):
    tmp, base, out = exported
    assert "step 1000: loss=[[" in out and "tendency = [[" in out and "QP 32:" in out
    lines = (tmp / "Models" / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
    assert lines[0] == "1000" and lines[-1] == ""
    assert [len(ln.split("  ")) for ln in lines[1:-1]] == [19, 19] and lines[2].startswith("1000  ")
    first, last = [float(v) for v in lines[1].split("  ")], [float(v) for v in lines[2].split("  ")]
    assert sum(last[1:4]) < sum(first[1:4])  # the training part's loss_list fell
    name = pkg.ethcnn.lstm_model_name_for_qp(32)
    assert name == "model_LDP_200000_qp32.dat"
    blob = pkg.ethcnn.read_ckpt_lstm_blob(str(tmp / "Models" / "model.dat"))
    assert np.array_equal(pkg.ethcnn.read_ckpt_lstm_blob(str(tmp / name)).view(np.uint32), blob.view(np.uint32))
    r = subprocess.run(base + ["--iters", "1000", "--reload"], cwd=str(tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "iter_times_last = 1000" in r.stdout
    lines = (tmp / "Models" / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
    assert lines[0] == "2000" and len(lines) == 5 and lines[3].startswith("2000  ")
    assert any(f.startswith("model_") and f.endswith("_2000_qp32.dat.index") for f in os.listdir(str(tmp / "Models")))
    assert not np.array_equal(pkg.ethcnn.read_ckpt_lstm_blob(str(tmp / "Models" / "model.dat")), blob)


def test_exported_model_in_lstm_step_ldp_step_and_daemons(pkg, ctx, oracle, exported, tmp_path, monkeypatch):
    import ethcnn_lstm_np as lstm
    tmp = exported[0]
    prefix = str(tmp / "model_LDP_200000_qp32.dat")
    lblob = pkg.ethcnn.read_ckpt_lstm_blob(prefix)
    # 24 samples at QP 32 with one i_frame, so that one lstm_step call per time step serves them all
    n, i_frame = 24, 1030
    raw = np.frombuffer(train_data_lstm.make_samples(n, seed=33, qps=(32,)), np.uint8).reshape(n, REC).copy()
    raw[:, 10:14] = np.array([i_frame], "<u4").view(np.uint8)
    t = pkg.LstmTrainer(ctx, batch=8, qp_scale=0.18)
    t.set_samples(1, raw)
    t.set_blob(lblob)
    _, _, probs = t.evaluate(1, n=n, want_probs=True)
    C = t.debug_fetch(pkg.ethcnn.LDBG_STATE_C).reshape(n, 20, 448)
    H = t.debug_fetch(pkg.ethcnn.LDBG_STATE_H).reshape(n, 20, 448)
    t.close()
    probs = probs.reshape(n, 20, 21)
    vec = raw[:, 64:].view(np.float32).reshape(n, 20, 465)[:, :, 17:]
    e = pkg.EthCnn(device=0)
    e.load_lstm_checkpoint(prefix)
    assert np.array_equal(e.get_lstm_blob().view(np.uint32), lblob.view(np.uint32))
    thr = e.get_thresholds()
    state = ostate = prev = None
    passed = 0
    for ts in range(20):
        p = 19 - ts                       # the cell reads slot 19 first; its heads get the features of slot ts (frame i_frame - ts)
        got, state = e.lstm_step(vec[:, p], state, 32, i_frame - ts)
        want, ostate = lstm.lstm_step(lblob, vec[:, p], ostate, 32, i_frame - ts, thr[0], thr[1], mode=0)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(state), _bits(ostate)), ts  # inference: bit-exact
        np.testing.assert_allclose(state[:, 0], C[:, p], rtol=0, atol=1e-5)
        np.testing.assert_allclose(state[:, 1], H[:, p], rtol=0, atol=1e-5)
        ungated, _ = lstm.lstm_forward64(lblob, vec[:, p], prev, 32, i_frame - ts)
        prev = ostate
        through = np.abs(got - ungated) < 1e-6  # the entries the gates passed
        np.testing.assert_allclose(got[through], probs[:, p][through], rtol=0, atol=1e-5)
        np.testing.assert_allclose(probs[:, p], ungated, rtol=0, atol=1e-5)  # the trainer's (ungated) = the deployed graph's
        assert through[:, 0].all()
        passed += int(through.sum())
    assert passed > 20 * n * 2
    # ldp_step and both daemons: a residual CNN (initial weights) + the exported LSTM, no synthetic seed
    c = pkg.Trainer(ctx, batch=8, net="ldp")
    c.init_weights(5)
    cblob = c.get_blob()
    c.close()
    cprefix = str(tmp_path / "model_LDP_2000000_qp22~37.dat")
    pkg.ethcnn.write_ckpt_blob(cprefix, cblob)
    w, h, qp = 416, 240, 32
    rng = np.random.default_rng(8)
    frames = [rng.integers(96, 160, size=(h, w), dtype=np.uint8) for _ in range(3)]
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    e.load_checkpoint(cprefix)
    e.set_thresholds(0.6, 0.7)  # Thr_info.txt below
    thr = (0.6, 0.7)
    want_frames, ostate = [], None
    for poc, luma in enumerate(frames, 1):
        want, ostate = lstm.lstm_step(lblob, oracle.resi_vectors(cblob, luma, w, h), ostate, qp, poc, thr[0], thr[1], mode=0)
        want_frames.append(want)
        assert np.array_equal(_bits(e.ldp_step(luma, w, h, qp, poc)), _bits(want)), poc
    e.close()
    monkeypatch.delenv("ETHCNN_SYNTHETIC_SEED", raising=False)
    works = {}
    for kind in ("python", "native"):
        work = tmp_path / kind
        work.mkdir()
        for ext in (".index", ".data-00000-of-00001"):
            shutil.copy(cprefix + ext, work / ("model_LDP_2000000_qp22~37.dat" + ext))
            shutil.copy(prefix + ext, work / ("model_LDP_200000_qp32.dat" + ext))
        (work / "Thr_info.txt").write_text("0.4 0.6 0.3 0.7 0.2 0.8")
        works[kind] = str(work)
    d = pkg.resi_to_cu_depth_LDP
    result = {}
    th = threading.Thread(target=lambda: result.setdefault("n", d.serve(works["python"], max_frames=3, idle_timeout=60.0, verbose=False)))
    th.start()
    try:
        got = _drive(works["python"], frames, w, h, qp, th.is_alive)
    finally:
        th.join(timeout=90)
    assert result.get("n") == 3
    for poc, (raw_out, want) in enumerate(zip(got, want_frames), 1):
        assert np.array_equal(_bits(np.frombuffer(raw_out, np.float32).reshape(nctu, 21)), _bits(want)), poc
    if os.path.exists(NATIVE):
        env = {k: v for k, v in os.environ.items() if k != "ETHCNN_SYNTHETIC_SEED"}
        pr = subprocess.Popen([NATIVE, "--max-frames", "3", "--idle-timeout", "60", "--quiet"], cwd=works["native"], env=env,
                              stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        try:
            nat = _drive(works["native"], frames, w, h, qp, lambda: pr.poll() is None)
        finally:
            _, err = pr.communicate(timeout=90)
        assert pr.returncode == 0, err
        assert nat == got


def test_get_lstm_input_against_the_transcription(pkg, ctx, tmp_path):
    """a small LDP file (192x128: 6 CTUs a frame, 42 frames) through get_LSTM_input.py in a subprocess; expected bytes from the
    numpy transcription of the definition fed with resi_vectors of the same checkpoint"""
    G = importlib.import_module("hevc-complexity-reduction_amd.get_LSTM_input")
    per, frames = 6, 42
    rec = np.frombuffer(train_data_ldp.make_records(per * frames, seed=5, width=192, height=128), np.uint8).reshape(-1, 16516).copy()
    for r in range(len(rec)):
        rec[r, 10:14] = np.array([r // per], "<u4").view(np.uint8)
    (tmp_path / "ldp.dat").write_bytes(rec.tobytes())
    c = pkg.Trainer(ctx, batch=8, net="ldp")
    c.init_weights(7)
    cblob = c.get_blob()
    c.close()
    cprefix = str(tmp_path / "cnn.dat")
    pkg.ethcnn.write_ckpt_blob(cprefix, cblob)
    tool = os.path.join(ROOT, "hevc-complexity-reduction_amd", "get_LSTM_input.py")
    r = subprocess.run([sys.executable, tool, "--model", cprefix, "--input", "ldp.dat", "--out", "lstm.dat", "--seed", "4"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "-> 72 samples (18 per QP); 0 skipped" in r.stdout  # frames 20, 30, 40 x 6 CTUs x 4 QPs
    got = np.fromfile(str(tmp_path / "lstm.dat"), np.uint8).reshape(-1, REC)
    e = pkg.EthCnn(device=0)
    e.load_blob(cblob)
    want = []
    for s in range(4):
        o = 64 + 4113 * s
        # resi_vectors frame by frame (192 x 128), not through the tool's tiling
        vec = np.concatenate([e.resi_vectors(np.ascontiguousarray(rec[f * per:(f + 1) * per, o + 17: o + 17 + 4096].reshape(2, 3, 64, 64)
                                                                   .transpose(0, 2, 1, 3).reshape(128, 192)), 192, 128) for f in range(frames)])
        for rr in range(len(rec)):
            fr = rr // per
            if fr < 19 or fr % 10:
                continue
            slots = [np.concatenate([rec[rr - k * per, o: o + 17].astype(np.float32), vec[rr - k * per]]) for k in range(20)]
            info = rec[rr, :64].copy()
            info[0] = 19
            want.append(np.concatenate([info, np.stack(slots).astype(np.float32).reshape(-1).view(np.uint8)]))
    e.close()
    assert np.array_equal(got, np.stack(want))
    sh = np.fromfile(str(tmp_path / "lstm.dat_shuffled"), np.uint8).reshape(-1, REC)
    assert np.array_equal(sh, G.shuffle_groups(got, 4)) and not np.array_equal(sh, got)
    t = pkg.LstmTrainer(ctx, batch=4)  # the trainer takes the file, QP selection included
    t.set_qps([27])
    assert t.set_samples(0, sh) == 18
    t.init_weights(1)
    l3, _ = t.step_indices(1, np.arange(4))
    assert np.isfinite(l3).all()
    t.close()
