"""GPU: the ETH-LSTM trainer (include/ethcnn.h "ETH-LSTM training") against the float64 torch restatement of
ETH-LSTM_Training_LDP/net_CTU64.py:85-276 (tests/train_ref_lstm.py).  Data: seeded synthetic 37264-byte samples
(tests/train_data_lstm.py); weights: the golden qp32 bundle and the trainer's own initialisation.

Tolerances are the CNN trainer tests': atol 1e-5 on losses, accuracies, probabilities and states; per tensor
1e-4 max|g_ref| + 1e-7 on gradients; 1e-5 relative on the global norm.  The restatement run in float32 on 8 samples from the golden
weights differs from float64 by 9e-8 (probabilities), 8e-7 (c), 3e-7 (h) and at most 3.1e-7 max|g_ref| per tensor, so twenty steps
of fp32 recurrence fit these bounds with two orders of magnitude to spare and nothing wider is needed."""
import os

import numpy as np
import pytest

import train_data_lstm
import train_ref_lstm as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM32 = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
NREC = 300
DATA = train_data_lstm.make_samples(NREC, seed=21)
VALID = train_data_lstm.make_samples(700, seed=22)


def _trainer(pkg, ctx, batch, dropout=False, seed=5, **kw):
    t = pkg.LstmTrainer(ctx, batch=batch, dropout=dropout, seed=seed, **kw)
    assert t.set_samples(0, DATA) == NREC
    return t


def _close(g, gref, rel=1e-4, floor=1e-7):
    for name, (off, n) in R.OFFS.items():
        a, b = g[off: off + n], gref[off: off + n]
        tol = rel * np.abs(b).max() + floor
        err = np.abs(a - b).max()
        print("%-50s max|g_ref| %.3e  max|g - g_ref| %.3e  (tol %.3e)" % (name, np.abs(b).max(), err, tol))
        assert err <= tol, "%s: max |g - g_ref| = %g > %g" % (name, err, tol)


def _check_step(pkg, t, w0, idx, rows, qp_scale=1.0, masks=(None, None)):
    vec, lab, qps, gop = R.parse_samples(DATA, idx)
    ref, gref, norm = R.loss_and_grad(w0, vec, lab, qps, gop, qp_scale, *masks)
    L = pkg.ethcnn
    probs = t.debug_fetch(L.LDBG_PROBS).reshape(rows, 21)
    C, H = t.debug_fetch(L.LDBG_STATE_C).reshape(rows, 448), t.debug_fetch(L.LDBG_STATE_H).reshape(rows, 448)
    gn = float(t.debug_fetch(L.LDBG_NORM)[0])
    print("probs %.3e  c %.3e  h %.3e  norm %.9g vs %.9g" % (np.abs(probs - ref["probs"]).max(), np.abs(C - ref["C"]).max(),
                                                              np.abs(H - ref["H"]).max(), gn, norm))
    np.testing.assert_allclose(probs, ref["probs"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(C, ref["C"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(H, ref["H"], rtol=0, atol=1e-5)
    _close(t.debug_fetch(L.LDBG_GRADS), gref)
    assert abs(gn - norm) <= 1e-5 * norm
    return ref, gref, norm


@pytest.mark.parametrize("batch", [64, 7, 200])
@pytest.mark.parametrize("start", ["golden", "init"])
def test_one_step_against_the_restatement(pkg, ctx, batch, start):
    t = _trainer(pkg, ctx, batch)
    if start == "golden":
        t.set_blob(pkg.ethcnn.read_ckpt_lstm_blob(LSTM32))
    else:
        t.init_weights(3)
    w0 = t.get_blob()
    idx = np.random.default_rng(batch).integers(0, NREC, batch)
    l3, a3 = t.step_indices(1, idx)
    ref, _, _ = _check_step(pkg, t, w0, idx, batch * 20)
    print("loss", l3, ref["loss_list"], "accuracy", a3, ref["accuracy_list"])
    np.testing.assert_allclose(l3, ref["loss_list"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(a3, ref["accuracy_list"], rtol=0, atol=1e-5)
    t.close()


def test_init_weights_follow_the_documented_stream(pkg, ctx):
    t = _trainer(pkg, ctx, 4)
    t.init_weights(9)
    w = t.get_blob()
    t.close()
    names = ["RNN64/fc2/full_connect_b", "RNN64/fc2/full_connect_w", "RNN64/multi_rnn_cell/cell_0/lstm_cell/kernel",
             "RNN32/fc3/full_connect_w", "RNN16/fc3/full_connect_b"]
    ref = R.init_weights(9, names)
    for n in names:
        off, cnt = R.OFFS[n]
        assert np.array_equal(w[off: off + cnt], ref[off: off + cnt]), n
    for n, (off, cnt) in R.OFFS.items():
        if n.endswith("lstm_cell/bias"):
            assert not w[off: off + cnt].any()
    off, cnt = R.OFFS["RNN16/multi_rnn_cell/cell_0/lstm_cell/kernel"]
    lim = np.sqrt(6.0 / (512 + 1024))
    assert 0.99 * lim < np.abs(w[off: off + cnt]).max() <= lim


def test_dropout_masks_device_batches_and_gradients(pkg, ctx):
    batch, seed, step = 12, 77, 9
    t = _trainer(pkg, ctx, batch, dropout=True, seed=seed, qp_scale=0.18)
    t.init_weights(4)
    w0 = t.get_blob()
    t.run(step, 1)
    L = pkg.ethcnn
    idx = R.batch_of(seed, step, batch, NREC)
    assert np.array_equal(t.debug_fetch(L.LDBG_INDICES), idx)
    mh, m2 = R.dropout_masks(seed, step, batch * 20)
    assert np.array_equal(t.debug_fetch(L.LDBG_MASK_H).reshape(-1, 448), mh)
    assert np.array_equal(t.debug_fetch(L.LDBG_MASK_FC2).reshape(-1, 336), m2)
    assert 0.45 < mh.mean() < 0.55 and 0.75 < m2.mean() < 0.85
    _check_step(pkg, t, w0, idx, batch * 20, qp_scale=0.18, masks=(mh, m2))
    t.close()


@pytest.mark.parametrize("batch,scale,above", [(2, 4.0, True), (16, 1.0, False)])
def test_clip_and_update(pkg, ctx, batch, scale, above):
    """fc2 / fc3 matrices scaled by 4 at batch 2 (small batch-global counts) push the global norm over 5 (5.69; asserted on the
    restatement) without saturating a sigmoid in fp32 (probabilities stay within [3e-4, 1 - 2e-3]: at scale 6 they reach 1 - 3e-9,
    where fp32's 1 - p is 0 and the float32 restatement itself is 5% off); the plain initialisation at batch 16 stays under it"""
    t = _trainer(pkg, ctx, batch, lr=0.05)
    t.init_weights(6)
    w0 = t.get_blob()
    for n, (off, cnt) in R.OFFS.items():
        if "fc3/full_connect_w" in n or "fc2/full_connect_w" in n:
            w0[off: off + cnt] *= np.float32(scale)
    rng = np.random.default_rng(1)
    a0 = (rng.standard_normal(w0.size) * 1e-3).astype(np.float32)
    t.set_blob(w0, a0)
    idx = rng.integers(0, NREC, batch)
    t.step_indices(3, idx)
    _, gref, norm = _check_step(pkg, t, w0, idx, batch * 20)
    print("global norm", norm)
    assert (norm > 5.0) == above
    w1, a1 = t.get_blob(with_accum=True)
    wr, ar = R.train_step(w0.astype(np.float64), a0.astype(np.float64), gref, R.lr_at(3, 0.05))
    for n, (off, cnt) in R.OFFS.items():
        tol = 1e-4 * np.abs(ar[off: off + cnt]).max() + 1e-7
        assert np.abs(a1[off: off + cnt] - ar[off: off + cnt]).max() <= tol, n
        assert np.abs(w1[off: off + cnt] - wr[off: off + cnt]).max() <= 0.05 * tol + 1e-7, n
    if above:  # the clipped accumulator is NOT the unclipped one
        assert np.abs(a1 - (a0 * 0.9 + gref)).max() > 1e-3
    t.close()


def test_decay_boundary_determinism_and_resume(pkg, ctx):
    def make():
        t = _trainer(pkg, ctx, 16, dropout=True, seed=11, decay_steps=3, lr=0.05)
        t.init_weights(2)
        return t
    a = make()
    a.run(1, 10)
    wa, aa = a.get_blob(with_accum=True)
    a.close()
    b = make()
    b.run(1, 4)
    wb, ab = b.get_blob(with_accum=True)
    b.close()
    c = _trainer(pkg, ctx, 16, dropout=True, seed=11, decay_steps=3, lr=0.05)
    c.set_blob(wb, ab)
    c.run(5, 6)
    wc, ac = c.get_blob(with_accum=True)
    c.close()
    assert np.array_equal(wa.view(np.uint32), wc.view(np.uint32)) and np.array_equal(aa.view(np.uint32), ac.view(np.uint32))
    d = make()
    d.run(1, 10)
    assert np.array_equal(d.get_blob().view(np.uint32), wa.view(np.uint32))
    d.close()
    # explicit steps across the boundary follow the restatement's schedule: lr 0.05, 0.05, then 0.05 * 0.3163
    t = _trainer(pkg, ctx, 8, decay_steps=3, lr=0.05)
    t.init_weights(2)
    w, acc = t.get_blob().astype(np.float64), np.zeros(R.FLOATS)
    rng = np.random.default_rng(4)
    for step in range(1, 5):
        idx = rng.integers(0, NREC, 8)
        vec, lab, qps, gop = R.parse_samples(DATA, idx)
        _, g, _ = R.loss_and_grad(w, vec, lab, qps, gop)
        w, acc = R.train_step(w, acc, g, R.lr_at(step, 0.05, 0.3163, 3))
        t.step_indices(step, idx)
    got = t.get_blob()
    t.close()
    assert R.lr_at(3, 0.05, 0.3163, 3) == 0.05 * 0.3163
    for n, (off, cnt) in R.OFFS.items():
        assert np.abs(got[off: off + cnt] - w[off: off + cnt]).max() <= 2e-5 * max(1.0, np.abs(w[off: off + cnt]).max()), n


def test_evaluation_is_one_batch_and_leaves_the_weights(pkg, ctx):
    t = _trainer(pkg, ctx, 8, qp_scale=0.18)
    t.set_qps([27, 37])
    keep = pkg.ethcnn.lstm_select_qp(VALID, [27, 37])
    assert t.set_samples(1, VALID) == len(keep) and 200 < len(keep) < 500
    t.set_blob(pkg.ethcnn.read_ckpt_lstm_blob(LSTM32))
    w0 = t.get_blob()
    idx = np.random.default_rng(3).integers(0, len(keep), 600)  # three pieces of 256, 256 and 88 samples
    l3, a3, probs = t.evaluate(1, idx=idx, want_probs=True)
    raw = np.frombuffer(VALID, np.uint8).reshape(-1, R.REC)[keep].tobytes()
    vec, lab, qps, gop = R.parse_samples(raw, idx)
    assert set(np.unique(qps)) == {27.0, 37.0}
    import torch
    ref = R.net(torch.tensor(w0.astype(np.float64)), vec, lab, qps, gop, qp_scale=0.18)
    print("eval loss", l3, ref["loss_list"].numpy(), "probs", np.abs(probs - ref["probs"].numpy()).max())
    np.testing.assert_allclose(probs, ref["probs"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(l3, ref["loss_list"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(a3, ref["accuracy_list"].numpy(), rtol=0, atol=1e-5)
    H = t.debug_fetch(pkg.ethcnn.LDBG_STATE_H).reshape(-1, 448)  # the last piece: samples 512 .. 599
    np.testing.assert_allclose(H, ref["H"].numpy()[512 * 20:], rtol=0, atol=1e-5)
    assert np.array_equal(t.get_blob().view(np.uint32), w0.view(np.uint32))
    t.close()


def test_learning_on_learnable_labels(pkg, ctx):
    def curve():
        t = _trainer(pkg, ctx, 64, dropout=True, seed=3, lr=0.1)
        t.init_weights(1)
        l0, _ = t.evaluate(0, n=NREC)
        t.run(1, 150)
        l1, _ = t.evaluate(0, n=NREC)
        t.close()
        return l0, l1
    l0, l1 = curve()
    print("loss before", l0, "after 150 steps", l1)
    assert np.isfinite(l1).all() and (l1 < l0).all()
    m0, m1 = curve()
    assert np.array_equal(l1, m1) and np.array_equal(l0, m0)


def test_bad_arguments_and_malformed_samples(pkg, ctx):
    E = pkg.EthCnnError
    with pytest.raises(E):
        pkg.LstmTrainer(ctx, batch=0)
    with pytest.raises(E):
        pkg.LstmTrainer(ctx, batch=8, qp_scale=-1.0)
    t = pkg.LstmTrainer(ctx, batch=8)
    with pytest.raises(E):
        t.run(1, 1)  # no samples yet
    with pytest.raises(E) as e:
        t.set_samples(0, DATA[:-1])
    assert e.value.code == -3  # ETHCNN_ERR_FORMAT
    raw = np.frombuffer(DATA, np.uint8).reshape(-1, R.REC)[:20].copy()
    f = raw[:, 64:].view(np.float32).reshape(20, 20, 465)
    for (s, p, c, v) in ((3, 2, 5, 4.0), (7, 0, 0, 52.0), (9, 19, 400, np.nan), (11, 4, 1, 0.5)):
        bad = raw.copy()
        bad[:, 64:].view(np.float32).reshape(20, 20, 465)[s, p, c] = v
        with pytest.raises(E) as e:
            t.set_samples(0, bad)
        assert e.value.code == -3 and ("sample %d" % s) in str(e.value)
    t.set_qps([5])
    with pytest.raises(E):
        t.set_samples(0, raw)  # nothing selected
    t.set_qps([])
    assert t.set_samples(0, raw) == 20 and f.shape
    with pytest.raises(E):
        t.step_indices(1, np.arange(7))
    with pytest.raises(E):
        t.step_indices(1, np.full(8, 20))
    with pytest.raises(E):
        t.evaluate(1, n=4)
    with pytest.raises((E, KeyError)):
        t.debug_fetch(99)
    t.init_weights(1)
    l3, _ = t.step_indices(1, np.arange(8))  # still usable
    assert np.isfinite(l3).all()
    t.close()
