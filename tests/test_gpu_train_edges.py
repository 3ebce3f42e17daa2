"""GPU: the branches of the training kernels that ordinary data does not reach, against the float64 restatements:
  the cell clip of the ETH-LSTM trainer (forward clamp, no gradient where c was clamped, the clipped c carried on), active on 9 % of
      all (sample, step, unit) elements through pushed biases, in the solo trainer, the trainer group and evaluate;
  the zero-count and fractional-label paths of the ETH-CNN loss (whole batches at one depth, depths drawn per 16x16 block, a batch of
      one), both nets;
  the leaky-ReLU slope at exactly 0 (flat records, zero biases), both nets.
Inputs, assertions and tolerances live in tests/train_edges.py; tests/test_train_edges_cpu.py shows on the CPU that each of these
assertions accepts the float32 restatement with a factor of 10 to spare and rejects every applicable wrong restatement by a factor of
10 or more.  Tolerances: atol 1e-5 on losses, accuracies, probabilities, C and H; per tensor 1e-4 max |g_ref| + 1e-7 on gradients and,
with the maximum over the slice only, on the slices a branch governs; 1e-5 relative on the global norm."""
import functools

import numpy as np
import pytest

import train_data_lstm
import train_edges as E
import train_ref_lstm as R

pytestmark = pytest.mark.gpu

LSTM_DATA = train_data_lstm.make_samples(300, seed=21)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_same(got, want, what):
    for key in want:
        assert _bits(got[key], want[key]), "%s: %s differs from the solo trainer's" % (what, key)


# --------------------------------------------------------------------------------------------------- ETH-LSTM: the cell clip ---
@functools.lru_cache(maxsize=None)
def _pushed():
    blob, bias_idx, kern_cols = E.push_lstm_biases(E.golden_lstm_blob())
    return blob, E.lstm_clip_slices(bias_idx, kern_cols)


@functools.lru_cache(maxsize=None)
def _lstm_ref(case):
    """float64, computed once: (reference, dropout masks)"""
    idx, dropout, _ = E.LSTM_CASES[case]
    blob, _ = _pushed()
    E.assert_clip_preconditions(E.clip_census(blob, R.parse_samples(LSTM_DATA, idx)[0]))
    masks = R.dropout_masks(E.LSTM_SEED, E.LSTM_STEP, 20 * len(idx)) if dropout else (None, None)
    return E.lstm_reference(blob, LSTM_DATA, idx, masks=masks, lr=E.LSTM_LR), masks


def _lstm_buffers(pkg, fetch, rows):
    L = pkg.ethcnn
    return {"probs": fetch(L.LDBG_PROBS).reshape(rows, 21), "C": fetch(L.LDBG_STATE_C).reshape(rows, 448),
            "H": fetch(L.LDBG_STATE_H).reshape(rows, 448), "norm": float(fetch(L.LDBG_NORM)[0]), "grads": fetch(L.LDBG_GRADS)}


@pytest.mark.parametrize("case", list(E.LSTM_CASES))
def test_lstm_step_update_and_evaluation_with_the_clip_active(pkg, ctx, case):
    idx, dropout, _ = E.LSTM_CASES[case]
    blob, slices = _pushed()
    ref, masks = _lstm_ref(case)
    rows = 20 * len(idx)
    with pkg.LstmTrainer(ctx, batch=len(idx), dropout=dropout, seed=E.LSTM_SEED, lr=E.LSTM_LR) as t:
        assert t.set_samples(0, LSTM_DATA) == 300
        t.set_blob(blob, E.lstm_accum0())  # non-zero accumulators: the momentum is in the update
        _, _, eval_probs = t.evaluate(0, idx=idx, want_probs=True)
        assert _bits(t.get_blob(), blob)
        l3, a3 = t.step_indices(E.LSTM_STEP, idx)
        got = _lstm_buffers(pkg, t.debug_fetch, rows)
        if dropout:
            assert np.array_equal(t.debug_fetch(pkg.ethcnn.LDBG_MASK_H).reshape(rows, 448), masks[0])
            assert np.array_equal(t.debug_fetch(pkg.ethcnn.LDBG_MASK_FC2).reshape(rows, 336), masks[1])
        got["blob1"], got["accum1"] = t.get_blob(with_accum=True)
    got.update(loss=l3, acc=a3, eval_probs=eval_probs)
    n_hi, n_lo = int((got["C"] == np.float32(5.0)).sum()), int((got["C"] == np.float32(-5.0)).sum())
    print("C holds %d words of +5.0f and %d of -5.0f out of %d" % (n_hi, n_lo, got["C"].size))
    assert n_hi >= 0.02 * got["C"].size and n_lo >= 0.02 * got["C"].size
    E.lstm_checks(got, ref, slices, lr=E.LSTM_LR).assert_ok()


def test_lstm_group_of_a_pushed_and_a_plain_member(pkg, ctx):
    """K = 2 on the batch of 16: member 0 has the pushed bundle, member 1 the plain one and dropout; each equals its solo trainer bit
    for bit, and the pushed member passes the slice check against float64"""
    idx, _, _ = E.LSTM_CASES["batch16"]
    pushed, slices = _pushed()
    ref, _ = _lstm_ref("batch16")
    blobs = [pushed, E.golden_lstm_blob()]
    # (member 1 differs in everything a member may differ in: its bundle, its seed, dropout and the trainer's default rate)
    members = [dict(batch=16, seed=E.LSTM_SEED, dropout=False, lr=E.LSTM_LR), dict(batch=16, seed=9, dropout=True, lr=0.1)]
    zeros = np.zeros(R.FLOATS, np.float32)
    L = pkg.ethcnn

    def state(fetch, blob_accum, stats):
        out = _lstm_buffers(pkg, fetch, 320)
        out.update(blob=blob_accum[0], accum=blob_accum[1], loss=stats[0], acc=stats[1], mask_h=fetch(L.LDBG_MASK_H), mask_fc2=fetch(L.LDBG_MASK_FC2))
        out["norm"] = fetch(L.LDBG_NORM)
        return out

    with pkg.LstmTrainerGroup(ctx, [L.lstm_train_options(**kw) for kw in members]) as g:
        assert g.set_samples(0, LSTM_DATA) == [300, 300]
        for m in range(2):
            g.set_blob(m, blobs[m], zeros)
        l3, a3 = g.step_indices(E.LSTM_STEP, np.stack([idx, idx]).astype(np.int32))
        got = [state(lambda which, m=m: g.debug_fetch(m, which), g.get_blob(m, with_accum=True), (l3[m], a3[m])) for m in range(2)]
    for m, kw in enumerate(members):
        with pkg.LstmTrainer(ctx, **kw) as t:
            t.set_samples(0, LSTM_DATA)
            t.set_blob(blobs[m], zeros)
            stats = t.step_indices(E.LSTM_STEP, idx)
            _assert_same(got[m], state(t.debug_fetch, t.get_blob(with_accum=True), stats), "member %d" % m)
    assert (got[0]["C"] == np.float32(5.0)).mean() >= 0.02 and not (np.abs(got[1]["C"]) == np.float32(5.0)).any()
    ck = E.close_on_slices(got[0]["grads"], ref["grads"], slices)
    E.close_per_tensor(got[0]["grads"], ref["grads"], R.OFFS, checks=ck)
    ck.atol("C", got[0]["C"], ref["C"], 1e-5).assert_ok()


# ----------------------------------------------------------------------------------------------- ETH-CNN: degenerate batches ---
@functools.lru_cache(maxsize=None)
def _cnn_ref(net, case):
    data, idx, qps, blob = E.cnn_case(net, case)
    ref = E.cnn_reference(net, blob, data, idx, qps)
    E.assert_cnn_preconditions(case, ref)
    return ref


def _cnn_trainer(pkg, ctx, net, data, **kw):
    t = pkg.Trainer(ctx, net=net, **kw)
    t.set_samples(0, data)
    if net == "ai":
        t.set_qps(list(E.QPS))
    return t


@pytest.mark.parametrize("net", ["ai", "ldp"])
@pytest.mark.parametrize("case", list(E.CNN_CASES))
def test_cnn_step_and_evaluation_on_a_degenerate_batch(pkg, ctx, net, case):
    data, idx, qps, blob = E.cnn_case(net, case)
    ref = _cnn_ref(net, case)
    print("levels without a valid element:", [E.LEVELS[lv] for lv in range(3) if ref["empty"][lv]], "loss", ref["loss"], "accuracy", ref["acc"])
    T = pkg.ethcnn
    with _cnn_trainer(pkg, ctx, net, data, batch=len(idx), dropout=False, seed=5) as t:
        t.set_blob(blob)
        el, ea, ep = t.evaluate(0, E.EVAL_QP, idx=idx, want_probs=True)
        l3, a3 = t.step_indices(1, idx, qps)
        got = {"loss": l3, "acc": a3, "probs": t.debug_fetch(T.TDBG_PROBS).reshape(len(idx), 21), "grads": t.debug_fetch(T.TDBG_GRADS),
               "eval_loss": el, "eval_acc": ea, "eval_probs": ep}
        h1 = t.debug_fetch(T.TDBG_H1).reshape(len(idx), 448)
    if case == "zero":  # first: the flat samples' FC1 outputs are exactly 0.0, so the slope is taken at exactly 0
        assert not h1[:8].any() and h1[8:].any()
    assert all(np.isfinite(np.asarray(v)).all() for v in got.values())
    E.cnn_checks(got, ref, E.zero_case_slices() if case == "zero" else ()).assert_ok()


@pytest.mark.parametrize("net", ["ai", "ldp"])
def test_cnn_group_on_degenerate_batches(pkg, ctx, net):
    """K = 2, one step: member 0 on the batch whose depths are all 0 (levels 32 and 16 empty), member 1 (dropout) on the batch whose
    depths are all 1; each equals its solo trainer bit for bit"""
    data = E.edge_records(net)
    idx = np.stack([E.CNN_CASES["all0"][0], E.CNN_CASES["all1"][0]]).astype(np.int32)
    qps = np.random.default_rng(2).choice(E.QPS, (2, 7)).astype(np.int32)
    members = [dict(batch=7, seed=11, dropout=False, net=net), dict(batch=7, seed=12, dropout=True, net=net)]
    T = pkg.ethcnn

    def state(fetch, blob_accum, stats):
        out = {"blob": blob_accum[0], "accum": blob_accum[1], "loss": stats[0], "acc": stats[1]}
        for name, which in (("mask_fc1", T.TDBG_MASK_FC1), ("mask_fc2", T.TDBG_MASK_FC2), ("probs", T.TDBG_PROBS), ("grads", T.TDBG_GRADS)):
            out[name] = fetch(which)
        return out

    with pkg.TrainerGroup(ctx, [T.train_options(**kw) for kw in members]) as g:
        g.set_samples(0, data)
        if net == "ai":
            for m in range(2):
                g.set_qps(m, list(E.QPS))
        g.init_weights([1, 2])
        start = [g.get_blob(m) for m in range(2)]
        l3, a3 = g.step_indices(1, idx, qps)
        got = [state(lambda which, m=m: g.debug_fetch(m, which), g.get_blob(m, with_accum=True), (l3[m], a3[m])) for m in range(2)]
    assert l3[0][1] == 0 and l3[0][2] == 0 and l3[1][2] == 0 and np.isfinite(l3).all()
    for m, kw in enumerate(members):
        with _cnn_trainer(pkg, ctx, net, data, **{k: v for k, v in kw.items() if k != "net"}) as t:
            t.set_blob(start[m])
            stats = t.step_indices(1, idx[m], qps[m])
            _assert_same(got[m], state(t.debug_fetch, t.get_blob(with_accum=True), stats), "member %d" % m)
            assert np.isfinite(got[m]["grads"]).all() and np.isfinite(got[m]["blob"]).all()
