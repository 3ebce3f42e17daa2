"""GPU: the training kernels at saturated, subnormal and non-finite values.
  Logit tables (every FC3 weight 0, the FC3 biases = the table: each column's logit is exactly its bias) isolate the loss kernel that
      ETH-CNN and ETH-LSTM share: P against the literal float32 sigmoid within 1 ulp, exactly 1.0f / 0.0f where that is, subnormal p
      not flushed; loss_list and accuracy_list against the literal evaluator on the kernels' own P; the FC3 gradients (the one window
      onto dZ3) against the literal dL/dlogit; every other gradient exactly 0; evaluate() bit for bit the same P.
  A table of +-Inf and NaN logits, a 263-sample evaluation and a step at 320 rows carry the same columns into a thread's second
      iteration of the loss loop.
  One head shifted by +25 or -40 on seeded / golden weights carries saturated dZ3 through the whole backward chain and one update
      (float32 reference at z >= 17.5, where the head's gradients are exactly 0; float64 at z <= -17.5).
  One LSTM gate kind at a time pushed by +-20 and +-95 saturates sigmoid and tanh inside the recurrence (float64 reference, slice
      rule on the pushed bias entries and kernel columns, at least 2 % of the gate values exactly 0 or +-1).
  Non-finite weights (a NaN FC3 bias, a +Inf conv weight, a NaN j-gate or o-gate bias) against the float32 restatements: equal NaN
      patterns in probabilities, states, losses, accuracies, gradients, the global norm, weights and accumulators after the update;
      every other value within the ordinary tolerance.
  Groups of two: a member with NaN weights beside a plain member with dropout; each equals its solo trainer bit for bit and nothing
      non-finite reaches the plain one.
Inputs, contract, assertions and tolerances live in tests/train_edge_values.py; tests/test_train_edge_values_cpu.py shows on the CPU
that the assertions accept the float32 restatement and reject every applicable wrong formula.  Tolerances: 1 ulp on P; atol 1e-5 on
accuracies, probabilities, C, H and losses below 2; 9.6e-6 on the larger losses (10 x what the float32 restatement differs from the
literal evaluator on the CPU); 1e-4 max |g_ref| + 1e-7 per FC3 column and per tensor; 1e-5 relative on the norm."""
import functools

import numpy as np
import pytest

import train_edge_values as V
import train_edges as E
import train_ref_lstm as R

pytestmark = pytest.mark.gpu

TABLES = dict(V.table_sets(), nonfinite=V.nonfinite_table())


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_same(got, want, what):
    for key in want:
        assert _bits(got[key], want[key]), "%s: %s differs from the solo trainer's" % (what, key)


def _cnn_trainer(pkg, ctx, data, net="ai", **kw):
    t = pkg.Trainer(ctx, net=net, **kw)
    t.set_samples(0, data)
    if net == "ai":
        t.set_qps(list(E.QPS))
    return t


def _cnn_step(pkg, t, blob, idx, qps):
    T = pkg.ethcnn
    t.set_blob(blob)
    el, ea, ep = t.evaluate(0, E.EVAL_QP, idx=idx, want_probs=True)
    l3, a3 = t.step_indices(1, idx, qps)
    return {"loss": l3, "acc": a3, "probs": t.debug_fetch(T.TDBG_PROBS).reshape(len(idx), 21), "grads": t.debug_fetch(T.TDBG_GRADS),
            "eval_loss": el, "eval_acc": ea, "eval_probs": ep}


def _lstm_step(pkg, t, blob, idx, accum=None):
    L = pkg.ethcnn
    rows = 20 * len(idx)
    t.set_blob(blob, accum)
    el, ea, ep = t.evaluate(0, idx=idx, want_probs=True)
    l3, a3 = t.step_indices(E.LSTM_STEP, idx)
    got = {"loss": l3, "acc": a3, "probs": t.debug_fetch(L.LDBG_PROBS).reshape(rows, 21), "grads": t.debug_fetch(L.LDBG_GRADS),
           "C": t.debug_fetch(L.LDBG_STATE_C).reshape(rows, 448), "H": t.debug_fetch(L.LDBG_STATE_H).reshape(rows, 448),
           "norm": float(t.debug_fetch(L.LDBG_NORM)[0]), "eval_loss": el, "eval_acc": ea, "eval_probs": ep}
    got["blob1"], got["accum1"] = t.get_blob(with_accum=True)
    return got


# ------------------------------------------------------------------------------------------------------- the logit tables ---
def test_the_inputs_meet_their_preconditions():
    V.assert_table_preconditions()
    V.assert_label_preconditions(V.cnn_depths(E.edge_records("ai"), V.CNN_IDX7, V.CNN_QPS7))
    V.assert_label_preconditions(V.lstm_depths(E.LSTM_IDX7))
    idx, data = V.cnn_eval_263()
    V.assert_label_preconditions(V.cnn_depths(data, idx[256:], E.EVAL_QP))
    V.assert_label_preconditions(V.lstm_depths(E.LSTM_IDX16)[256:])


@pytest.mark.parametrize("name", list(TABLES))
def test_cnn_loss_kernel_on_a_logit_table(pkg, ctx, name):
    data = E.edge_records("ai")
    tab = TABLES[name]
    with _cnn_trainer(pkg, ctx, data, batch=7, dropout=False, seed=5) as t:
        got = _cnn_step(pkg, t, V.table_blob("cnn", tab), V.CNN_IDX7, V.CNN_QPS7)
    print("P", got["probs"][0], "loss", got["loss"], "accuracy", got["acc"])
    V.table_checks("cnn", tab, got, V.cnn_depths(data, V.CNN_IDX7, V.CNN_QPS7), V.cnn_x3(),
                   V.cnn_depths(data, V.CNN_IDX7, E.EVAL_QP)).assert_ok()
    if name == "nonfinite":   # heads 64 and 32 keep finite losses and FC tensors; everything fed by head 16's FC2 is NaN
        assert np.isfinite(got["loss"][:2]).all() and np.isnan(got["loss"][2]) and np.isfinite(got["acc"]).all()
        for tname, (off, n) in E.CNN_OFFS.items():
            part = got["grads"][off: off + n]
            if "__64__" in tname or "__32__" in tname:
                assert np.isfinite(part).all(), tname
            elif not tname.startswith("y_conv_flat__16"):
                assert np.isnan(part).all(), tname


def test_ldp_cnn_loss_kernel_on_a_logit_table(pkg, ctx):
    """the Low-Delay-P residual CNN (the same loss kernel and heads kernel, its own records and preprocessing) on table D"""
    data = E.edge_records("ldp")
    tab = TABLES["D"]
    with _cnn_trainer(pkg, ctx, data, net="ldp", batch=7, dropout=False, seed=5) as t:
        got = _cnn_step(pkg, t, V.table_blob("cnn", tab, "ldp"), V.CNN_IDX7, V.CNN_QPS7)
    V.table_checks("cnn", tab, got, V.cnn_depths(data, V.CNN_IDX7, V.CNN_QPS7, "ldp"), V.cnn_x3("ldp"),
                   V.cnn_depths(data, V.CNN_IDX7, E.EVAL_QP, "ldp")).assert_ok()


@pytest.mark.parametrize("name,batch", [("A", 7), ("B", 7), ("C", 16), ("D", 16), ("nonfinite", 16)])
def test_lstm_loss_kernel_on_a_logit_table(pkg, ctx, name, batch):
    """batch 16: 320 rows, so that rows from 256 on are a thread's second iteration of the loss loop, with the subnormal, overflow,
    +-Inf and NaN columns"""
    tab = TABLES[name]
    idx = E.LSTM_IDX7 if batch == 7 else E.LSTM_IDX16
    with pkg.LstmTrainer(ctx, batch=batch, dropout=False, seed=E.LSTM_SEED, lr=E.LSTM_LR) as t:
        assert t.set_samples(0, V.lstm_data()) == 300
        got = _lstm_step(pkg, t, V.table_blob("lstm", tab), idx)
    print("P", got["probs"][0], "loss", got["loss"], "accuracy", got["acc"], "norm", got["norm"])
    depths = V.lstm_depths(idx)
    V.table_checks("lstm", tab, got, depths, V.lstm_x3(tuple(idx)), depths).assert_ok()
    if name == "nonfinite":   # the NaN norm is reported, and the whole update is NaN
        assert np.isnan(got["norm"]) and np.isnan(got["blob1"]).all() and np.isnan(got["accum1"]).all()


def test_cnn_evaluation_of_263_samples_with_saturated_and_nan_columns(pkg, ctx):
    """one evaluation over 263 samples: those from 256 on are a thread's second iteration of the loss loop"""
    idx, data = V.cnn_eval_263()
    with _cnn_trainer(pkg, ctx, data, batch=7, dropout=False, seed=5) as t:
        t.set_blob(V.table_blob("cnn", V.nonfinite_table()))
        el, ea, ep = t.evaluate(0, E.EVAL_QP, idx=idx, want_probs=True)
    print("loss", el, "accuracy", ea)
    lit = np.broadcast_to(V.sigmoid_literal(V.nonfinite_table()), ep.shape)
    ok = ~np.isnan(lit)
    ck = V.Checks().exact("P is NaN exactly where the logit is", int((np.isnan(ep) != np.isnan(lit)).sum()))
    ck.add("P within 1 ulp where the logit is not NaN", V.ulp_distance(np.where(ok, ep, 0), np.where(ok, lit, 0)), 1.0)
    V.loss_stage_checks(ck, "eval_", ep, el, ea, V.cnn_depths(data, idx, E.EVAL_QP)).assert_ok()
    assert np.isfinite(el[:2]).all() and np.isnan(el[2]) and np.isfinite(ea).all()


# ------------------------------------------------------------------------- saturation through the whole backward chain ---
@functools.lru_cache(maxsize=None)
def _shift_ref(kind, case):
    V.assert_shift_preconditions(case, V.shift_logits(kind, case))
    return (V.cnn_shift_reference if kind == "cnn" else V.lstm_shift_reference)(case)


@pytest.mark.parametrize("case", list(V.SHIFT_CASES))
def test_cnn_step_with_a_saturated_head(pkg, ctx, case):
    """seeded weights, the FC3 biases of one head shifted by +25 (reference: the float32 restatement; the head's FC2 / FC3 gradients
    are exactly 0) or by -40 (reference: float64); the other heads ordinary"""
    data = E.edge_records("ai")
    ref = _shift_ref("cnn", case)
    with _cnn_trainer(pkg, ctx, data, batch=7, dropout=False, seed=5) as t:
        got = _cnn_step(pkg, t, V.shifted_blob("cnn", case), V.CNN_IDX7, V.CNN_QPS7)
    print("loss", got["loss"], "accuracy", got["acc"])
    V.shift_checks("cnn", case, got, ref).assert_ok()


@pytest.mark.parametrize("case", list(V.SHIFT_CASES))
def test_lstm_step_and_update_with_a_saturated_head(pkg, ctx, case):
    """the golden bundle with one head shifted; one step of the update (weights and accumulators) included"""
    ref = _shift_ref("lstm", case)
    with pkg.LstmTrainer(ctx, batch=7, dropout=False, seed=E.LSTM_SEED, lr=E.LSTM_LR) as t:
        assert t.set_samples(0, V.lstm_data()) == 300
        got = _lstm_step(pkg, t, V.shifted_blob("lstm", case), E.LSTM_IDX7, E.lstm_accum0())
    print("loss", got["loss"], "accuracy", got["acc"], "norm", got["norm"])
    V.shift_checks("lstm", case, got, ref, lr=E.LSTM_LR).assert_ok()


# ------------------------------------------------------------------------------------------ ETH-LSTM gates in saturation ---
@functools.lru_cache(maxsize=None)
def _gate_ref(gate, amt):
    V.assert_gate_census(gate, amt, V.GATE_IDX7)
    return V.lstm_gate_reference(gate, amt)


@pytest.mark.parametrize("gate,amt", V.GATE_CASES)
def test_lstm_step_and_update_with_saturated_gates(pkg, ctx, gate, amt):
    """one gate kind pushed by +-20 or +-95 on every 8th unit, so that sigmoid and tanh inside the recurrence return exactly 0 and
    +-1; float64 is the reference, with the slice rule on the pushed bias entries and kernel columns"""
    ref = _gate_ref(gate, amt)
    blob, slices = V.gate_case(gate, amt)
    with pkg.LstmTrainer(ctx, batch=7, dropout=False, seed=E.LSTM_SEED, lr=E.LSTM_LR) as t:
        assert t.set_samples(0, V.lstm_data()) == 300
        got = _lstm_step(pkg, t, blob, V.GATE_IDX7, E.lstm_accum0())
    print("loss", got["loss"], "accuracy", got["acc"], "norm", got["norm"])
    E.lstm_checks(got, ref, slices, lr=E.LSTM_LR).assert_ok()


# --------------------------------------------------------------------------------------------------- non-finite weights ---
@functools.lru_cache(maxsize=None)
def _lstm_nan_ref(gate):
    return V.lstm_nan_reference(gate)


@pytest.mark.parametrize("gate", ["j", "o"])
def test_lstm_step_and_update_with_a_nan_gate_bias(pkg, ctx, gate):
    """j: the cell becomes -5, the forward pass stays finite, the clipped elements get no gradient, the NaN
    enters through tanh'(j) in the backward pass; o: NaN reaches h, the probabilities and the losses.  Either way the global norm is
    NaN and so is the whole update."""
    ref = _lstm_nan_ref(gate)
    with pkg.LstmTrainer(ctx, batch=len(V.LSTM_NAN_IDX), dropout=False, seed=E.LSTM_SEED, lr=E.LSTM_LR) as t:
        assert t.set_samples(0, V.lstm_data()) == 300
        got = _lstm_step(pkg, t, V.lstm_nan_blob(gate), V.LSTM_NAN_IDX, E.lstm_accum0())
    print("loss", got["loss"], "accuracy", got["acc"], "norm", got["norm"], "NaN gradients", int(np.isnan(got["grads"]).sum()))
    V.nan_checks(got, ref, R.OFFS, V.LSTM_NAN_KEYS, lr=E.LSTM_LR).assert_ok()
    assert np.isnan(got["norm"]) and np.isnan(got["blob1"]).all() and np.isnan(got["accum1"]).all()
    if gate == "j":
        units = np.concatenate([col + np.array([3, 40]) for _, _, _, _, col in R.CELLS])
        assert (got["C"][:, units] == np.float32(-5.0)).all() and np.isfinite(got["probs"]).all()
    else:
        assert (got["acc"] == 0).all() and (got["eval_acc"] == 0).all()      # a NaN probability counts as wrong


@functools.lru_cache(maxsize=None)
def _cnn_nan_ref(which):
    return V.cnn_nan_reference(which)


@pytest.mark.parametrize("which", ["b3", "conv"])
def test_cnn_step_with_a_non_finite_weight(pkg, ctx, which):
    """b3: one NaN FC3 bias in head 16: loss_64 and loss_32 stay finite, heads 64 and 32 keep finite FC gradients, everything fed by
    the features' gradient is NaN.  conv: one +Inf conv1 weight."""
    data = E.edge_records("ai")
    ref = _cnn_nan_ref(which)
    with _cnn_trainer(pkg, ctx, data, batch=7, dropout=False, seed=5) as t:
        got = _cnn_step(pkg, t, V.cnn_nan_blob(which), V.CNN_IDX7, V.CNN_QPS7)
    print("loss", got["loss"], "accuracy", got["acc"], "NaN gradients", int(np.isnan(got["grads"]).sum()))
    V.nan_checks(got, ref, E.CNN_OFFS, V.CNN_NAN_KEYS).assert_ok()
    if which == "b3":
        assert np.isfinite(got["loss"][:2]).all() and np.isnan(got["loss"][2])
        for tname, (off, n) in E.CNN_OFFS.items():
            assert np.isfinite(got["grads"][off: off + n]).all() == ("__64__" in tname or "__32__" in tname), tname


# ---------------------------------------------------------------------------------------------------------------- groups ---
def test_lstm_group_of_a_nan_member_and_a_plain_member(pkg, ctx):
    """K = 2: member 0 has the NaN j-gate bias, member 1 the plain bundle and dropout; each equals its solo trainer bit for bit and
    nothing non-finite reaches member 1"""
    idx = V.LSTM_NAN_IDX
    blobs = [V.lstm_nan_blob("j"), E.golden_lstm_blob()]
    members = [dict(batch=4, seed=E.LSTM_SEED, dropout=False, lr=E.LSTM_LR), dict(batch=4, seed=9, dropout=True, lr=0.1)]
    zeros = np.zeros(R.FLOATS, np.float32)
    L = pkg.ethcnn

    def state(fetch, blob_accum, stats):
        return {"blob": blob_accum[0], "accum": blob_accum[1], "loss": stats[0], "acc": stats[1], "probs": fetch(L.LDBG_PROBS),
                "C": fetch(L.LDBG_STATE_C), "H": fetch(L.LDBG_STATE_H), "grads": fetch(L.LDBG_GRADS), "norm": fetch(L.LDBG_NORM)}

    with pkg.LstmTrainerGroup(ctx, [L.lstm_train_options(**kw) for kw in members]) as g:
        assert g.set_samples(0, V.lstm_data()) == [300, 300]
        for m in range(2):
            g.set_blob(m, blobs[m], zeros)
        l3, a3 = g.step_indices(E.LSTM_STEP, np.stack([idx, idx]).astype(np.int32))
        got = [state(lambda which, m=m: g.debug_fetch(m, which), g.get_blob(m, with_accum=True), (l3[m], a3[m])) for m in range(2)]
    for m, kw in enumerate(members):
        with pkg.LstmTrainer(ctx, **kw) as t:
            t.set_samples(0, V.lstm_data())
            t.set_blob(blobs[m], zeros)
            stats = t.step_indices(E.LSTM_STEP, idx)
            _assert_same(got[m], state(t.debug_fetch, t.get_blob(with_accum=True), stats), "member %d" % m)
    assert np.isnan(got[0]["norm"]).all() and np.isnan(got[0]["blob"]).all()
    assert all(np.isfinite(v).all() for v in got[1].values())


def test_cnn_group_of_a_nan_member_and_a_plain_member(pkg, ctx):
    """K = 2: member 0 on the table of +-Inf and NaN logits, member 1 on seeded weights with dropout"""
    data = E.edge_records("ai")
    idx = np.stack([V.CNN_IDX7, V.CNN_IDX7]).astype(np.int32)
    qps = np.stack([V.CNN_QPS7, V.CNN_QPS7[::-1]]).astype(np.int32)
    blobs = [V.table_blob("cnn", V.nonfinite_table()), E.cnn_case("ai", "random")[3]]
    members = [dict(batch=7, seed=11, dropout=False, net="ai"), dict(batch=7, seed=12, dropout=True, net="ai")]
    T = pkg.ethcnn

    def state(fetch, blob_accum, stats):
        out = {"blob": blob_accum[0], "accum": blob_accum[1], "loss": stats[0], "acc": stats[1]}
        for name, which in (("mask_fc1", T.TDBG_MASK_FC1), ("mask_fc2", T.TDBG_MASK_FC2), ("probs", T.TDBG_PROBS), ("grads", T.TDBG_GRADS)):
            out[name] = fetch(which)
        return out

    with pkg.TrainerGroup(ctx, [T.train_options(**kw) for kw in members]) as g:
        g.set_samples(0, data)
        for m in range(2):
            g.set_qps(m, list(E.QPS))
            g.set_blob(m, blobs[m])
        l3, a3 = g.step_indices(1, idx, qps)
        got = [state(lambda which, m=m: g.debug_fetch(m, which), g.get_blob(m, with_accum=True), (l3[m], a3[m])) for m in range(2)]
    for m, kw in enumerate(members):
        with _cnn_trainer(pkg, ctx, data, **kw) as t:
            t.set_blob(blobs[m])
            stats = t.step_indices(1, idx[m], qps[m])
            _assert_same(got[m], state(t.debug_fetch, t.get_blob(with_accum=True), stats), "member %d" % m)
    assert np.isnan(got[0]["loss"][2]) and np.isnan(got[0]["grads"]).any()
    assert all(np.isfinite(v).all() for v in got[1].values())
