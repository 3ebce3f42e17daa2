"""CPU: proof that the assertions of tests/test_gpu_train_edge_values.py bite.  The very functions that file calls
(tests/train_edge_values.py: table_checks, nan_checks, the preconditions) are run
  on the float32 restatement: every check passes and the worst error is at most 1/10 of its tolerance (one exception, below);
  on every mutant a case lists: at least one check fails by a factor of 10 or more, as not finite, or as an exact check;
  on every mutant a case does not list: nothing moves.
Run with -s to print the figures again.

MEASURED (worst error / tolerance).
Logit tables, ETH-CNN batch of 7 and ETH-LSTM batch of 7 (140 rows); sets A .. D of train_edge_values.table_sets():
  the float32 restatement: 0.004 .. 0.012 on losses, accuracies and gradients.  Its P is torch.sigmoid, whose exp is torch's own and
      not the correctly rounded one of the literal formula: it is 0 or 1 ulp from the literal p (1 ulp in set D), so the check
      "P within 1 ulp" is at 0 or at 1.0 of its bound.  That check counts whole ulps and cannot have a margin of 10; it is the one
      check held to <= 1 and not to <= 0.1 here.
  k (e^z / (1 + e^z))   inf: NaN at z >= 88.73, and P != 1.0f                 every set
  m (flush)              inf: P is 0 where the literal value is subnormal       sets A, B, D (C holds no subnormal p)
  n (log1p)              inf: a loss is +Inf                                    every set
  o (no eps)             inf: a loss is NaN                                     every set
  p (1 - (p - eps))      inf: a loss is +Inf                                    every set
  q (closed form)        9.1e5 .. 4.2e6 on an FC3 bias column with z >= 16.65   every set
  r (1 - p in float64)   KNOWN GAP, NOT rejected: 0 .. 7.9e-4.  p is a float32, so 1 - p is exact in float64 and, for p >= 0.5,
      in float32 too (Sterbenz); below 0.5 float32 rounds 1 - p by 6e-8 relative, a thousandth of the gradient tolerance.  The
      mutant matters only when p itself is kept in float64, which is mutant q's territory.
  Large losses: the float32 restatement's loss against literal_loss on the same P differs by at most 9.54e-7 (ETH-LSTM, 320 rows,
      a loss of 13.19: one float32 ulp; 0 .. 4.8e-7 in the other runs) over all table runs of this file, so LARGE_LOSS_TOL =
      9.6e-6.  (On the GPU the kernels end at 0 .. 1.9e-6 of literal_loss, 0.2 of that tolerance.)
The non-finite table (+-Inf, NaN in head 16 only): the float32 restatement 0.011; l (clamped argument) inf: P finite where the
  logit is NaN; u (NaN counted as correct) 2.2e4 on the accuracy of level 16.
Non-finite weights, ETH-LSTM batch of 4, against the float32 restatement (the float64 one stands in for the kernels):
  NaN j-gate bias: float64 0.079 (C); s (NaN cell kept) inf: NaN pattern of the probabilities; t (NaN norm, scale 1) inf: NaN
      pattern of the accumulators; u moves nothing (no probability is NaN)
  NaN o-gate bias: float64 0.027 (C; NaN reaches h, so every later cell is NaN and becomes -5); s inf: NaN pattern of C; u 1e5 on
      the accuracies (0, not 1); t moves nothing (every gradient is NaN, whatever the scale)
Non-finite weights, ETH-CNN batch of 7: NaN FC3 bias of head 16 and a +Inf conv1 weight: float64 against float32 <= 0.1 (printed).
"""
import numpy as np
import pytest
import torch

import train_edge_values as V
import train_edges as E
import train_ref
import train_ref_lstm as R

TABLE_MUTANTS = {"A": "kmnopq", "B": "kmnopq", "C": "knopq", "D": "kmnopq"}   # r: the known gap
FORMULA_LETTERS = "kmnopqr"


def test_table_preconditions():
    V.assert_table_preconditions(verbose=True)
    tabs = V.table_sets()
    assert sorted(np.concatenate(list(tabs.values())[:2]).tolist()) == sorted(V.table_values())
    V.assert_label_preconditions(V.cnn_depths(E.edge_records("ai"), V.CNN_IDX7, V.CNN_QPS7))
    idx, data = V.cnn_eval_263()
    V.assert_label_preconditions(V.cnn_depths(data, idx[256:], E.EVAL_QP))     # the second iteration has every class too
    V.assert_label_preconditions(V.lstm_depths(E.LSTM_IDX7))
    V.assert_label_preconditions(V.lstm_depths(E.LSTM_IDX16)[256:])


def test_thresholds_of_the_float32_sigmoid():
    """the band and thresholds the module states, in numpy's, torch's and the literal arithmetic"""
    for sig in (V.sigmoid_literal, lambda z: torch.sigmoid(torch.tensor(z)).numpy(), lambda z: (V.ONE / (V.ONE + np.exp(-z))).astype(V.F32)):
        with np.errstate(all="ignore"):
            p = sig(np.array([16.62, 16.65, -87.33, -87.35, -88.72, -88.73, 88.73, 104.0, np.inf, -np.inf, np.nan], V.F32))
        tiny = np.finfo(V.F32).tiny
        assert p[0] < 1 and p[1] == 1 and p[2] >= tiny and 0 < p[3] < tiny and 0 < p[4] < tiny and p[5] == 0
        assert p[6] == 1 and p[7] == 1 and p[8] == 1 and p[9] == 0 and np.isnan(p[10])
    # one ulp of p in the band moves the loss term by what the module says
    for z, lo, hi in ((9.7, 5e-4, 2e-3), (12.0, 5e-3, 2e-2), (15.0, 0.1, 0.2), (16.0, 0.3, 0.5)):
        p = V.sigmoid_literal(V.F32(z))
        q = np.nextafter(p, V.F32(0), dtype=V.F32)
        step = abs(float(V._log_neg(p)) - float(V._log_neg(q)))
        assert lo < step < hi, (z, step)


def _cnn_run(tab, dtype):
    data = E.edge_records("ai")
    luma, lab = train_ref.parse_records(data, V.CNN_IDX7, V.CNN_QPS7)
    with np.errstate(all="ignore"):
        out, g = train_ref.loss_and_grad(V.table_blob("cnn", tab), luma, lab, V.CNN_QPS7, dtype=dtype)
    return {"probs": out["probs"], "loss": out["loss_list"], "acc": out["accuracy_list"], "grads": g, "eval_probs": out["probs"],
            "eval_loss": out["loss_list"], "eval_acc": out["accuracy_list"], "total": out["total_loss"]}


def _lstm_run(tab, idx, dtype):
    vec, lab, qps, gop = R.parse_samples(V.lstm_data(), idx)
    with np.errstate(all="ignore"):
        out, g, norm = R.loss_and_grad(V.table_blob("lstm", tab), vec, lab, qps, gop, dtype=dtype)
    return {"probs": out["probs"], "loss": out["loss_list"], "acc": out["accuracy_list"], "grads": g, "eval_probs": out["probs"],
            "eval_loss": out["loss_list"], "eval_acc": out["accuracy_list"], "total": out["total_loss"]}


def _large_loss_gap(got, depths):
    lit = V.literal_loss(got["probs"], depths)["loss"]
    big = lit >= V.ORDINARY_LOSS
    return float(np.abs(np.asarray(got["loss"], np.float64) - lit)[big].max()) if big.any() else 0.0


def _judge_table(kind, name, tab, got32, depths, x3):
    ck = V.table_checks(kind, tab, got32, depths, x3, depths)
    ulp = [c for c in ck if c[0].startswith("P within 1 ulp")]
    rest = V.Checks([c for c in ck if not c[0].startswith("P within 1 ulp")])
    worst, where = rest.worst()
    print("%s table %s: float32 restatement %.3g of the tolerance (%s); P %g ulp from the literal; large-loss gap %.3g" % (
        kind, name, worst, where, ulp[0][1], _large_loss_gap(got32, depths)))
    ck.assert_ok(verbose=False)
    assert worst <= 0.1
    assert _large_loss_gap(got32, depths) <= 0.1 * V.LARGE_LOSS_TOL
    for m in FORMULA_LETTERS:
        worst, where = V.table_checks(kind, tab, V.simulate(kind, tab, depths, x3, m, depths), depths, x3, depths).worst()
        print("%s table %s: mutant %s %.3g x the tolerance (%s)" % (kind, name, m, worst, where))
        if m in TABLE_MUTANTS[name]:
            assert worst >= 10.0, (name, m, worst)
        elif m == "r":
            assert worst < 0.01      # the known gap: stated in the docstring
        else:
            assert worst <= 1e-6, (name, m, worst)
    # the literal formulas themselves pass with nothing to spare needed
    assert V.table_checks(kind, tab, V.simulate(kind, tab, depths, x3, None, depths), depths, x3, depths).worst()[0] <= 1e-6


@pytest.mark.parametrize("name", list(V.table_sets()))
def test_cnn_table_assertions_bite(name):
    tab = V.table_sets()[name]
    depths = V.cnn_depths(E.edge_records("ai"), V.CNN_IDX7, V.CNN_QPS7)
    _judge_table("cnn", name, tab, _cnn_run(tab, torch.float32), depths, V.cnn_x3())


@pytest.mark.parametrize("name", ["A", "B"])
def test_lstm_table_assertions_bite(name):
    tab = V.table_sets()[name]
    idx = E.LSTM_IDX7
    _judge_table("lstm", name, tab, _lstm_run(tab, idx, torch.float32), V.lstm_depths(idx), V.lstm_x3(tuple(idx)))


def test_lstm_table_at_320_rows_large_loss_gap():
    """the batch of 16 (rows from 256 on are a thread's second iteration of the loss loop): the restatement's float32 sums are
    longest here, so this is where LARGE_LOSS_TOL is measured"""
    idx = E.LSTM_IDX16
    depths = V.lstm_depths(idx)
    for name in ("C", "D"):
        tab = V.table_sets()[name]
        got = _lstm_run(tab, idx, torch.float32)
        gap = _large_loss_gap(got, depths)
        print("lstm table %s, 320 rows: losses %s, large-loss gap %.3g (tolerance %.3g)" % (name, got["loss"], gap, V.LARGE_LOSS_TOL))
        assert gap <= 0.1 * V.LARGE_LOSS_TOL
        V.table_checks("lstm", tab, got, depths, V.lstm_x3(tuple(idx)), depths).assert_ok(verbose=False)


def test_nonfinite_table_assertions_bite():
    tab = V.nonfinite_table()
    depths = V.cnn_depths(E.edge_records("ai"), V.CNN_IDX7, V.CNN_QPS7)
    x3 = V.cnn_x3()
    got = _cnn_run(tab, torch.float32)
    assert np.isfinite(got["loss"][:2]).all() and np.isnan(got["loss"][2]) and np.isfinite(got["acc"]).all()
    ck = V.table_checks("cnn", tab, got, depths, x3, depths)
    rest = V.Checks([c for c in ck if not c[0].startswith("P within 1 ulp")])
    print("non-finite table: float32 restatement %.3g of the tolerance (%s)" % rest.worst())
    ck.assert_ok(verbose=False)
    assert rest.worst()[0] <= 0.1
    # the gradient pattern the rules give: heads 64 and 32 keep finite FC tensors, everything fed by head 16's FC2 is NaN
    g = got["grads"]
    for tname, (off, n) in E.CNN_OFFS.items():
        part = g[off: off + n]
        if tname.startswith("h_fc") and ("__64__" in tname or "__32__" in tname) or tname.startswith("y_conv_flat__64") or tname.startswith("y_conv_flat__32"):
            assert np.isfinite(part).all(), tname
        elif tname.startswith("y_conv_flat__16"):
            assert np.isnan(part).any() and np.isfinite(part).any(), tname
        else:
            assert np.isnan(part).all(), tname
    for m in "lu":
        worst, where = V.table_checks("cnn", tab, V.simulate("cnn", tab, depths, x3, m, depths), depths, x3, depths).worst()
        print("non-finite table: mutant %s %.3g x the tolerance (%s)" % (m, worst, where))
        assert worst >= 10.0


def test_literal_evaluator_is_pinned_to_the_restatements():
    """unsaturated data: train_ref.net in float32 (and float64); logits <= 0 of any magnitude: float64"""
    data, idx, qps, blob = E.cnn_case("ai", "random")
    luma, lab = train_ref.parse_records(data, idx, qps)
    for dtype, tol in ((torch.float32, 1e-6), (torch.float64, 1e-6)):
        out, g = train_ref.loss_and_grad(blob, luma, lab, qps, dtype=dtype)
        lit = V.literal_loss(out["probs"], lab)
        assert np.abs(out["loss_list"] - lit["loss"]).max() < tol and np.abs(out["accuracy_list"] - lit["acc"]).max() < 1e-6
        assert abs(float(out["total_loss"]) - float(lit["total"])) < 3 * tol
        for (tag, _, _, _), sl in zip(train_ref.HEADS, V.LEVEL_COLS):
            off, n = E.CNN_OFFS["y_conv_flat__%s__b" % tag]
            ref = g[off: off + n]
            assert np.abs(lit["dZ"][:, sl].astype(np.float64).sum(0) - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-8
    neg = np.array([z for z in V.table_values() if z <= 0], V.F32)
    for k in range(2):     # 21 of the values <= 0 at a time, float64 restatement against the float32 literal contract
        tab = np.roll(neg, 7 * k)[:21]
        depths = V.cnn_depths(E.edge_records("ai"), V.CNN_IDX7, V.CNN_QPS7)
        got = _cnn_run(tab, torch.float64)
        lit = V.literal_loss(V.sigmoid_literal(np.broadcast_to(tab, (7, 21))), depths)
        print("z <= 0, float64 against the literal float32 contract: loss %s / %s" % (got["loss"], lit["loss"]))
        assert np.abs(got["loss"] - lit["loss"]).max() <= V.LARGE_LOSS_TOL and abs(float(got["total"]) - float(lit["total"])) <= 3 * V.LARGE_LOSS_TOL
        sim = V.simulate("cnn", tab, depths, V.cnn_x3(), None, depths)
        E.close_per_tensor(sim["grads"], got["grads"], E.CNN_OFFS).assert_ok(verbose=False)
    # and where float64 cannot be the contract: z = +20 on a negative label
    tab = np.full(21, 20.0, V.F32)
    got = _cnn_run(tab, torch.float64)
    lit = V.literal_loss(V.sigmoid_literal(np.broadcast_to(tab, (7, 21))), depths)
    assert (lit["loss"] - got["loss"]).min() > 1.0 and not lit["dZ"].any()


# --------------------------------------------------------------------------------------------------- non-finite weights ---
def test_the_cell_clip_of_the_restatement_follows_the_rule():
    c = torch.tensor([np.nan, -7.0, 0.5, 7.0, np.inf, -np.inf], dtype=torch.float64, requires_grad=True)
    out = R._cell_clip(c)
    assert out.tolist() == [-5.0, -5.0, 0.5, 5.0, 5.0, -5.0]
    (out * torch.arange(1.0, 7.0, dtype=torch.float64)).sum().backward()
    assert c.grad.tolist() == [0.0, 0.0, 3.0, 0.0, 0.0, 0.0]
    g = np.array([1.0, np.nan, 3.0])
    assert np.isnan(R.clip_by_global_norm(g)).all()                         # a NaN norm makes the whole update NaN
    assert not np.isnan(V._nan_norm_scale_one(g)[[0, 2]]).any()             # which mutant t does not


def _judge_nan(what, ref32, run, offs, keys, mutants, lr=None):
    got = run(torch.float64, None)
    ck = V.nan_checks(got, ref32, offs, keys, lr)
    worst, where = ck.worst()
    print("%s: the float64 restatement against the float32 one: %.3g of the tolerance (%s)" % (what, worst, where))
    ck.assert_ok(verbose=False)
    assert worst <= 0.1
    for m in "stu":
        worst, where = V.nan_checks(run(torch.float32, m), ref32, offs, keys, lr).worst()
        print("%s: mutant %s %.3g x the tolerance (%s)" % (what, m, worst, where))
        if m in mutants:
            assert worst >= 10.0, (what, m, worst)
        else:
            assert worst == 0.0, (what, m, worst, where)


@pytest.mark.parametrize("gate,mutants", [("j", "st"), ("o", "su")])
def test_lstm_nan_gate_bias_assertions_bite(gate, mutants):
    ref32 = V.lstm_nan_reference(gate)

    def run(dtype, m):
        with V.patched(m):
            return V.lstm_nan_reference(gate, dtype)

    C, H = ref32["C"].reshape(-1, 20, 448), ref32["H"].reshape(-1, 20, 448)
    units = np.concatenate([col + np.array([3, 40]) for _, _, _, _, col in R.CELLS])
    assert not np.isnan(C).any() and np.isnan(ref32["norm"]) and np.isnan(ref32["blob1"]).all() and np.isnan(ref32["accum1"]).all()
    if gate == "j":   # the cell becomes -5 at the first unrolled step (slot 19), h stays finite there: the NaN enters backward only
        assert (C[:, :, units] == -5.0).all() and np.isfinite(ref32["probs"]).all() and np.isfinite(ref32["loss"]).all()
        for name, (off, n) in R.OFFS.items():
            assert np.isnan(ref32["grads"][off: off + n]).any() == ("lstm_cell" in name), name
    else:
        assert np.isnan(H[:, :, units]).all() and np.isnan(ref32["probs"]).all() and np.isnan(ref32["loss"]).all()
        assert (ref32["acc"] == 0).all()          # a NaN probability counts as wrong
    _judge_nan("lstm NaN %s-gate bias" % gate, ref32, run, R.OFFS, V.LSTM_NAN_KEYS, mutants, lr=E.LSTM_LR)


@pytest.mark.parametrize("which", ["b3", "conv"])
def test_cnn_nan_weight_patterns(which):
    ref32 = V.cnn_nan_reference(which)
    ref64 = V.cnn_nan_reference(which, torch.float64)
    ck = V.nan_checks(ref64, ref32, E.CNN_OFFS, V.CNN_NAN_KEYS)
    print("cnn %s: float64 against float32 %.3g of the tolerance (%s)" % ((which,) + ck.worst()))
    ck.assert_ok(verbose=False)
    assert ck.worst()[0] <= 0.1
    g = ref32["grads"]
    if which == "b3":
        assert np.isfinite(ref32["loss"][:2]).all() and np.isnan(ref32["loss"][2]) and np.isfinite(ref32["acc"]).all()
        for tname, (off, n) in E.CNN_OFFS.items():
            own = "__64__" in tname or "__32__" in tname     # the heads' own FC tensors; everything fed by the features' gradient is NaN
            assert np.isfinite(g[off: off + n]).all() == own, tname
    else:
        assert np.isnan(ref32["probs"]).all() and np.isnan(ref32["loss"]).all() and (ref32["acc"] == 0).all()


# ------------------------------------------------------------------------- saturation through the whole backward chain ---
def _two_thread_counts(what, run, checks):
    threads = torch.get_num_threads()
    try:
        for nt in sorted({1, threads}):
            torch.set_num_threads(nt)
            ck = checks(run())
            worst, where = ck.worst()
            print("%s: float32 restatement, %d thread(s): %.3g of the tolerance (%s)" % (what, nt, worst, where))
            ck.assert_ok(verbose=False)
            assert worst <= 0.1, (what, worst, where)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("case", list(V.SHIFT_CASES))
@pytest.mark.parametrize("kind", ["cnn", "lstm"])
def test_shifted_head_assertions_bite(kind, case):
    """MEASURED.  One head shifted by +25 (reference: the float32 restatement on torch's default threads) or by -40 (reference:
    float64).  The float32 restatement on one thread and on the default threads: ETH-CNN 0.012 .. 0.072, ETH-LSTM 0 .. 0.090 (the
    loss of 13.58 of the head at -40: 9e-7, one ulp).  At +25 the float64 restatement is the wrong model and is rejected by the exact
    check (its 1 - p is 1.4e-11, not 0, and the saturated head's FC2 / FC3 gradients are not 0): inf.  At -40 float32 and float64
    agree and no formula of the list changes the result; what is shown there is that the check 'not all 0' rejects a head whose
    gradient was dropped."""
    V.assert_shift_preconditions(case, V.shift_logits(kind, case))
    reff = V.cnn_shift_reference if kind == "cnn" else V.lstm_shift_reference
    ref = reff(case)
    up = V.SHIFT_CASES[case][1] == torch.float32
    what = "%s %s" % (kind, case)
    _two_thread_counts(what, lambda: reff(case, torch.float32), lambda got: V.shift_checks(kind, case, got, ref, lr=E.LSTM_LR))
    for name, idx in V.shift_slices(kind, case):
        print("%s: %-28s max |g_ref| %.3e" % (what, name, np.abs(ref["grads"][idx]).max()))
        assert (np.abs(ref["grads"][idx]).max() == 0) == up
    if up:
        worst, where = V.shift_checks(kind, case, reff(case, torch.float64), ref, lr=E.LSTM_LR).worst()
        print("%s: the float64 restatement %.3g x the tolerance (%s)" % (what, worst, where))
        assert worst >= 10.0
    else:
        got = dict(reff(case, torch.float32))
        got["grads"] = got["grads"].copy()
        got["grads"][V.shift_slices(kind, case)[0][1]] = 0.0
        assert V.shift_checks(kind, case, got, ref, lr=E.LSTM_LR).worst()[0] >= 10.0


# ------------------------------------------------------------------------------------------ ETH-LSTM gates in saturation ---
@pytest.mark.parametrize("gate,amt", V.GATE_CASES)
def test_lstm_saturated_gate_assertions_bite(gate, amt):
    """MEASURED.  One gate kind pushed by +-20 or +-95 on every 8th unit; float64 is the reference.  Exactly saturated gate values in
    the float32 run: 6.25 % at 20 for i, f, o (sigmoid(-20) is 2e-9, not 0), 12.5 % at 95 and for j at both.  The float32
    restatement: 0.057 .. 0.071 (C).  Mutant k (sigmoid as e^z / (1 + e^z), run in float32): inf at 95 for i, f and o (e^z overflows:
    Inf / Inf); at 20 and for the j gate it gives the same floats and nothing of the list applies."""
    V.assert_gate_census(gate, amt, V.GATE_IDX7)
    _, slices = V.gate_case(gate, amt)
    ref = V.lstm_gate_reference(gate, amt)
    what = "lstm gate %s pushed by %g" % (gate, amt)
    _two_thread_counts(what, lambda: V.lstm_gate_reference(gate, amt, torch.float32), lambda got: E.lstm_checks(got, ref, slices, lr=E.LSTM_LR))
    with V.exp_form_sigmoid(), np.errstate(all="ignore"):
        got = V.lstm_gate_reference(gate, amt, torch.float32)
    worst, where = E.lstm_checks(got, ref, slices, lr=E.LSTM_LR).worst()
    print("%s: mutant k %.3g x the tolerance (%s)" % (what, worst, where))
    if amt == 95.0 and gate != "j":
        assert worst >= 10.0
    else:
        assert worst <= 0.2


def test_ldp_table_assertions_accept_the_restatement():
    """the Low-Delay-P residual CNN shares loss_body and the heads kernel: table D on its restatement"""
    import train_ref_ldp
    tab = V.table_sets()["D"]
    data = E.edge_records("ldp")
    luma, lab = train_ref_ldp.parse_records(data, V.CNN_IDX7, V.CNN_QPS7)
    with np.errstate(all="ignore"):
        out, g = train_ref_ldp.loss_and_grad(V.table_blob("cnn", tab, "ldp"), luma, lab, V.CNN_QPS7, dtype=torch.float32)
    got = {"probs": out["probs"], "loss": out["loss_list"], "acc": out["accuracy_list"], "grads": g, "eval_probs": out["probs"],
           "eval_loss": out["loss_list"], "eval_acc": out["accuracy_list"]}
    depths = V.cnn_depths(data, V.CNN_IDX7, V.CNN_QPS7, "ldp")
    V.assert_label_preconditions(depths)
    ck = V.table_checks("cnn", tab, got, depths, V.cnn_x3("ldp"), depths)
    ck.assert_ok(verbose=False)
    assert V.Checks([c for c in ck if not c[0].startswith("P within 1 ulp")]).worst()[0] <= 0.1
