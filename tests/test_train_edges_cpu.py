"""CPU: proof that the assertions of tests/test_gpu_train_edges.py bite.  For every case of that file the very functions it calls
(tests/train_edges.py: lstm_checks, cnn_checks, close_on_slices, the preconditions) are run
  on the float32 restatement: every check passes, and the worst error is at most 1/10 of its tolerance;
  on every mutant the case lists (train_edges.py's table; h is the known gap, below): at least one check fails, by a factor of 10
      or more, or the mutant's result is not finite;
  on every mutant the case does not list: nothing moves by more than a millionth of its tolerance (float64 rounding: 7 + 1e-12 is
      not 7), which is why it is not listed.
The float32 figure depends on the order of the float32 sums, which is the CPU library's choice: every case runs it on one thread and
on the threads torch starts with, and the inputs were chosen (train_edges.py: LSTM_IDX*, HEAD_GAIN) so that the factor of 10 held on
every order that could be tried.

MEASURED (worst error / tolerance; run with -s to print them again).  The float32 column is the range over five runs of this file:
torch 2.10 with its AVX-512, AVX2 and SSE4 (no fused multiply-add) code paths at 8 threads, and the default path at 3 and 16
threads, each with the 1-thread run the test adds.  The mutants run in float64 and do not depend on any of that.
ETH-LSTM, golden QP-32 bundle, push every 8th unit by 3.0: per cell 4.6 .. 4.7 % of all (sample, step, unit) elements above +5 and as
many below -5, the nearest to +-5 at 2.5e-3 (batch7; 5.5e-3 for the dropout batch of 7, 2.5e-3 for the batch of 16).  On the clip
slice max |g_ref| is 3.9e-4 / 1.8e-4 / 2.3e-4 (cells 64 / 32 / 16, batch7), so the slice tolerance is 1.2e-7 .. 1.4e-7.
  case             float32     a (slice)  b                     c (C)    f (norm)  i (weights)  j (accumulators)
  batch7           0.065 (C)   202        inf (C not +-5.0f)    -        4.5e17    6.5e3        286
  batch7-dropout   0.078 (C)   135        inf                   1.5e4    4.3e17    6.5e3        258
  batch16          0.078 (C)   201        inf                   1.5e4    8.9e17    6.5e3        288
  batch16-dropout  0.078 (C)   197        inf                   1.5e4    1.0e18    6.5e3        288
  The float32 C is the one figure near the limit, and by nature: a pushed unit climbs through [2, 5) for four steps at 2.4e-7 and
  4.8e-7 an ulp.  With samples drawn without looking (default_rng(7), (16)) it is 0.075 .. 0.126, and 0.129 without fused
  multiply-add: hence the chosen samples.  Mutant (c) changes nothing in a batch where no unit leaves saturation (batch7) and is
  not listed there.  Mutant (a) against the per-tensor rule alone: 1.97 (no margin); against the slices: 202.  Mutants d, e, g
  move nothing in these cases (no pre-activation at 0, integer labels, no empty class).  Mutant (h), (c) in the backward pass
  alone, is NOT rejected: 0.37 of the slice tolerance (test_known_gap_... below says why).
ETH-CNN, synth_blob(3, gain 3.0 / 1.5), both nets (All-Intra / Low-Delay-P):
  case      float32                          d              e                f                  g
  all0      0.016 .. 0.032 / 0.010 .. 0.032  -              -                3.6e17 / 2.9e17    NaN
  all1      0.016 .. 0.026 / 0.014 .. 0.033  -              -                -                  NaN
  all3      0.015 .. 0.038 / 0.010 .. 0.022  -              -                -                  NaN
  random    0.017 .. 0.040 / 0.014 .. 0.037  -              3.6e4 / 3.0e4    -                  -
  mixed16   0.017 .. 0.023 / 0.016 .. 0.022  -              1.1e4 / 1.1e4    8.2e4 / 1.1e5      -
  single    0.032 .. 0.033 / 0.005 .. 0.012  -              5.4e4 / 3.5e4    -                  NaN
  zero      0.013 .. 0.016 / 0.011 .. 0.016  1.4e4 / 1.7e4  -                2.5e17 / 1.5e18    -
  (f is listed wherever a batch holds a CTU with y64 = 0: its negative count at level 64 loses that CTU, and is 0 where no y64 is
  fractional, hence the 1e17.  d's figure is on a conv bias, one of the zero case's slices.  At head gain 3 the Low-Delay-P cases
  reached 0.14 on the evaluation's probabilities without fused multiply-add.)
"""
import functools

import numpy as np
import pytest
import torch

import train_data_lstm
import train_edges as E
import train_ref_lstm as R

ALL = "abcdefgij"   # (h is the known gap: its own test below)


@functools.lru_cache(maxsize=None)
def _lstm_inputs():
    blob, bias_idx, kern_cols = E.push_lstm_biases(E.golden_lstm_blob())
    return train_data_lstm.make_samples(300, seed=21), blob, E.lstm_clip_slices(bias_idx, kern_cols)


def _judge(what, mutants, run, checks):
    """run(dtype) -> the restatement's result under the mutant in force; checks(got) -> Checks against the float64 reference"""
    threads = torch.get_num_threads()
    try:  # two orders of the float32 sums: one thread, and the threads torch starts with
        for nt in sorted({1, threads}):
            torch.set_num_threads(nt)
            ck = checks(run(torch.float32))
            worst, where = ck.worst()
            print("%-24s float32 restatement, %d thread(s): %.3f of the tolerance (%s)" % (what, nt, worst, where))
            ck.assert_ok(verbose=False)
            assert worst <= 0.1, "%s: the float32 restatement uses %.3f of the tolerance of %s" % (what, worst, where)
    finally:
        torch.set_num_threads(threads)
    for m in ALL:
        with E.mutant(m):
            ck = checks(run(torch.float64))
        worst, where = ck.worst()
        if m in mutants:
            print("%-24s mutant %s: %s x the tolerance (%s)%s" % (what, m, "%.3g" % worst, where, "" if ck.finite() else ", not finite"))
            assert worst >= 10.0, "%s: mutant %s stays within %.3g of the tolerance" % (what, m, worst)
            with pytest.raises(AssertionError):
                ck.assert_ok(verbose=False)
        else:
            assert worst <= 1e-6, "%s: mutant %s changes the result (%s by %.3g of its tolerance) and must be listed" % (what, m, where, worst)


def test_mutants_restore_the_restatement():
    import train_ref
    import train_ref_ldp
    before = (R._forget, R._cell_clip, R._carry, train_ref._lrelu, train_ref_ldp._lrelu, train_ref.split_labels, train_ref._counts64, train_ref._denom)
    for m in ALL + "h":
        with pytest.raises(ZeroDivisionError):
            with E.mutant(m):
                1 / 0
    assert before == (R._forget, R._cell_clip, R._carry, train_ref._lrelu, train_ref_ldp._lrelu, train_ref.split_labels, train_ref._counts64,
                      train_ref._denom)
    assert sorted(E.MUTANTS) == sorted(ALL + "h")


def test_push_and_census():
    blob = E.golden_lstm_blob()
    pushed, bias_idx, kern_cols = E.push_lstm_biases(blob, every=8, amt=3.0)
    changed = np.flatnonzero(pushed != blob)
    assert np.array_equal(changed, np.sort(np.concatenate(list(bias_idx.values()))))
    for tag, hid, _, _, _ in R.CELLS:
        off, _ = R.OFFS["RNN%s/multi_rnn_cell/cell_0/lstm_cell/bias" % tag]
        d = (pushed.astype(np.float64) - blob)[off: off + 4 * hid].reshape(4, hid)
        assert np.allclose(d[0, ::8], 3.0, atol=1e-6) and np.allclose(d[2, ::8], 3.0, atol=1e-6) and not d[3].any()
        assert np.allclose(d[1, ::16], 3.0, atol=1e-6) and np.allclose(d[1, 8::16], -3.0, atol=1e-6)
        assert np.array_equal(kern_cols[tag], bias_idx[tag] - off) and kern_cols[tag].size == 3 * hid // 8
    # the plain bundle clips nothing, which is why the push is needed
    data = _lstm_inputs()[0]
    vec = R.parse_samples(data, E.LSTM_IDX7)[0]
    for tag, (hi, lo, _) in E.clip_census(blob, vec).items():
        assert hi == 0 and lo == 0, tag


@pytest.mark.parametrize("case", list(E.LSTM_CASES))
def test_lstm_clip_assertions_bite(case):
    idx, dropout, mutants = E.LSTM_CASES[case]
    data, blob, slices = _lstm_inputs()
    census = E.clip_census(blob, R.parse_samples(data, idx)[0])
    E.assert_clip_preconditions(census)
    masks = R.dropout_masks(E.LSTM_SEED, E.LSTM_STEP, 20 * len(idx)) if dropout else (None, None)

    def run(dtype):
        return E.lstm_reference(blob, data, idx, masks=masks, dtype=dtype, lr=E.LSTM_LR)

    ref = run(torch.float64)
    assert ("c" in mutants) == (E.units_leaving_saturation(ref["Cpre"], len(idx)) > 0)
    for name, sl in slices:
        print("%-44s max |g_ref| %.3e" % (name, np.abs(ref["grads"][sl]).max()))
    _judge("lstm " + case, mutants, run, lambda got: E.lstm_checks(got, ref, slices, lr=E.LSTM_LR))


def test_the_per_tensor_rule_alone_has_no_margin_on_the_straight_through_clamp():
    """why the slice rule exists: against mutant (a) the per-tensor rule ends between 1 and 2 times its tolerance (the tensor's
    maximum comes from units that do not clip), the slice rule above 100 times"""
    idx, _, _ = E.LSTM_CASES["batch7"]
    data, blob, slices = _lstm_inputs()
    ref = E.lstm_reference(blob, data, idx)
    with E.mutant("a"):
        got = E.lstm_reference(blob, data, idx)
    per_tensor = E.close_per_tensor(got["grads"], ref["grads"], R.OFFS).worst()
    on_slices = E.close_on_slices(got["grads"], ref["grads"], slices).worst()
    print("mutant a: per tensor %.3g x (%s), on the slices %.3g x (%s)" % (per_tensor + on_slices))
    assert per_tensor[0] < 3.0 and on_slices[0] > 100.0


def test_known_gap_a_backward_only_c_prev_error_is_not_seen_on_these_inputs():
    """What the pushed biases do NOT show.  Mutant (h) is (c) in the backward pass alone: the forget gate's gradient multiplies the
    c_prev from before the clamp while the forward pass is right.  It matters only where a unit leaves saturation (five
    (sample, step, unit) elements of the batch of 16), and there the forget gate is itself saturated (f (1 - f) = 0.02) and c_prev
    was only just clipped, so the gradient moves by 0.37 of the slice tolerance: under every check.  Seeing it needs
    vectors that drive a unit in and out of the clip from step to step, which these samples do not do.  This test states the
    measured figure; when inputs are found that reject (h), list it in the cases and drop this test."""
    idx, dropout, _ = E.LSTM_CASES["batch16"]
    data, blob, slices = _lstm_inputs()
    ref = E.lstm_reference(blob, data, idx, lr=E.LSTM_LR)
    assert E.units_leaving_saturation(ref["Cpre"], len(idx)) > 0
    with E.mutant("h"):
        got = E.lstm_reference(blob, data, idx, lr=E.LSTM_LR)
    for key in ("probs", "C", "H", "loss"):
        assert np.array_equal(got[key], ref[key]), key  # the forward pass is untouched
    worst, where = E.lstm_checks(got, ref, slices, lr=E.LSTM_LR).worst()
    print("mutant h: %.3g of the tolerance (%s)" % (worst, where))
    assert 0.01 < worst < 1.0


@pytest.mark.parametrize("net", ["ai", "ldp"])
@pytest.mark.parametrize("case", list(E.CNN_CASES))
def test_cnn_degenerate_batch_assertions_bite(net, case):
    data, idx, qps, blob = E.cnn_case(net, case)
    mutants = E.CNN_CASES[case][2]
    slices = E.zero_case_slices() if case == "zero" else ()

    def run(dtype):
        return E.cnn_reference(net, blob, data, idx, qps, dtype=dtype)

    ref = run(torch.float64)
    E.assert_cnn_preconditions(case, ref)
    print("empty levels", ref["empty"], "loss", ref["loss"], "accuracy", ref["acc"])
    _judge("%s %s" % (net, case), mutants, run, lambda got: E.cnn_checks(got, ref, slices))


@pytest.mark.parametrize("net", ["ai", "ldp"])
def test_the_degenerate_records_are_what_they_claim(net):
    import train_ref
    import train_ref_ldp
    ref = {"ai": train_ref, "ldp": train_ref_ldp}[net]
    data = E.edge_records(net)
    n = len(E.GROUPS) * E.N_EACH
    for qp in E.QPS:
        luma, lab = ref.parse_records(data, np.arange(n), qp)
        g = {name: slice(E.N_EACH * k, E.N_EACH * (k + 1)) for k, name in enumerate(E.GROUPS)}
        assert (lab[g["all0"]] == 0).all() and (lab[g["all1"]] == 1).all() and (lab[g["all3"]] == 3).all()
        assert (luma[g["flat"]] == E.FLAT_VALUE[net]).all() and luma[g["all0"]].std() > 1
        y = torch.as_tensor(lab[g["random"]].astype(np.float64)).reshape(-1, 4, 4, 1)
        y64, y32, _, v32, _ = train_ref.split_labels(y)
        for t in (y64, y32, v32):
            assert ((t > 0) & (t < 1)).any()
    # the flat value preprocesses to exactly 0.0, in float64 and in float32
    for dt in (np.float64, np.float32):
        v = dt(E.FLAT_VALUE[net])
        x = v * dt(train_ref.INV255) if net == "ai" else (v - dt(128)) / dt(255.0) * dt(10)
        assert x == 0
