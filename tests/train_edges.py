"""TEST INFRASTRUCTURE: the inputs that reach the rarely taken branches of the training kernels, the assertions made on them,
and deliberately wrong restatements ("mutants") that show the assertions bite.  Nothing here is imported by the product.

Branches and what reaches them:
  cell clip of the ETH-LSTM trainer (c clamped to +-5, no gradient where it was clamped, the clipped c carried on):
      push_lstm_biases raises the i / f bias and moves the j bias of every 8th hidden unit, so that those units saturate within a
      few unrolled steps; clip_census says how many (sample, step, unit) elements are clipped on each side and how far from +-5
      the nearest one stays
  zero counts and fractional labels of the balanced loss: labels_all(d) (a whole batch at one depth: empty classes, levels without
      a valid element), labels_random (depths drawn per 16x16 block: fractional y64, y32 and v32)
  leaky-ReLU slope at exactly 0: flat_records (constant luma that preprocesses to exactly 0.0) with every bias zeroed

Checks collects (what, error, tolerance) triples; the GPU tests call assert_ok(), tests/test_train_edges_cpu.py runs the same
functions on the float32 restatement (worst error / tolerance <= 0.1) and on every mutant that applies (>= 10, or not finite).

Mutants patch one function of the restatements (tests/train_ref*.py look these up when called) for the length of a `with`:
  a  LSTM  straight-through clamp: the gradient passes where c was clipped
  b  LSTM  no clamp in the forward pass
  c  LSTM  the next step's c_prev taken before the clamp
  d  both  leaky-ReLU gradient 1.0 at exactly 0
  e  both  labels rounded to 0 / 1 before the loss
  f  both  the level-64 counts multiplied by a validity mask (level 32's formula on the 64x64 average, which equals y64: a CTU
           with y64 = 0 is no longer counted as a negative)
  g  both  the count denominators without their eps: 0 / 0 = NaN where a class is empty
  h  LSTM  (c) in the backward pass only: the forget gate's gradient multiplies c_prev before its clamp, the forward pass is right.
           No case lists it: these inputs move it by a third of the slice tolerance (the known gap stated in the CPU test file)
  i  LSTM  the learning rate of the update decayed once too early (lr x 0.3163 at a step before the first decay)
  j  LSTM  the update without its momentum factor (accum + g in place of 0.9 accum + g)
"""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import train_data
import train_data_ldp
import train_ref
import train_ref_ldp
import train_ref_lstm as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM32 = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
CNN_OFFS = {n: (o // 4, int(np.prod(s))) for n, s, o in train_ref.ethcnn_np.TENSORS}
LEVELS = ("64", "32", "16")


def golden_lstm_blob():
    return np.fromfile(LSTM32 + ".data-00000-of-00001", dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------- checks ---
class Checks(list):
    """(what, error, tolerance) triples.  An error that is not finite fails whatever the tolerance."""

    def add(self, what, err, tol):
        self.append((what, float(err), float(tol)))
        return self

    def atol(self, what, got, ref, tol, forced=0.0):
        """forced: per element, the part of a difference that the number format forces and no arithmetic can avoid"""
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        return self.add(what, np.maximum(np.abs(got - ref) - forced, 0.0).max() if np.isfinite(got).all() else np.nan, tol)

    def exact(self, what, wrong):
        """wrong: the number of elements that are not exactly what they must be"""
        return self.add(what, wrong, 0.0)

    @staticmethod
    def _ratio(err, tol):
        if not np.isfinite(err):
            return np.inf
        return err / tol if tol > 0 else (0.0 if err == 0 else np.inf)

    def worst(self):
        """(largest error / tolerance, its name); inf for a failed exact check or an error that is not finite"""
        r = [self._ratio(e, t) for _, e, t in self]
        k = int(np.argmax(r))
        return r[k], self[k][0]

    def finite(self):
        return all(np.isfinite(e) for _, e, _ in self)

    def assert_ok(self, verbose=True):
        for what, err, tol in self:
            if verbose:
                print("%-58s error %.3e  tolerance %.3e" % (what, err, tol))
        for what, err, tol in self:
            assert np.isfinite(err) and err <= tol, "%s: error %g > tolerance %g" % (what, err, tol)


def close_per_tensor(g, g_ref, offs, rel=1e-4, floor=1e-7, checks=None):
    """the GPU trainer tests' _close: per tensor, max |g - g_ref| <= rel max |g_ref| + floor"""
    ck = Checks() if checks is None else checks
    for name, (off, n) in offs.items():
        a, b = np.asarray(g[off: off + n], np.float64), np.asarray(g_ref[off: off + n], np.float64)
        ck.add("grad " + name, np.abs(a - b).max() if np.isfinite(a).all() else np.nan, rel * np.abs(b).max() + floor)
    return ck


def close_on_slices(g, g_ref, slices, rel=1e-4, floor=1e-7, checks=None):
    """the same rule with the maximum taken over a slice only; slices: (name, flat blob indices) pairs"""
    ck = Checks() if checks is None else checks
    for name, idx in slices:
        a, b = np.asarray(g, np.float64)[idx], np.asarray(g_ref, np.float64)[idx]
        ck.add("slice " + name, np.abs(a - b).max() if np.isfinite(a).all() else np.nan, rel * np.abs(b).max() + floor)
    return ck


# ------------------------------------------------------------------------------------------------------------ mutants ---
class _LreluOneAtZero(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return F.leaky_relu(x, 0.2)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.where(x >= 0, torch.ones_like(x), torch.full_like(x, 0.2))


class _ForgetGradFromUnclippedPrev(torch.autograd.Function):
    """f * c_prev whose gradient to the forget gate uses c_prev before its clip (the forward value is right)"""

    @staticmethod
    def forward(ctx, fg, c_prev, cpre_prev):
        ctx.save_for_backward(fg, cpre_prev)
        return fg * c_prev

    @staticmethod
    def backward(ctx, g):
        fg, cpre_prev = ctx.saved_tensors
        return g * cpre_prev, g * fg, None


def _rounded_labels(split):
    return lambda y: tuple(torch.round(t) for t in split(y))


def _patches(name):
    if name == "a":
        return [(R, "_cell_clip", lambda c: c + (torch.clamp(c, -5.0, 5.0) - c).detach())]
    if name == "b":
        return [(R, "_cell_clip", lambda c: c)]
    if name == "c":
        return [(R, "_carry", lambda cpre, c: cpre)]
    if name == "d":
        return [(train_ref, "_lrelu", _LreluOneAtZero.apply), (train_ref_ldp, "_lrelu", _LreluOneAtZero.apply)]
    if name == "e":
        return [(train_ref, "split_labels", _rounded_labels(train_ref.split_labels))]
    if name == "f":
        return [(train_ref, "_counts64", lambda y64: (train_ref._cnz(y64 * y64), train_ref._cnz((1 - y64) * y64)))]
    if name == "g":
        return [(train_ref, "_denom", lambda count: count)]
    if name == "h":
        return [(R, "_forget", _ForgetGradFromUnclippedPrev.apply)]
    if name == "i":
        return [(R, "lr_at", lambda step, lr_init=0.1, decay_rate=0.3163, decay_steps=25000: lr_init * decay_rate)]
    if name == "j":
        return [(train_ref, "momentum_update", lambda blob, accum, grad, lr, momentum=0.9: (blob - lr * (accum + grad), accum + grad))]
    raise KeyError(name)


MUTANTS = {"a": "lstm", "b": "lstm", "c": "lstm", "d": "both", "e": "both", "f": "both", "g": "both", "h": "lstm", "i": "lstm", "j": "lstm"}


@contextlib.contextmanager
def mutant(name):
    """the restatements with one deliberate error, until the block ends (name None: unchanged)"""
    todo = [] if name is None else _patches(name)
    saved = [(mod, attr, getattr(mod, attr)) for mod, attr, _ in todo]
    try:
        for mod, attr, new in todo:
            setattr(mod, attr, new)
        yield
    finally:
        for mod, attr, old in saved:
            setattr(mod, attr, old)


# ------------------------------------------------------------------------------------------------ ETH-LSTM: the cell clip ---
def push_lstm_biases(blob, every=8, amt=3.0):
    """+amt on the i and f bias of every `every`-th hidden unit of each cell, +amt on the j bias of every second one of those and
    -amt on the others (bias layout [i | j | f | o]).  -> (blob, {cell tag: flat blob indices of those units' i, j, f bias
    entries} = the clip slice, {cell tag: the same gates' columns of the cell's kernel})"""
    out = np.array(blob, dtype=np.float32, copy=True)
    bias_idx, kern_cols = {}, {}
    for tag, hid, _, _, _ in R.CELLS:
        off, n = R.OFFS["RNN%s/multi_rnn_cell/cell_0/lstm_cell/bias" % tag]
        assert n == 4 * hid
        units = np.arange(0, hid, every)
        sign = np.where(np.arange(units.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
        out[off + units] += np.float32(amt)
        out[off + hid + units] += sign * np.float32(amt)
        out[off + 2 * hid + units] += np.float32(amt)
        cols = np.concatenate([units, hid + units, 2 * hid + units])
        bias_idx[tag], kern_cols[tag] = off + cols, cols
    return out, bias_idx, kern_cols


def lstm_clip_slices(bias_idx, kern_cols):
    """-> (name, flat blob indices) pairs for close_on_slices: per cell the clip slice of the bias and, of the kernel, every row of
    the same gates' columns"""
    out = []
    for tag, hid, _, _, _ in R.CELLS:
        out.append(("RNN%s bias [i j f] of the pushed units" % tag, bias_idx[tag]))
        koff, kn = R.OFFS["RNN%s/multi_rnn_cell/cell_0/lstm_cell/kernel" % tag]
        rows = np.arange(kn // (4 * hid))
        out.append(("RNN%s kernel columns of the pushed units" % tag, (koff + rows[:, None] * 4 * hid + kern_cols[tag][None, :]).reshape(-1)))
    return out


def clip_census(blob, vec):
    """float64, per cell tag: (share of (sample, step, unit) elements with cpre > 5, share with cpre < -5, min | |cpre| - 5 |).
    The cell state depends on the vectors and the cell weights alone (dropout acts on the cell's output)."""
    n = np.asarray(vec).shape[0]
    with torch.no_grad():
        cpre = R.net(torch.tensor(np.asarray(blob, dtype=np.float64)), vec, np.zeros((n, 20, 16)), np.zeros((n, 20)),
                     np.zeros((n, 20), np.int64))["Cpre"].numpy()
    out = {}
    for tag, hid, _, _, col in R.CELLS:
        c = cpre[:, col: col + hid]
        out[tag] = (float((c > 5).mean()), float((c < -5).mean()), float(np.abs(np.abs(c) - 5).min()))
    return out


def assert_clip_preconditions(census, share=0.02, margin=1e-3):
    """every cell clips at least `share` of its elements on each side, and no element sits where fp32 rounding could flip the gate"""
    for tag, (hi, lo, m) in census.items():
        print("cell %s: %.2f %% of elements above +5, %.2f %% below -5, nearest to +-5 at %.3e" % (tag, 100 * hi, 100 * lo, m))
        assert hi >= share and lo >= share, "cell %s: clipped shares %.4f / %.4f < %.2f" % (tag, hi, lo, share)
        assert m >= margin, "cell %s: an element %.3e away from the clip" % (tag, m)


def lstm_reference(blob, data, idx, qp_scale=1.0, masks=(None, None), dtype=torch.float64, lr=0.05):
    """the restatement (or, under `with mutant(..)`, a wrong one) in the shape the checks take: probs, C, H, Cpre, loss, acc, grads,
    norm, the dropout-free probabilities an evaluation gives, and weights / accumulators after the update of step LSTM_STEP from the
    accumulators lstm_accum0()"""
    vec, lab, qps, gop = R.parse_samples(data, idx)
    out, g, norm = R.loss_and_grad(blob, vec, lab, qps, gop, qp_scale, masks[0], masks[1], dtype=dtype)
    res = {"probs": out["probs"], "C": out["C"], "H": out["H"], "Cpre": out["Cpre"], "loss": out["loss_list"], "acc": out["accuracy_list"],
           "grads": g, "norm": norm}
    if masks[0] is None:
        res["eval_probs"] = out["probs"]
    else:
        with torch.no_grad():
            res["eval_probs"] = R.net(torch.tensor(np.asarray(blob, dtype=np.float64), dtype=dtype), vec, lab, qps, gop, qp_scale)["probs"].numpy()
    w1, a1 = R.train_step(np.asarray(blob, np.float64), lstm_accum0().astype(np.float64), g, R.lr_at(LSTM_STEP, lr))
    if dtype != torch.float64:  # the trainer keeps both in float32
        w1, a1 = w1.astype(np.float32), a1.astype(np.float32)
    res["blob1"], res["accum1"] = w1, a1
    return res


def lstm_accum0():
    """the momentum accumulators before the step (test_clip_and_update's: normal, 1e-3), so that the momentum is in the update"""
    return (np.random.default_rng(1).standard_normal(R.FLOATS) * 1e-3).astype(np.float32)


def lstm_checks(got, ref, slices, lr=0.05):
    """got: the GPU trainer's buffers (or another restatement's); ref: lstm_reference in float64.  The tolerances of
    tests/test_gpu_train_lstm.py, the slice rule, and C = +-5.0f bit for bit wherever float64 clips."""
    ck = Checks()
    for key in ("probs", "C", "H", "loss", "acc", "eval_probs"):
        ck.atol(key, got[key], ref[key], 1e-5)
    close_per_tensor(got["grads"], ref["grads"], R.OFFS, checks=ck)
    ck.add("global norm", abs(got["norm"] - ref["norm"]), 1e-5 * ref["norm"])
    close_on_slices(got["grads"], ref["grads"], slices, checks=ck)
    C = np.asarray(got["C"], np.float32)
    ck.exact("C is +5.0f wherever float64 clips from above", int((C[ref["Cpre"] > 5] != np.float32(5.0)).sum()))
    ck.exact("C is -5.0f wherever float64 clips from below", int((C[ref["Cpre"] < -5] != np.float32(-5.0)).sum()))
    # test_clip_and_update's bounds, unchanged.  A weight is stored in float32, so each is off by up to half an ulp, 2^-24 |w|, whatever
    # the kernel does (3.6e-7 at the pushed biases' |w| = 6, against a bound of 1.3e-7 there): that much, per element, is what
    # float32 forces and is taken off the difference before it is held against the bound.
    for name, (off, n) in R.OFFS.items():
        tol = 1e-4 * np.abs(ref["accum1"][off: off + n]).max() + 1e-7
        ck.atol("accumulator after the update " + name, got["accum1"][off: off + n], ref["accum1"][off: off + n], tol)
        ck.atol("weights after the update " + name, got["blob1"][off: off + n], ref["blob1"][off: off + n], lr * tol + 1e-7,
                forced=2.0 ** -24 * np.abs(ref["blob1"][off: off + n]))
    return ck


# name -> (sample indices into train_data_lstm.make_samples(300, seed=21), dropout, the mutants that change the case's result).
# The samples are chosen by the float32 restatement's own error.  A pushed unit's c climbs by at most 1 a step, so it spends
# steps in [2, 4) and [4, 5), where an ulp is 2.4e-7 and 4.8e-7, and the float32 C of a sample ends 0.6e-6 .. 2.4e-6 from float64,
# depending on the sample and on the order of the float32 sums: measured with the CPU library's AVX-512, AVX2 and SSE4 code paths
# (with and without fused multiply-add), on 1 and 8 threads, in batches of 7, 16 and 300 (the matrix products take another path
# per row count).  The trainer tests' bound on C is 1e-5 and the restatement has to stay a factor of 10 inside it, so the cases
# take the samples whose largest error over all those runs is smallest: LSTM_IDX7 the seven best (0.64e-6 .. 0.65e-6), LSTM_IDX7C
# the five best in which a unit LEAVES saturation (its c is clipped at one step and not at the next: where mutant (c) changes
# something; up to 0.78e-6) and the next two, the batch of 16 both and the next two.  A sample's forward quantities depend on
# that sample alone.  Samples drawn without looking (default_rng(7), (16)) end at 0.75e-6 .. 1.26e-6.
LSTM_IDX7 = np.array([236, 53, 175, 189, 66, 193, 161])
LSTM_IDX7C = np.array([114, 94, 143, 46, 68, 35, 219])
LSTM_IDX16 = np.concatenate([LSTM_IDX7, LSTM_IDX7C, [240, 201]])
LSTM_CASES = {
    "batch7": (LSTM_IDX7, False, ("a", "b", "f", "i", "j")),
    "batch7-dropout": (LSTM_IDX7C, True, ("a", "b", "c", "f", "i", "j")),
    "batch16": (LSTM_IDX16, False, ("a", "b", "c", "f", "i", "j")),
    "batch16-dropout": (LSTM_IDX16, True, ("a", "b", "c", "f", "i", "j")),
}
LSTM_SEED, LSTM_STEP, LSTM_LR = 5, 3, 0.05   # the trainer's seed and the step number: the dropout masks are R.dropout_masks of them


def units_leaving_saturation(cpre, n):
    """the number of (sample, step, unit) elements that are not clipped although the step before them was (slot p + 1 runs before p)"""
    clipped = np.abs(np.asarray(cpre).reshape(n, 20, 448)) > 5
    return int((clipped[:, 1:] & ~clipped[:, :-1]).sum())


# ------------------------------------------------------------------------------------------- ETH-CNN: degenerate batches ---
QPS = (22, 27, 32, 37)
HEAD_GAIN = {"ai": 3.0, "ldp": 1.5}
EVAL_QP = 22     # what an evaluation puts every sample at: the first slot of the Low-Delay-P records, whose depths are not capped
FLAT_VALUE = {"ai": 0, "ldp": 128}   # the luma that preprocesses to exactly 0.0, in float64 and in fp32
_REF = {"ai": train_ref, "ldp": train_ref_ldp}
_REC = {"ai": train_data.REC, "ldp": train_data_ldp.REC}
N_EACH = 8


def _ordinary(net, n, seed):
    make = train_data.make_records if net == "ai" else train_data_ldp.make_records
    return np.frombuffer(make(n, seed), np.uint8).reshape(n, _REC[net]).copy()


def _set_labels(rec, net, depths):
    depths = np.asarray(depths, np.uint8).reshape(len(rec), 16)
    if net == "ai":
        rec[:, 4160:] = np.tile(depths, (1, 52))       # the label row of every QP
    else:
        for s in range(4):                             # the label bytes of every slot
            o = train_data_ldp.slot_offset(s)
            rec[:, o + 1: o + 17] = depths
    return rec


def labels_all(d, net="ai", n=N_EACH, seed=31):
    """ordinary records whose 16 depths are all d"""
    return _set_labels(_ordinary(net, n, seed + d), net, np.full((n, 16), d)).tobytes()


def labels_random(seed, net="ai", n=N_EACH):
    """independent depths 0 .. 3 per 16x16 block (no quadtree: y32 and v32 are fractional); every second record draws depth 0 with
    probability 0.8, so that its 64x64 average lies below 1 and y64 is fractional too"""
    rng = np.random.default_rng(seed)
    depths = rng.integers(0, 4, (n, 16))
    depths[1::2] *= rng.random((n, 16))[1::2] >= 0.8
    return _set_labels(_ordinary(net, n, seed), net, depths).tobytes()


def flat_records(value, net="ai", n=N_EACH, seed=37):
    """ordinary records (their labels stay) whose luma is the constant `value`"""
    rec = _ordinary(net, n, seed)
    if net == "ai":
        rec[:, :4096] = value
    else:
        for s in range(4):
            o = train_data_ldp.slot_offset(s)
            rec[:, o + 17: o + 17 + 4096] = value
    return rec.tobytes()


GROUPS = ("ordinary", "all0", "all1", "all3", "random", "flat")


@functools.lru_cache(maxsize=None)
def edge_records(net):
    """one sample set per net: N_EACH records of each group, in GROUPS order (group k at indices N_EACH k ...)"""
    parts = [_ordinary(net, N_EACH, 41).tobytes(), labels_all(0, net), labels_all(1, net), labels_all(3, net), labels_random(43, net),
             flat_records(FLAT_VALUE[net], net)]
    return b"".join(parts)


def _of(group, count):
    return N_EACH * GROUPS.index(group) + np.arange(count)


# name -> (sample indices, zero the biases, the mutants that change the case's result).  Batches of 7 and 16, and one of 1.
CNN_CASES = {
    "all0": (_of("all0", 7), False, ("f", "g")),
    "all1": (_of("all1", 7), False, ("g",)),
    "all3": (_of("all3", 7), False, ("g",)),
    "random": (_of("random", 7), False, ("e",)),
    "mixed16": (np.concatenate([_of("all0", 3), _of("all1", 3), _of("all3", 3), _of("random", 4), _of("ordinary", 3)]), False, ("e", "f")),
    "single": (_of("random", 1), False, ("e", "g")),
    "zero": (np.concatenate([_of("flat", 8), _of("ordinary", 8)]), True, ("d", "f")),
}


def cnn_case(net, name):
    """-> (records, indices, per-sample QPs, weights): synthetic weights (oracle synth_blob, seed 3, head gain HEAD_GAIN: 3 for
    All-Intra spreads the probabilities over 0.16 .. 0.81, at 1 they crowd around 0.5; the Low-Delay-P net, whose input is scaled by
    10, has them over 0.24 .. 0.78 at 1.5, and at 3 its float32 restatement comes within 0.14 of the tolerance on probabilities when
    the sums run without fused multiply-add), the biases zeroed for "zero\""""
    idx, zero_bias, _ = CNN_CASES[name]
    rng = np.random.default_rng(len(name) + len(idx))
    qps = rng.choice(QPS, len(idx))
    blob = train_ref.ethcnn_np.synth_blob(3, HEAD_GAIN[net])
    if zero_bias:
        for tname, shape, off in train_ref.ethcnn_np.TENSORS:
            if len(shape) == 1:
                blob[off // 4: off // 4 + shape[0]] = 0.0
    return edge_records(net), idx, qps, blob


def zero_case_slices():
    """the tensors whose gradient runs through the leaky-ReLU slope at exactly 0: the FC1 biases and the conv biases"""
    out = []
    for tname, shape, off in train_ref.ethcnn_np.TENSORS:
        if len(shape) == 1 and (tname.startswith("h_fc1__") or tname.startswith("Variable")):
            out.append((tname, off // 4 + np.arange(shape[0])))
    assert len(out) == 3 + 9
    return out


def cnn_reference(net, blob, data, idx, qps, dtype=torch.float64):
    """the restatement (or a mutant of it) in the shape cnn_checks takes"""
    ref = _REF[net]
    luma, lab = ref.parse_records(data, idx, qps)
    out, g = ref.loss_and_grad(blob, luma, lab, qps, dtype=dtype)
    with torch.no_grad():  # an evaluation puts every sample at one QP
        eluma, elab = ref.parse_records(data, idx, EVAL_QP)
        ev = ref.net(torch.tensor(np.asarray(blob, dtype=np.float64), dtype=dtype), eluma, elab, EVAL_QP, dtype=dtype)
        empty = []
        for labels in (lab, elab):
            y = torch.as_tensor(np.asarray(labels, dtype=np.float64)).reshape(len(labels), 4, 4, 1)
            _, _, _, v32, v16 = train_ref.split_labels(y)
            empty.append([False, float(v32.sum()) == 0.0, float(v16.sum()) == 0.0])
    return {"probs": out["probs"], "H1": out["H1"], "loss": out["loss_list"], "acc": out["accuracy_list"], "grads": g,
            "eval_probs": ev["probs"].numpy(), "eval_loss": ev["loss_list"].numpy(), "eval_acc": ev["accuracy_list"].numpy(),
            "empty": empty[0], "eval_empty": empty[1]}


def cnn_checks(got, ref, slices=()):
    """got: the GPU trainer's buffers (or another restatement's); ref: cnn_reference in float64 with no mutant.  The tolerances of
    tests/test_gpu_train.py; where a level has no valid element, its loss, its accuracy and its head's FC2 / FC3 gradients are 0.0."""
    ck = Checks()
    for key in ("probs", "loss", "acc", "eval_probs", "eval_loss", "eval_acc"):
        ck.atol(key, got[key], ref[key], 1e-5)
    ck.exact("every gradient is finite", int((~np.isfinite(got["grads"])).sum()))
    close_per_tensor(got["grads"], ref["grads"], CNN_OFFS, checks=ck)
    close_on_slices(got["grads"], ref["grads"], slices, checks=ck)
    for lv in range(3):
        for keys, empty in ((("loss", "acc"), ref["empty"][lv]), (("eval_loss", "eval_acc"), ref["eval_empty"][lv])):
            for key in keys if empty else ():
                ck.exact("%s of the empty level %s is 0.0" % (key, LEVELS[lv]), int(np.asarray(got[key])[lv] != 0))
        if not ref["empty"][lv]:
            continue
        for tname in ("h_fc2__%s__w", "h_fc2__%s__b", "y_conv_flat__%s__w", "y_conv_flat__%s__b"):
            off, n = CNN_OFFS[tname % LEVELS[lv]]
            ck.exact("grad %s of the empty level is 0.0" % (tname % LEVELS[lv]), int((np.asarray(got["grads"][off: off + n]) != 0).sum()))
    return ck


def assert_cnn_preconditions(name, ref):
    """no probability within 1e-5 of 0.5 (an accuracy counts rounded probabilities, and a probability may be 1e-5 off: none may be
    able to change sides) or within 1e-3 of 0 or 1; the flat samples of the zero case have FC1 outputs of exactly 0.0"""
    for key in ("probs", "eval_probs"):
        assert np.abs(ref[key] - 0.5).min() > 1e-5, "a probability within 1e-5 of 0.5"
        assert 1e-3 <= ref[key].min() and ref[key].max() <= 1 - 1e-3
    if name == "zero":
        assert not ref["H1"][:8].any() and ref["H1"][8:].any()
