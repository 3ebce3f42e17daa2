"""Weight sets and inputs that take the EXACT paths (plan 0, the single-launch pass, the ETH-LSTM kernels) out of the finite, normal
arithmetic every seeded blob stays in: subnormal stages, saturated and clamped exponentials, infinities, NaN and signed zeros.

Every builder starts from a seeded blob and edits it through oracle.tensor_views / ethcnn_lstm_np.lstm_views, in the style of
tests/adversarial_blobs.py.  tests/test_edge_values_cpu.py asserts, with the oracle alone and without a GPU, that every fixture really reaches its edge, and tests/test_gpu_edge_values.py imports the same fixtures, so no path
can pass by missing the edge.  Nothing here needs a GPU."""
import numpy as np

f32 = np.float32
NAN, INF = f32("nan"), f32("inf")
TINY = f32(1.4e-45)            # the smallest subnormal
SUB_MAX = f32(1.1754942e-38)   # the largest subnormal: nextafter(2^-126, 0)
SEED, GAIN = 11, 8.0


def nxt(x, to):
    return np.nextafter(f32(x), f32(to))


def _a(xs):
    return np.array(xs, dtype=np.float32)


# --------------------------------------------------------------------------------------------------- the values
# x * log2(e) within an ulp of n + 1/2, where rintf decides between two n: 0.5 ln2, 1.5 ln2, 10.5 ln2 and their neighbours
_TIES = [f32(0.34657359), nxt(0.34657359, 1), nxt(0.34657359, 0), f32(1.0397208), f32(7.2780453)]
EDGE = _a([0.0, -0.0, TINY, -TINY, SUB_MAX, 1e-30, -1e-30, 0.3, -1.7, 2.5]
          + _TIES + [-t for t in _TIES[:2]]
          + [16.6, -16.6,                                   # sigmoid within an ulp of 1 / of e^-16.6
             80.0, nxt(80, INF), nxt(80, 0), -80.0, 86.0, nxt(86, INF), -86.0, nxt(-86, -INF), nxt(-86, 0),   # the clamps and both neighbours
             87.5, -87.5, 89.0, -89.0, 104.0, -104.0, 1e30, -1e30, 3.0e38, -3.0e38,                           # beyond them (2 * 3e38 = Inf in tanh)
             INF, -INF, NAN])
EDGE_FINITE = EDGE[np.isfinite(EDGE)]
# tanh: (e - 1) / (e + 1) cancels for small |x| (2^-30 .. 2^-8) and saturates where exp(2 x) clamps (|x| >= 40 / 43)
TANH_SWEEP = _a([s * 2.0 ** -k for k in range(30, 7, -2) for s in (1, -1)]
                + [0.1, -0.1, 1.0, -1.0, 9.0, -9.0, 39.9, 40.0, 40.1, -42.9, -43.0, -43.1, 44.0, -44.0])
# cell states as a state file may hold them (not necessarily clipped)
CELL = _a([5.0, -5.0, nxt(5, INF), nxt(-5, -INF), nxt(5, 0), 7.0, -7.0, 0.0, -0.0, TINY, -TINY, 1e-39, 0.7, -2.2, INF, -INF, NAN])
CELL_FINITE = CELL[np.isfinite(CELL)]


def logit_tables():
    """tables of 21 logits that together hold every EDGE entry; table 0 starts with NaN (the first gate tests a NaN), table 1 with 80
    (first gate open) and has a NaN among its y32"""
    rest = [x for x in EDGE if not np.isnan(x) and x != f32(80.0)]
    pad = [f32(0.25 * (i + 1)) for i in range(max(0, 39 - len(rest)))]
    rest = rest + pad
    assert len(rest) == 39, len(rest)
    return [_a([NAN] + rest[:20]), _a([f32(80.0), rest[20], NAN] + rest[21:])]


# --------------------------------------------------------------------------------------------------- ETH-CNN blobs
HEAD_TAGS = ("64", "32", "16")
CONV_ALL = ["Variable"] + ["Variable_%d" % i for i in range(1, 18)]
CONV_LAST = ["Variable_4", "Variable_5", "Variable_10", "Variable_11", "Variable_16", "Variable_17"]  # conv3 of L, M, S: kernel, bias


def base_blob(oracle):
    return oracle.synth_blob(SEED, GAIN).copy()


def logit_table_blob(oracle, table):
    """every FC3 weight (qp row included) 0, the 1 + 4 + 16 FC3 biases = table: the logits ARE the table, for every CTU"""
    blob = base_blob(oracle)
    tv = oracle.tensor_views(blob)
    o = 0
    for tag in HEAD_TAGS:
        tv["y_conv_flat__%s__w" % tag][...] = 0.0
        b = tv["y_conv_flat__%s__b" % tag]
        b[...] = table[o:o + b.size]
        o += b.size
    return blob


def scaled_blob(oracle, names, exp2):
    """the named tensors x 2^exp2 (exact: a power of two, until the result leaves the normal range)"""
    blob = base_blob(oracle)
    tv = oracle.tensor_views(blob)
    for n in names:
        tv[n][...] = np.ldexp(tv[n], exp2).astype(np.float32)
    return blob


def subnormal_fc1_blob(oracle):
    return scaled_blob(oracle, ["h_fc1__%s__%s" % (t, p) for t in HEAD_TAGS for p in "wb"], -125)


def subnormal_features_blob(oracle):
    """the LAST conv layer's kernels and biases scaled: the 672 conv3 features are subnormal (the 2016 conv2 features stay as they are).
    Scaling all conv tensors by one factor does not do it: the last bias dominates."""
    return scaled_blob(oracle, CONV_LAST, -128)


def subnormal_fc2_blob(oracle):
    return scaled_blob(oracle, ["h_fc2__%s__%s" % (t, p) for t in HEAD_TAGS for p in "wb"], -125)


def overflow_blob(oracle):
    """finite but huge conv weights: Inf features, Inf - Inf = NaN from FC1 on"""
    return scaled_blob(oracle, CONV_ALL, 43)


# (case name, tensor, index): one element of the tensor is replaced
ONE_WEIGHT_SITES = [("conv1_kernel", "Variable_12", (1, 2, 0, 3)), ("conv3_bias", "Variable_11", (4,)),
                    ("fc1_column", "h_fc1__32__w", (100, 5)), ("fc2_weight", "h_fc2__16__w", (3, 7)),
                    ("fc2_qp_row", "h_fc2__64__w", (64, 2)), ("fc3_bias", "y_conv_flat__32__b", (2,))]
NONFINITE = [("nan", NAN), ("pinf", INF), ("ninf", -INF)]


def one_weight_blob(oracle, tensor, index, value):
    blob = base_blob(oracle)
    oracle.tensor_views(blob)[tensor][index] = value
    return blob


def signed_zero_blob(oracle):
    """output channel 2 of every branch's conv2: weights -0.0 and bias -0.0, and every conv1 bias made positive.  On a flat picture
    the mean-removed input is exactly +0.0, so conv1 gives lrelu(b1) > 0 and the channel's chain is (-0.0) * positive + (-0.0) = -0.0: a
    conv2 FEATURE that is -0.0.  Where a conv1 output is negative the product is +0.0 and the sum +0.0 -- the sign of a zero follows
    the order of the chain."""
    blob = base_blob(oracle)
    tv = oracle.tensor_views(blob)
    for base in (0, 6, 12):
        v = lambda i: "Variable" if base + i == 0 else "Variable_%d" % (base + i)
        tv[v(1)][...] = np.abs(tv[v(1)])
        tv[v(2)][..., 2] = -0.0
        tv[v(3)][2] = -0.0
    return blob


def nan_where_flat_blob(oracle):
    """y64's logit is NaN exactly for a CTU whose top-left 16x16 block is flat, +-Inf otherwise: conv1 channel 0 of branch S without
    bias is exactly 0 on a flat block; one tap of conv2 channel 0, one FC1 column and one FC2 column of head 64 hand that value on
    (x lrelu), and the FC3 weight behind it is +Inf: 0 * Inf = NaN.  Lets a picture place a NaN in one gate sub-batch only."""
    blob = base_blob(oracle)
    tv = oracle.tensor_views(blob)
    tv["Variable_13"][0] = 0.0                       # S conv1 bias, channel 0
    tv["Variable_14"][..., 0] = 0.0                  # S conv2 channel 0: one tap (ky 0, kx 0, ci 0) = 1, no bias
    tv["Variable_14"][0, 0, 0, 0] = 1.0
    tv["Variable_15"][0] = 0.0
    f = 672                                          # first conv2 feature of branch S: position (0, 0), channel 0
    tv["h_fc1__64__w"][:, 0] = 0.0
    tv["h_fc1__64__w"][f, 0] = 1.0
    tv["h_fc1__64__b"][0] = 0.0
    tv["h_fc2__64__w"][:, 0] = 0.0
    tv["h_fc2__64__w"][0, 0] = 1.0
    tv["h_fc2__64__b"][0] = 0.0
    tv["y_conv_flat__64__w"][0, 0] = INF
    return blob


def cnn_fixtures(oracle):
    """name -> blob: every ETH-CNN fixture"""
    out = {}
    for k, t in enumerate(logit_tables()):
        out["logit_table_%d" % k] = logit_table_blob(oracle, t)
    out["subnormal_fc1"] = subnormal_fc1_blob(oracle)
    out["subnormal_features"] = subnormal_features_blob(oracle)
    out["subnormal_fc2"] = subnormal_fc2_blob(oracle)
    out["overflow"] = overflow_blob(oracle)
    for site, tensor, index in ONE_WEIGHT_SITES:
        for vn, v in NONFINITE:
            out["%s_%s" % (site, vn)] = one_weight_blob(oracle, tensor, index, v)
    out["signed_zero"] = signed_zero_blob(oracle)
    return out


FLAT_AI, FLAT_RESI = 0, 128  # after mean removal such a picture is exactly 0.0 (train_edges.FLAT_VALUE)


def mixed_ctus(n, seed=5, resi=False):
    """[n, 64, 64] u8: noise, smooth ramps, flat CTUs (the exact-zero value and others), half-flat CTUs"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, size=(n, 64, 64), dtype=np.uint8)
    if resi:
        c = np.clip(np.rint(128 + rng.laplace(0, 9, size=(n, 64, 64))), 0, 255).astype(np.uint8)
    flat = FLAT_RESI if resi else FLAT_AI
    for i in range(n):
        k = i % 6
        if k == 1:
            c[i] = flat
        elif k == 2:
            c[i] = (np.add.outer(np.arange(64), np.arange(64)) + i) // 2 + 40
        elif k == 3:
            c[i, :, :32] = flat
        elif k == 4:
            c[i] = 255 if i % 12 == 4 else 77
    return c


def picture(w, h, seed=9, resi=False):
    """[h, w] u8 with a flat band (exact zeros after mean removal) and texture"""
    rng = np.random.default_rng(seed)
    if resi:
        p = np.clip(np.rint(128 + rng.laplace(0, 9, size=(h, w))), 0, 255).astype(np.uint8)
        p[: h // 3] = FLAT_RESI
    else:
        p = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        p[: h // 3] = FLAT_AI
    return p


def oracle_stages(oracle, blob, ctus, qp, mode=0, resi=0):
    """-> dict F, H1, logits, probs (ungated) of the C oracle"""
    F = oracle.features(blob, ctus, mode=mode, resi=resi)
    H1 = oracle.fc1(blob, F, mode=mode)
    P, Z = oracle.heads(blob, H1, qp, mode=mode)
    return {"F": F, "H1": H1, "logits": Z, "probs": P}


# --------------------------------------------------------------------------------------------------- ETH-LSTM blobs and inputs
LEVELS = (("64", 64), ("32", 128), ("16", 256))
_K = "RNN%s/multi_rnn_cell/cell_0/lstm_cell/kernel"
_B = "RNN%s/multi_rnn_cell/cell_0/lstm_cell/bias"


def base_lstm_blob(lstm, seed=4, gain=3.0):
    return lstm.synth_lstm_blob(seed, gain).copy()


def gate_table(n, values, jvalues):
    """(i, j, f, o) of n units: i walks `values`, f and o walk it with other strides, every 9th f is -1 (f + forget_bias = 0),
    j walks the tanh sweep followed by `values`"""
    m = len(values)
    jv = np.concatenate([jvalues, values])
    u = np.arange(n)
    gi, gf, go = values[u % m], values[(3 * u + 1) % m].copy(), values[(5 * u + 2) % m]
    gf[::9] = -1.0
    gj = jv[u % len(jv)]
    return np.concatenate([gi, gj, gf, go]).astype(np.float32)


def gate_table_blob(lstm, finite_only=False):
    """cell kernels 0, cell biases = gate tables: i, j, f, o of every unit ARE the table.  Level 64 holds finite entries only (its h,
    and with it y64, stays finite: the first gate has an ordinary value to test); levels 32 and 16 hold +-Inf and NaN unless
    finite_only"""
    blob = base_lstm_blob(lstm)
    tv = lstm.lstm_views(blob)
    for tag, n in LEVELS:
        tv[_K % tag][...] = 0.0
        vals = EDGE_FINITE if (finite_only or tag == "64") else EDGE
        tv[_B % tag][...] = gate_table(n, vals, TANH_SWEEP)
    return blob


def lstm_logit_table_blob(lstm, table):
    """finite gate tables (h finite) + fc3 weights 0 and fc3 biases = table: the LSTM heads' logits are the table"""
    blob = gate_table_blob(lstm, finite_only=True)
    tv = lstm.lstm_views(blob)
    o = 0
    for tag, n in LEVELS:
        tv["RNN%s/fc3/full_connect_w" % tag][...] = 0.0
        b = tv["RNN%s/fc3/full_connect_b" % tag]
        b[...] = table[o:o + b.size]
        o += b.size
    return blob


def subnormal_lstm_blob(lstm):
    """cell kernels x 2^-130: z is subnormal before the bias; the biases of the odd units are 0, so that their gates enter sigmoid /
    tanh subnormal"""
    blob = base_lstm_blob(lstm)
    tv = lstm.lstm_views(blob)
    for tag, n in LEVELS:
        tv[_K % tag][...] = np.ldexp(tv[_K % tag], -130).astype(np.float32)
        tv[_B % tag][1::2] = 0.0
    return blob


# kernel_row and cell_bias_o sit in the o gate (columns 3 n ..): h = sigmoid(o) * tanh(c) takes the value.  cell_bias_j sits in the j gate:
# a NaN there makes c NaN, which the cell clip fminf(fmaxf(c, -5), 5) turns into -5 -- the state stays finite.
# Rows 256..260 of level 16's fc2 are the efs columns; 257 is the one-hot column of phase 0 (i_frame % 4 == 0).
LSTM_ONE_WEIGHT_SITES = [("kernel_row", _K % "32", (7, 390)), ("cell_bias_o", _B % "16", (773,)), ("cell_bias_j", _B % "16", (300,)),
                         ("fc2_efs_row", "RNN16/fc2/full_connect_w", (257, 11))]


def lstm_one_weight_blob(lstm, tensor, index, value):
    blob = base_lstm_blob(lstm)
    lstm.lstm_views(blob)[tensor][index] = value
    return blob


def lstm_fixtures(lstm):
    out = {"gate_table": gate_table_blob(lstm), "gate_table_finite": gate_table_blob(lstm, finite_only=True)}
    for k, t in enumerate(logit_tables()):
        out["lstm_logit_table_%d" % k] = lstm_logit_table_blob(lstm, t)
    out["subnormal_lstm"] = subnormal_lstm_blob(lstm)
    for site, tensor, index in LSTM_ONE_WEIGHT_SITES:
        for vn, v in NONFINITE:
            out["lstm_%s_%s" % (site, vn)] = lstm_one_weight_blob(lstm, tensor, index, v)
    return out


def lstm_inputs(n, seed=3, edge_cells=True, subnormal=False, finite_only=False):
    """vec [n, 448], state [n, 2, 448].  edge_cells: c walks CELL (another entry per CTU and unit); subnormal: half of vec and of
    h_prev scaled into the subnormal range (the MFMA B operands of the cell)"""
    rng = np.random.default_rng(seed)
    vec = (np.abs(rng.standard_normal((n, 448))) * 0.5).astype(np.float32)
    vec[:, ::7] *= -0.2
    c = rng.uniform(-5, 5, (n, 448)).astype(np.float32)
    h = rng.uniform(-1, 1, (n, 448)).astype(np.float32)
    if edge_cells:
        cells = CELL_FINITE if finite_only else CELL
        c = cells[(np.arange(n)[:, None] + 7 * np.arange(448)[None, :]) % len(cells)].astype(np.float32)
    if subnormal:
        vec[:, 1::2] = np.ldexp(vec[:, 1::2], -130).astype(np.float32)
        h[:, ::2] = np.ldexp(h[:, ::2], -130).astype(np.float32)
        vec[:, 4::9] = -0.0
    return vec, np.stack([c, h], 1).astype(np.float32)


# --------------------------------------------------------------------------------------------------- regime checks
def subnormal_share(a):
    """share of non-zero subnormal entries"""
    a = np.abs(np.asarray(a, dtype=np.float32))
    return float(np.mean((a > 0) & (a < f32(2.0 ** -126))))


def same_values(got, want):
    """NaN-aware equality of values (a table entry -0.0 is seen as +0.0 behind `0 + b`, so zeros compare by value)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]))


def same(got, want):
    """THE comparison rule of the exact paths at edge values: NaN patterns equal, everything else equal as uint32 bits (Inf and the
    sign of a zero included).  A NaN's payload and sign are not compared (x86 makes 0xffc00000 for Inf - Inf, the matrix pipe its own)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def diff_report(got, want):
    """a short description of where two arrays differ under same()"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))
    idx = np.argwhere(bad)
    head = ["%s got %r (0x%08x) want %r (0x%08x)" % (tuple(i), float(got[tuple(i)]), int(got.view(np.uint32)[tuple(i)]), float(want[tuple(i)]),
                                                     int(want.view(np.uint32)[tuple(i)])) for i in idx[:4]]
    return "%d of %d differ (%d in the NaN pattern): %s" % (int(bad.sum()), bad.size, int((gn != wn).sum()), "; ".join(head))
