"""No GPU.  (1) Every fixture of tests/edge_values.py really reaches the regime it is named after, shown with the oracle alone -- the
GPU tests (test_gpu_edge_values.py) use the same fixtures, so none of them can pass by missing the edge.  (2) The canonical exp /
sigmoid / tanh of the oracle against numpy float64 over the whole float range.  (3) The oracle against itself: canonical against
literal order (the same NaN positions) and against the float64 restatement.

Measured (x86-64, gcc, -ffp-contract=off), asserted rounded up to the next whole ulp / the next power of two:
    exp      max error over [-86, 80]       0.8873 ulp of the float64 result rounded to float32 (bound asserted: 1 ulp)
    sigmoid  max |error|, whole float range  8.89e-8                                           (bound asserted: 2^-23 = 1.19e-7)
    tanh     max |error|, whole float range  1.34e-7                                           (bound asserted: 2^-22 = 2.38e-7)
tanh is odd to within its bound and monotone non-decreasing across the clamps of its exp (|x| around 40 and 43) to within it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_values as ev  # noqa: E402

EXP_ULP_BOUND = 1.0
SIGMOID_ABS_BOUND = 2.0 ** -23
TANH_ABS_BOUND = 2.0 ** -22
QP = 32
N_CTUS = 37


@pytest.fixture(scope="module")
def lstm(oracle):
    import ethcnn_lstm_np
    return ethcnn_lstm_np


@pytest.fixture(scope="module")
def ctus():
    return ev.mixed_ctus(N_CTUS)


@pytest.fixture(scope="module")
def cnn(oracle):
    return ev.cnn_fixtures(oracle)


@pytest.fixture(scope="module")
def stages(oracle, cnn, ctus):
    """name -> oracle stages (canonical mode), computed once"""
    with np.errstate(all="ignore"):
        return {name: ev.oracle_stages(oracle, blob, ctus, QP) for name, blob in cnn.items()}


# ------------------------------------------------------------------------------------------------ regimes: ETH-CNN
def test_seeded_weights_stay_in_finite_normal_arithmetic(oracle, ctus):
    """what the issue starts from: the seeded blob reaches none of the edges"""
    st = ev.oracle_stages(oracle, ev.base_blob(oracle), ctus, QP)
    for k in ("F", "H1", "logits", "probs"):
        assert np.isfinite(st[k]).all() and ev.subnormal_share(st[k]) == 0.0, k
    assert np.abs(st["logits"]).max() < 40.0


def test_logit_tables_are_the_logits(stages):
    seen = []
    for k, table in enumerate(ev.logit_tables()):
        st = stages["logit_table_%d" % k]
        for row in st["logits"]:
            assert ev.same_values(row, table), (k, row, table)   # every CTU: the 21 logits are the table (-0.0 arrives as +0.0 behind 0 + b)
        seen.append(table)
        p = st["probs"][0]
        fin = np.isfinite(table)
        with np.errstate(over="ignore"):
            assert np.abs(p[fin] - 1.0 / (1.0 + np.exp(-table[fin].astype(np.float64)))).max() <= 2.0 ** -23
        assert np.array_equal(np.isnan(p), np.isnan(table))       # NaN logit -> NaN probability, nothing else is NaN
        for x, want in ((np.inf, 0x3f800000), (-np.inf, 0x05bfecba), (0.0, 0x3f000000), (1e30, 0x3f800000), (-1e30, 0x05bfecba)):
            for j in np.flatnonzero(table == np.float32(x)):
                assert int(p[j:j + 1].view(np.uint32)[0]) == want, (x, hex(int(p[j:j + 1].view(np.uint32)[0])))
    allv = np.concatenate(seen)
    for e in ev.EDGE:  # every edge value is in some table
        assert (np.isnan(allv).any() if np.isnan(e) else (allv.view(np.uint32) == np.float32(e).view(np.uint32)).any()), e


@pytest.mark.parametrize("name,stage,part", [("subnormal_fc1", "H1", slice(None)), ("subnormal_features", "F", slice(0, 672))])
def test_subnormal_stage_is_subnormal(stages, name, stage, part):
    share = ev.subnormal_share(stages[name][stage][:, part])
    print(name, "share of non-zero subnormals: %.3f" % share)
    assert share >= 0.25, share
    assert np.isfinite(stages[name]["probs"]).all()


def test_subnormal_fc2_stage_is_subnormal(oracle, cnn, stages):
    """the oracle does not export FC2 outputs: restated here in float64 from its FC1 outputs"""
    tv = oracle.tensor_views(cnn["subnormal_fc2"])
    H1 = stages["subnormal_fc2"]["H1"].astype(np.float64)
    o, shares = 0, []
    for tag, n1 in zip(ev.HEAD_TAGS, (64, 128, 256)):
        x = np.concatenate([H1[:, o:o + n1], np.full((H1.shape[0], 1), QP * np.float64(np.float32(1.0 / 51.0)))], 1)
        z = x @ tv["h_fc2__%s__w" % tag].astype(np.float64) + tv["h_fc2__%s__b" % tag]
        h2 = np.abs(np.maximum(0.2 * z, z))
        shares.append(float(np.mean((h2 > 0) & (h2 < 2.0 ** -126))))
        o += n1
    print("subnormal_fc2 shares per head", shares)
    assert min(shares) >= 0.25, shares


def test_subnormal_probabilities_stay_close_to_float64(oracle, cnn, ctus, stages):
    for name in ("subnormal_fc1", "subnormal_features", "subnormal_fc2"):
        ref = oracle.forward64(cnn[name], ctus, QP)
        d = float(np.abs(stages[name]["probs"] - ref["probs"]).max())
        print(name, "max |p - float64| = %.3g" % d)
        assert d <= 1e-4, (name, d)


def test_overflow_from_finite_weights(cnn, stages):
    assert np.isfinite(cnn["overflow"]).all()
    st = stages["overflow"]
    assert np.isinf(st["F"]).any() and np.isinf(st["H1"]).any() and np.isnan(st["H1"]).any()
    share = float(np.isnan(st["logits"]).mean())
    print("overflow: NaN logits %.2f, Inf FC1 %.2f, NaN FC1 %.2f" % (share, np.isinf(st["H1"]).mean(), np.isnan(st["H1"]).mean()))
    assert 0.05 <= share <= 0.95          # NaN and non-NaN logits both present
    assert np.isnan(st["probs"]).any() and (~np.isnan(st["probs"])).any()


@pytest.mark.parametrize("site", [s[0] for s in ev.ONE_WEIGHT_SITES])
@pytest.mark.parametrize("vn", [v[0] for v in ev.NONFINITE])
def test_one_nonfinite_weight_reaches_the_output(cnn, stages, site, vn):
    """A NaN weight gives at least one NaN probability, and at least one value of the pass stays a number (features of another branch
    at the least, for the sites in front of FC1, whose every output sums every feature).  An infinite weight gives a non-finite
    logit; whether that is a NaN depends on the site (Inf in an FC3 bias is a saturated probability, not a NaN)."""
    name = "%s_%s" % (site, vn)
    assert int((~np.isfinite(cnn[name])).sum()) == 1
    st = stages[name]
    assert (~np.isfinite(st["logits"])).any(), name
    if vn == "nan":
        assert np.isnan(st["probs"]).any(), name
    every = np.concatenate([st[k].reshape(-1) for k in ("F", "H1", "logits", "probs")])
    assert (~np.isnan(every)).any() and np.isfinite(st["F"]).any(), name
    if site in ("fc1_column", "fc2_weight", "fc2_qp_row", "fc3_bias"):   # one head only: the other heads' probabilities are numbers
        assert (~np.isnan(st["probs"])).any(), name


def test_flat_ctus_give_negative_zero_features(stages, ctus):
    F = stages["signed_zero"]["F"]
    negzero = (F == 0) & np.signbit(F)
    flat = np.array([(c == c.flat[0]).all() for c in ctus])
    assert flat.any() and negzero[flat].any(), "a flat CTU must give a -0.0 feature"
    assert ((F == 0) & ~np.signbit(F)).sum() >= 0 and np.isfinite(F).all()
    print("signed_zero: %d features are -0.0, %d of them in flat CTUs" % (int(negzero.sum()), int(negzero[flat].sum())))


def test_nan_where_flat_blob_places_its_nan(oracle):
    """y64 is NaN where the CTU's first 16x16 block is the exact-zero flat value, a saturated number where that block has texture
    (a flat block of another value is not exactly 0 after mean removal: either may come out)"""
    blob = ev.nan_where_flat_blob(oracle)
    c = ev.mixed_ctus(12, seed=8)
    zero_block = np.array([(x[:16, :16] == ev.FLAT_AI).all() for x in c])
    textured = np.array([len(np.unique(x[:16, :16])) > 16 for x in c])
    with np.errstate(all="ignore"):
        st = ev.oracle_stages(oracle, blob, c, QP)
    assert zero_block.any() and textured.any()
    assert np.isnan(st["probs"][zero_block, 0]).all() and not np.isnan(st["probs"][textured, 0]).any()
    assert not np.isnan(st["probs"][:, 1:]).any()


# ------------------------------------------------------------------------------------------------ regimes: ETH-LSTM
def _levels(a):
    return {"64": a[..., 0:64], "32": a[..., 64:192], "16": a[..., 192:448]}


def test_gate_tables_are_the_gates(lstm):
    """with zero kernels the pre-activations are the biases; shown through the state the oracle writes: c and h equal the cell
    formula evaluated on the table in float64 wherever that is finite, NaN where the table or the state says so"""
    blob = ev.gate_table_blob(lstm)
    vec, state = ev.lstm_inputs(45)
    with np.errstate(all="ignore"):
        P, S = lstm.lstm_step(blob, vec, state, QP, 2, 0.5, 0.5, mode=0)
        tv = lstm.lstm_views(blob)
        for tag, n in ev.LEVELS:
            gi, gj, gf, go = [tv[ev._B % tag][k * n:(k + 1) * n].astype(np.float64) for k in range(4)]
            for e in (ev.EDGE_FINITE if tag == "64" else ev.EDGE):   # every table entry is a gate value
                assert (np.isnan(gi).any() if np.isnan(e) else (gi.astype(np.float32).view(np.uint32) == np.float32(e).view(np.uint32)).any()), (tag, e)
            assert (gf == -1.0).any()
            sig = lambda x: 1.0 / (1.0 + np.exp(-np.clip(x, -86.0, 80.0)))
            cp = _levels(state[:, 0])[tag].astype(np.float64)
            c64 = np.clip(sig(gf + 1.0) * cp + sig(gi) * np.tanh(gj), -5.0, 5.0)
            c = _levels(S[:, 0])[tag]
            ok = np.isfinite(c64)
            assert np.abs(c[ok] - c64[ok]).max() <= 1e-5, tag
            if tag != "64":
                assert np.isnan(S[:, 1][:, 64:]).any()
    assert np.isfinite(S[:, :, :64]).all() and np.isfinite(P[:, 0]).all()      # level 64 stays finite: y64 is a number
    assert np.isnan(P[:, 1:5]).all()                                            # a NaN h poisons every output of its level
    # the cell clip maps a NaN to -5 (fminf(fmaxf(NaN, -5), 5)): c is never NaN, h = sigmoid(o) * tanh(-5) is
    assert not np.isnan(S[:, 0]).any() and (S[:, 0] == -5.0).any()


def test_lstm_fixtures_reach_their_regimes(lstm):
    fx = ev.lstm_fixtures(lstm)
    vec, state = ev.lstm_inputs(45, finite_only=True)
    with np.errstate(all="ignore"):
        for k, table in enumerate(ev.logit_tables()):
            P, S = lstm.lstm_step(fx["lstm_logit_table_%d" % k], vec, state, QP, 2, -1.0, -1.0, mode=0)
            assert np.isfinite(S).all()
            want = np.asarray(base_sigmoid(table), np.float32)
            keep = np.ones(21, bool)
            if np.isnan(table[0]):
                keep[1:5] = False          # a NaN y64 fails `> thr`: the first gate closes and zero-fills y32, whatever the threshold
                assert (P[:, 1:5] == 0).all()
            assert np.array_equal(np.isnan(P[0, keep]), np.isnan(table[keep])) and np.nanmax(np.abs(P[0, keep] - want[keep])) <= 2.0 ** -23
        # subnormal z: the share is measured on z itself, restated in float64
        tv = lstm.lstm_views(fx["subnormal_lstm"])
        for tag, n in ev.LEVELS:
            x = np.concatenate([_levels(vec)[tag], _levels(state[:, 1])[tag]], 1).astype(np.float64)
            z = np.abs(x @ tv[ev._K % tag].astype(np.float64))
            share = float(np.mean((z > 0) & (z < 2.0 ** -126)))
            assert share >= 0.25, (tag, share)
        P, S = lstm.lstm_step(fx["subnormal_lstm"], vec, state, QP, 2, 0.5, 0.5, mode=0)
        assert np.isfinite(P).all() and np.isfinite(S).all()
        for site, _, _ in ev.LSTM_ONE_WEIGHT_SITES:
            for vn, _ in ev.NONFINITE:
                P, S = lstm.lstm_step(fx["lstm_%s_%s" % (site, vn)], vec, state, QP, 4, -1.0, -1.0, mode=0)   # i_frame 4: phase 0, the efs row used
                every = np.concatenate([P.reshape(-1), S.reshape(-1)])
                assert np.isfinite(every).any(), (site, vn)
                if site == "cell_bias_j":      # the clip swallows it: NaN -> c = -5 exactly, +-Inf -> tanh saturates; all finite
                    assert np.isfinite(every).all(), (site, vn)
                    if vn == "nan":
                        assert (S[:, 0, 192 + 44] == -5.0).all()
                elif vn == "nan":
                    assert np.isnan(P).any() and (~np.isnan(P)).any(), (site, vn)
                    assert np.isnan(S[:, 1]).any() == (site != "fc2_efs_row"), (site, vn)   # fc2 lies behind the state
    v2, s2 = ev.lstm_inputs(45, subnormal=True, edge_cells=False)
    assert ev.subnormal_share(v2) >= 0.25 and ev.subnormal_share(s2[:, 1]) >= 0.25


def base_sigmoid(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.clip(x, -86.0, 80.0)))


# ------------------------------------------------------------------------------------------------ the canonical functions
def _all_exponents(lo=None, hi=None):
    """every exponent x 4096 mantissas x both signs (subnormals, zeros included), optionally cut to [lo, hi]"""
    e = np.arange(0, 255, dtype=np.uint32)[:, None] << np.uint32(23)
    m = (np.arange(4096, dtype=np.uint32) * np.uint32(2048) + np.uint32(1023))[None, :]   # 4096 mantissas over the 23 bits, odd low bits
    pos = (e | m).reshape(-1)
    bits = np.concatenate([pos, pos | np.uint32(0x80000000), np.array([0, 0x80000000, 1, 0x80000001, 0x7f7fffff, 0xff7fffff], np.uint32)])
    x = bits.view(np.float32)
    if lo is not None:
        x = x[(x >= lo) & (x <= hi)]
    return x


def test_canonical_exp_against_float64(oracle):
    x = np.concatenate([_all_exponents(-86.0, 80.0), np.linspace(-86, 80, 400001).astype(np.float32), ev.EDGE_FINITE[np.abs(ev.EDGE_FINITE) <= 80]])
    got = oracle.canon_math("exp", x).astype(np.float64)
    want = np.exp(x.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = float((np.abs(got - want) / ulp).max())
    print("canonical exp: max error %.4f ulp over %d arguments" % (err, x.size))
    assert err <= EXP_ULP_BOUND
    assert (got >= np.float64(2.0 ** -126)).all()   # "stays normal": no result is subnormal
    assert float(oracle.lib().oracle_expf_export(0.0)) == 1.0
    # outside the clamps: exp(80) above, exp(-86) below, +-Inf included; NaN stays NaN
    e80, e86 = oracle.canon_math("exp", [80.0])[0], oracle.canon_math("exp", [-86.0])[0]
    out = oracle.canon_math("exp", [81.0, 1e30, np.inf, -86.5, -1e30, -np.inf, np.nan])
    assert (out[:3] == e80).all() and (out[3:6] == e86).all() and np.isnan(out[6])


def test_canonical_sigmoid_and_tanh_against_float64(oracle):
    x = np.concatenate([_all_exponents(), ev.EDGE_FINITE, ev.TANH_SWEEP, np.linspace(-100, 100, 400001).astype(np.float32)])
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore"):
        s_err = float(np.abs(oracle.canon_math("sigmoid", x) - 1.0 / (1.0 + np.exp(-x64))).max())
        t = oracle.canon_math("tanh", x)
        t_err = float(np.abs(t - np.tanh(x64)).max())
    print("canonical sigmoid: max |error| %.3g; tanh: max |error| %.3g over %d arguments" % (s_err, t_err, x.size))
    assert s_err <= SIGMOID_ABS_BOUND
    assert t_err <= TANH_ABS_BOUND
    # odd to within the bound (exp(2x) and exp(-2x) clamp at different |x|: 40 and 43)
    assert np.abs(t + oracle.canon_math("tanh", -x)).max() <= TANH_ABS_BOUND
    # monotone across the clamps to within the bound
    xs = np.sort(np.concatenate([np.linspace(-44, -39, 200001), np.linspace(39, 44, 200001)]).astype(np.float32))
    ts = oracle.canon_math("tanh", xs)
    assert (np.diff(ts.astype(np.float64)) >= -TANH_ABS_BOUND).all()
    assert np.abs(ts).max() <= 1.0
    # non-finite: TensorFlow's sigmoid / tanh of NaN are NaN; +-Inf saturate
    assert np.isnan(oracle.canon_math("sigmoid", [np.nan])[0]) and np.isnan(oracle.canon_math("tanh", [np.nan])[0])
    sg = oracle.canon_math("sigmoid", [np.inf, -np.inf]).view(np.uint32)
    assert int(sg[0]) == 0x3f800000 and int(sg[1]) == 0x05bfecba
    th = oracle.canon_math("tanh", [np.inf, -np.inf, 3e38, -3e38])
    assert th[0] == 1.0 and th[2] == 1.0 and th[1] == -1.0 and th[3] == -1.0


# ------------------------------------------------------------------------------------------------ the oracle against itself
def test_canonical_and_literal_order_have_the_same_nan_positions(oracle, cnn, ctus, stages):
    """Every fixture but one: the same NaN positions at every stage.  The overflow fixture cannot promise that: its largest features
    lie within a rounding of FLT_MAX, so the ORDER of a chain decides whether one becomes Inf (measured: 4 of 99456 features are Inf
    in one order only), and every FC1 output sums every feature -- from FC1 on its NaN pattern belongs to the order.  There the
    features are compared: no NaN in either order, and Inf patterns that differ in at most 0.1 % of the positions."""
    with np.errstate(all="ignore"):
        for name, blob in cnn.items():
            lit = ev.oracle_stages(oracle, blob, ctus, QP, mode=1)
            rows = np.ones(len(ctus), bool)
            if name in ("conv1_kernel_pinf", "conv1_kernel_ninf"):
                # Inf * v is NaN where the mean-removed input v is exactly 0, +-Inf elsewhere.  On a flat block of a NON-zero value the
                # canonical centring fma(sum, c, -mean) gives exactly 0 and the literal x * c - mean need not (DESIGN.md section 2,
                # centring): those CTUs are left out, all others must agree
                rows = np.array([not ((c == c.flat[0]).all() and c.flat[0] != ev.FLAT_AI) for c in ctus])
                assert rows.sum() >= len(ctus) - 6
            if name == "overflow":
                assert not np.isnan(lit["F"]).any() and not np.isnan(stages[name]["F"]).any()
                assert np.isinf(lit["F"]).any() and (np.isinf(lit["F"]) != np.isinf(stages[name]["F"])).mean() <= 1e-3
                continue
            for k in ("F", "H1", "logits", "probs"):
                assert np.array_equal(np.isnan(lit[k][rows]), np.isnan(stages[name][k][rows])), (name, k)


def test_against_float64_where_no_stage_overflowed(oracle, cnn, ctus, stages):
    with np.errstate(all="ignore"):
        for name, blob in cnn.items():
            if name == "overflow":
                continue   # the float64 model legitimately differs: it does not overflow where fp32 does
            ref = oracle.forward64(blob, ctus, QP)
            got = stages[name]["probs"]
            both = np.isfinite(got) & np.isfinite(ref["probs"])
            # a CTU whose fp32 stages are all finite
            clean = np.isfinite(stages[name]["F"]).all(axis=1) & np.isfinite(stages[name]["H1"]).all(axis=1)
            sel = both & clean[:, None]
            if sel.any():
                d = float(np.abs(got[sel] - ref["probs"][sel]).max())
                assert d <= 1e-4, (name, d)


# ------------------------------------------------------------------------------------------------ the 16-bit plans' guard, host side
@pytest.mark.parametrize("plan", [2, 3])
def test_fast_plan_bound_refuses_nonfinite_weights_and_unrepresentable_scales(pkg, oracle, cnn, plan):
    """ethcnn_fast_plan_bound (host arithmetic on the blob, no device): stage 0 of the guard.  A weight that is not finite has no scale
    -- also where it enters neither the bound nor a scale (an FC3 bias: the logit tables).  FC1 weights x 2^-125 make the power-of-two
    scale of W1 overflow a float (the plan computed NaN probabilities while the bound, computed in double, accepted it); the conv3
    kernels x 2^-128 do the same to plan 3's trunk scale and leave plan 2, which runs the exact trunk, alone."""
    e = pkg.ethcnn
    ok, bound, _ = e.fast_plan_bound(ev.base_blob(oracle), plan)
    assert np.isfinite(bound) and bound > 0
    for name, blob in cnn.items():
        ok, bound, _ = e.fast_plan_bound(blob, plan)
        if not np.isfinite(blob).all() or name == "subnormal_fc1" or (name == "subnormal_features" and plan == 3):
            assert not ok and bound == np.inf, (name, ok, bound)
        elif name in ("subnormal_fc2", "signed_zero") or (name == "subnormal_features" and plan == 2):
            assert np.isfinite(bound), (name, bound)
