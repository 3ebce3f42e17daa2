"""-m gpu: the exact paths at subnormal, saturated and non-finite values (plan 0, the single-launch small pass and
the ETH-LSTM kernels match the oracle's canonical mode bit for bit -- here where no seeded blob takes them).  The fixtures are
tests/edge_values.py; tests/test_edge_values_cpu.py shows with the oracle alone that each reaches its regime.

Comparison rule (edge_values.same): equal NaN patterns, everything else equal as uint32 bits -- Inf and the sign of a zero included;
a NaN's payload and sign are not compared.  Every stage the library can hand out (features, FC1, logits, ungated probabilities, gated
output; LSTM probabilities and the (c, h) state) is compared on its own, so a failure names the stage.

The kernels' addresses and loop bounds do not depend on float values (the only float -> int conversion of the inference kernels is
the exponent of the canonical exp, behind its clamps and its NaN return; gate predicates only set flag words): these inputs are data."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_values as ev  # noqa: E402

pytestmark = pytest.mark.gpu

QP = 32
THR = (0.5, 0.5)
TOL = 1e-4


def _assert_same(got, want, what):
    assert ev.same(got, want), "%s: %s" % (what, ev.diff_report(got, want))


@pytest.fixture(scope="module")
def lstm(oracle):
    import ethcnn_lstm_np
    return ethcnn_lstm_np


@pytest.fixture(scope="module")
def cnn(oracle):
    return ev.cnn_fixtures(oracle)


@pytest.fixture(scope="module")
def ctus37():
    return ev.mixed_ctus(37)   # two groups of 16 and a partial one


_WANT = {}


def _want(oracle, cnn, name, ctus, key):
    """oracle stages of fixture `name` on a CTU set, computed once per (fixture, set)"""
    k = (name, key)
    if k not in _WANT:
        with np.errstate(all="ignore"):
            st = ev.oracle_stages(oracle, cnn[name], ctus, QP)
            st["gated"] = oracle.gates(st["probs"], THR[0], THR[1])
        _WANT[k] = st
    return _WANT[k]


def _run_and_compare(pkg, c, run, n, want, what):
    """run() -> gated output of a pass over n CTUs with debug capture on; every stage against `want`"""
    e = pkg.ethcnn
    c.set_debug_capture(True)
    try:
        got = run()
        _assert_same(c.debug_fetch(e.DBG_FEATURES, n), want["F"], what + ": features")
        _assert_same(c.debug_fetch(e.DBG_FC1, n), want["H1"], what + ": FC1")
        _assert_same(c.debug_fetch(e.DBG_LOGITS, n), want["logits"], what + ": logits")
        _assert_same(c.debug_fetch(e.DBG_RAW_PROBS, n), want["probs"], what + ": ungated probabilities")
        _assert_same(got, want["gated"], what + ": gated output")
    finally:
        c.set_debug_capture(False)


CNN_NAMES = ["logit_table_0", "logit_table_1", "subnormal_fc1", "subnormal_features", "subnormal_fc2", "overflow", "signed_zero"] + \
            ["%s_%s" % (s[0], v[0]) for s in ev.ONE_WEIGHT_SITES for v in ev.NONFINITE]


def test_fixture_list_is_complete(oracle, cnn):
    assert sorted(CNN_NAMES) == sorted(cnn.keys())


# ------------------------------------------------------------------------------------------------ ETH-CNN, plan 0
@pytest.mark.parametrize("name", CNN_NAMES)
def test_multi_launch_pass_37_ctus(pkg, ctx, oracle, cnn, ctus37, name):
    want = _want(oracle, cnn, name, ctus37, "37")
    ctx.load_blob(cnn[name])
    ctx.set_thresholds(*THR)
    ctx.set_small_pass_launch(False)
    try:
        _run_and_compare(pkg, ctx, lambda: ctx.predict_ctus(ctus37, QP), 37, want, name)
    finally:
        ctx.set_small_pass_launch(True)


@pytest.mark.parametrize("name", ["subnormal_fc1", "fc1_column_nan"])
def test_multi_launch_pass_1800_ctus_bulk_fc1(pkg, ctx, oracle, cnn, name):
    """past the last FC1 shape switch (1793 CTUs): k_fc1_bulk"""
    ctus = ev.mixed_ctus(1800, seed=6)
    with np.errstate(all="ignore"):
        want = ev.oracle_stages(oracle, cnn[name], ctus, QP)
        want["gated"] = oracle.gates(want["probs"], THR[0], THR[1])
    if name == "subnormal_fc1":
        assert ev.subnormal_share(want["H1"]) >= 0.25
    else:
        assert np.isnan(want["probs"]).any() and (~np.isnan(want["probs"])).any()
    ctx.load_blob(cnn[name])
    ctx.set_thresholds(*THR)
    ctx.set_small_pass_launch(False)
    try:
        _run_and_compare(pkg, ctx, lambda: ctx.predict_ctus(ctus, QP), 1800, want, name)
    finally:
        ctx.set_small_pass_launch(True)


@pytest.mark.parametrize("name", CNN_NAMES)
def test_small_pictures_default_path(pkg, ctx, oracle, cnn, name):
    """one small picture as the library runs it by default, 12 CTUs, ragged right and bottom (zero pad: flat blocks, exact zeros):
    208 x 136 is ONE launch (the single-launch pass needs rows that are multiples of 16 bytes), 200 x 136 is not and takes the
    five launches on its own"""
    for w, h, single in ((208, 136, True), (200, 136, False)):
        luma = ev.picture(w, h)
        ctus = oracle.tile_frame(luma, w, h)
        want = _want(oracle, cnn, name, ctus, "%dx%d" % (w, h))
        ctx.load_blob(cnn[name])
        ctx.set_thresholds(*THR)
        ctx.set_small_pass_launch(True)
        ctx.set_profiling(2)
        ctx.reset_stage_times()
        try:
            _run_and_compare(pkg, ctx, lambda: ctx.predict_luma(luma, w, h, 1, QP), 12, want, "%s %dx%d" % (name, w, h))
            st = ctx.stage_times()["launches"]
            assert ((st["tile"], st["trunk"], st["heads"], st["gate"]) == (0, 0, 0, 0)) == single, (w, st)   # 208: really ONE launch
        finally:
            ctx.set_profiling(0)


def test_single_launch_pass_nan_in_the_second_gate_sub_batch(pkg, ctx, oracle):
    """2560 x 1920: 1200 CTUs, gate sub-batches of 1024 and 176.  Every CTU is textured (y64 saturated, a number) except CTUs of
    the SECOND sub-batch whose first block is flat zero: their y64 is NaN (edge_values.nan_where_flat_blob), so that sub-batch's gate
    predicate tests NaN > thr; expected result from oracle.gates"""
    w, h = 2560, 1920
    blob = ev.nan_where_flat_blob(oracle)
    rng = np.random.default_rng(77)
    luma = rng.integers(1, 256, size=(h, w), dtype=np.uint8)
    for i in (1030, 1100, 1199):   # CTU index -> its top-left 16x16 block
        cy, cx = divmod(i, w // 64)
        luma[cy * 64: cy * 64 + 16, cx * 64: cx * 64 + 16] = ev.FLAT_AI
    ctus = oracle.tile_frame(luma, w, h)
    with np.errstate(all="ignore"):
        want = ev.oracle_stages(oracle, blob, ctus, QP)
    nan64 = np.isnan(want["probs"][:, 0])
    assert not nan64[:1024].any() and sorted(np.flatnonzero(nan64)) == [1030, 1100, 1199]
    ctx.load_blob(blob)
    for thr in (THR, (2.0, 0.5), (0.5, 2.0)):   # open; first gate closed everywhere (NaN > 2 is as false as 1 > 2); second closed
        want["gated"] = oracle.gates(want["probs"], thr[0], thr[1])
        ctx.set_thresholds(*thr)
        _run_and_compare(pkg, ctx, lambda: ctx.predict_luma(luma, w, h, 1, QP), 1200, want, "thr %r" % (thr,))
    ctx.set_thresholds(*THR)


@pytest.mark.parametrize("name", ["subnormal_fc1", "subnormal_features", "overflow", "signed_zero", "conv1_kernel_nan", "conv1_kernel_pinf",
                                  "conv3_bias_ninf", "fc1_column_nan", "fc1_column_pinf"])
def test_resi_vectors_small_pictures(ctx, oracle, cnn, name):
    """the LDP front end (FC1 outputs of a residual picture; flat value 128 is exactly 0 after mean removal); 208 wide: the single
    launch where it is on"""
    ctx.load_blob(cnn[name])
    for w, h in ((200, 136), (208, 136)):
        luma = ev.picture(w, h, seed=10, resi=True)
        with np.errstate(all="ignore"):
            want = oracle.resi_vectors(cnn[name], luma, w, h, mode=0)
        for on in (True, False):
            ctx.set_small_pass_launch(on)
            _assert_same(ctx.resi_vectors(luma, w, h), want, "%s %dx%d, single launch %s" % (name, w, h, on))
    ctx.set_small_pass_launch(True)


# ------------------------------------------------------------------------------------------------ ETH-LSTM
@pytest.fixture(scope="module")
def lfx(lstm):
    return ev.lstm_fixtures(lstm)


LSTM_NAMES = ["gate_table", "gate_table_finite", "lstm_logit_table_0", "lstm_logit_table_1", "subnormal_lstm"] + \
             ["lstm_%s_%s" % (s[0], v[0]) for s in ev.LSTM_ONE_WEIGHT_SITES for v in ev.NONFINITE]


@pytest.mark.parametrize("n", [45, 700])   # k_lstm_frame / k_lstm_cell + k_lstm_heads (the switch is 640)
@pytest.mark.parametrize("name", LSTM_NAMES)
def test_lstm_step(ctx, lstm, lfx, name, n):
    assert sorted(LSTM_NAMES) == sorted(lfx.keys())
    blob = lfx[name]
    ctx.load_lstm_blob(blob)
    ctx.set_thresholds(*THR)
    finite = name != "gate_table"                      # the fixtures with finite tables keep finite cell states: h stays a number
    sub = name == "subnormal_lstm"
    vec, state = ev.lstm_inputs(n, seed=n, edge_cells=not sub, subnormal=sub, finite_only=finite)
    # i_frame 1: zero state; 2: the state given; 4: phase 0 (the efs row the one-weight fixture edits)
    for i_frame, sin in ((1, None), (2, state), (4, state)):
        with np.errstate(all="ignore"):
            want_p, want_s = lstm.lstm_step(blob, vec, sin, QP, i_frame, THR[0], THR[1], mode=0)
        got_p, got_s = ctx.lstm_step(vec, sin, QP, i_frame)
        _assert_same(got_s, want_s, "%s n %d i_frame %d: state" % (name, n, i_frame))
        _assert_same(got_p, want_p, "%s n %d i_frame %d: probabilities" % (name, n, i_frame))


def test_lstm_step_with_nonfinite_state_on_seeded_weights(ctx, lstm):
    """a state file holding +-Inf, NaN, unclipped and subnormal cells, through the seeded kernels (the MFMA chain sees the h values)"""
    blob = ev.base_lstm_blob(lstm)
    ctx.load_lstm_blob(blob)
    ctx.set_thresholds(*THR)
    for n in (45, 700):
        vec, state = ev.lstm_inputs(n, seed=50 + n, subnormal=True)
        rows, cols = state[::5, 1, 3::11].shape                                         # h_prev: edge values too, in every 5th CTU
        state[::5, 1, 3::11] = ev.CELL[(np.arange(rows)[:, None] + np.arange(cols)[None, :]) % len(ev.CELL)]
        with np.errstate(all="ignore"):
            want_p, want_s = lstm.lstm_step(blob, vec, state, QP, 3, THR[0], THR[1], mode=0)
        assert np.isnan(want_s).any() and np.isfinite(want_s).any()
        got_p, got_s = ctx.lstm_step(vec, state, QP, 3)
        _assert_same(got_s, want_s, "n %d: state" % n)
        _assert_same(got_p, want_p, "n %d: probabilities" % n)


SEQ_NAMES = ["gate_table", "lstm_logit_table_0", "subnormal_lstm", "lstm_kernel_row_nan", "lstm_cell_bias_j_nan", "lstm_fc2_efs_row_pinf"]


@pytest.mark.parametrize("name", SEQ_NAMES)
def test_ldp_sequence_3_frames_200x136(ctx, oracle, lstm, lfx, name):
    """the one-launch recurrence (ethcnn_lstm_seq.hip) against the per-frame oracle loop; the front end runs on seeded weights"""
    w, h, nf = 200, 136, 3
    cblob = ev.base_blob(oracle)
    ctx.load_blob(cblob)
    ctx.load_lstm_blob(lfx[name])
    ctx.set_thresholds(*THR)
    frames = np.stack([ev.picture(w, h, seed=20 + t, resi=True) for t in range(nf)])
    got = ctx.ldp_sequence(frames, w, h, nf, QP, i_frame_first=1)
    st = None
    with np.errstate(all="ignore"):
        for t in range(nf):
            vec = oracle.resi_vectors(cblob, frames[t], w, h)
            p, st = lstm.lstm_step(lfx[name], vec, st, QP, 1 + t, THR[0], THR[1], mode=0)
            _assert_same(got[t], p, "%s frame %d" % (name, t))
    _assert_same(ctx.ldp_get_state(w, h), st, name + ": final state")


def test_group_of_two_one_member_with_a_nan_cell_bias(pkg, ctx, oracle, lstm, lfx):
    """the NaN member gives the oracle's NaN pattern; the plain member's bits are those of its solo run and of the oracle"""
    w, h, nf = 200, 136, 3
    cblob = ev.base_blob(oracle)
    ctx.load_blob(cblob)
    ctx.set_thresholds(*THR)
    plain, bad = ev.base_lstm_blob(lstm), lfx["lstm_cell_bias_o_nan"]
    lums = [np.stack([ev.picture(w, h, seed=30 + 5 * m + t, resi=True) for t in range(nf)]) for m in range(2)]
    ctx.load_lstm_blob(plain)
    solo = ctx.ldp_sequence(lums[0], w, h, nf, QP, i_frame_first=1).copy()
    solo_state = ctx.ldp_get_state(w, h).copy()
    with pkg.LdpGroup(ctx, 2) as g:
        g.load_lstm_blob(0, plain)
        g.load_lstm_blob(1, bad)
        got = g.sequence(lums, w, h, [QP, QP])
        assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), solo.view(np.uint32)), "the plain member's bits changed"
        assert np.array_equal(np.ascontiguousarray(g.get_state(0)).view(np.uint32).reshape(-1), solo_state.view(np.uint32).reshape(-1))
        assert np.isfinite(got[0]).all()
        for m, lb in enumerate((plain, bad)):
            st = None
            with np.errstate(all="ignore"):
                for t in range(nf):
                    p, st = lstm.lstm_step(lb, oracle.resi_vectors(cblob, lums[m][t], w, h), st, QP, 1 + t, THR[0], THR[1], mode=0)
                    _assert_same(got[m][t], p, "member %d frame %d" % (m, t))
            _assert_same(g.get_state(m), st, "member %d: state" % m)
        assert np.isnan(got[1]).any()


# ------------------------------------------------------------------------------------------------ the 16-bit plans
@pytest.mark.parametrize("plan", [2, 3])
def test_fast_plans_accept_within_tolerance_or_refuse(pkg, oracle, cnn, plan):
    """The assertion shape of test_load_time_accuracy_guard_with_adversarial_weights on the edge fixtures: either the load-time guard
    accepts the plan and the output has the oracle's NaN pattern and is within 1e-4 of it elsewhere, or the plan is refused
    (ETHCNN_ERR_PLAN_REFUSED or ETHCNN_ERR_ARG), nothing is written, and the same context still matches the oracle under plan 0.
    Non-finite weights must be refused.  The tiny-weight fixtures probe the small side of the fp16 scales."""
    e = pkg.ethcnn
    w, h, frames = 1280, 768, 1                    # 240 CTUs: the multi-launch path, where the plans apply
    ctus = ev.mixed_ctus(240, seed=12)
    luma = ctus.reshape(12, 20, 64, 64).transpose(0, 2, 1, 3).reshape(h, w)
    seen = {}
    c = pkg.EthCnn(device=0)                       # one context for all fixtures: every weight load is judged anew
    try:
        c.set_small_pass_launch(False)
        c.set_thresholds(*THR)
        for name in CNN_NAMES:
            blob = cnn[name]
            with np.errstate(all="ignore"):
                want = oracle.predict_frames(blob, luma, w, h, frames, QP, THR[0], THR[1], mode=0)
            c.set_fc1_plan(0)
            c.load_blob(blob)
            refused = None
            try:
                accepted = c.check_fc1_plan(plan)["accepted"]
            except e.EthCnnError as err:
                assert err.code == e.ERR_ARG, (name, err.code)
                accepted, refused = False, err.code
            if accepted:
                c.set_fc1_plan(plan)
                got = c.predict_luma(luma, w, h, frames, QP)
                assert np.array_equal(np.isnan(got), np.isnan(want)), name
                ok = ~np.isnan(want)
                assert np.array_equal(got[ok] == 0.0, want[ok] == 0.0), name
                assert np.abs(got[ok] - want[ok]).max() <= TOL, (name, float(np.abs(got[ok] - want[ok]).max()))
            else:
                try:
                    c.set_fc1_plan(plan)
                    with pytest.raises(e.EthCnnError) as ei:
                        c.predict_luma(luma, w, h, frames, QP)
                    refused = ei.value.code
                except e.EthCnnError as err:       # refused at the switch already
                    refused = err.code
                assert refused in (e.ERR_PLAN_REFUSED, e.ERR_ARG), (name, refused)
                c.set_fc1_plan(0)
                _assert_same(c.predict_luma(luma, w, h, frames, QP), want, name + ": plan 0 after the refusal")
            seen[name] = "accepted" if accepted else "refused %d" % refused
            if not np.isfinite(blob).all():
                assert not accepted, "%s: a non-finite weight must be refused" % name
    finally:
        c.close()
        print("plan", plan, seen)
