"""-m gpu: the cell clip of the inference recurrences (k_lstm through lstm_step, the sequence and group recurrences), reached from the
zero state a real sequence starts from and asserted to have happened.  The other LSTM tests hit the clip only where they pass a random
c in [-5, 5] as state_in.  Bundles: the reference's trained QP-32 bundle and synth_lstm_blob(22, 3.0), both with pushed biases
(tests/train_edges.push_lstm_biases, every 8th unit, amt 3.0: on the CPU, in float64, all of those units sit at +-5 after 10 frames,
6.25 % of the c words on each side, with these vectors and with the residual CNN's; no larger amt was needed).  No state_in anywhere."""
import functools

import numpy as np
import pytest

import train_edges as E

pytestmark = pytest.mark.gpu
AMT = 3.0
QP = 32
SHARE = 0.02


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d words differ, max |d| = %g" % (what, int((_bits(got) != _bits(want)).sum()), np.abs(got - want).max())


def _inputs(rng, n, scale):
    """the vectors of tests/test_gpu_lstm.py"""
    vec = (np.abs(rng.standard_normal((n, 448))) * scale).astype(np.float32)
    vec[:, ::7] *= -0.2
    return vec


def _frames(seed, w, h, nf):
    """residual-like luma with quieter bands that move from frame to frame (tests/test_gpu_ldp_sequence.py)"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(nf, h, w), dtype=np.uint8)
    for t in range(nf):
        r0 = (t * h // nf) // 2
        out[t, r0: r0 + h // 2] = (out[t, r0: r0 + h // 2] // (8 << (t % 3)) + 120).astype(np.uint8)
    return out


@pytest.fixture(scope="module")
def lstm(oracle):
    import ethcnn_lstm_np
    return ethcnn_lstm_np


@functools.lru_cache(maxsize=None)
def _bundle(kind):
    import ethcnn_lstm_np
    plain = E.golden_lstm_blob() if kind == "real" else ethcnn_lstm_np.synth_lstm_blob(22, 3.0)
    return E.push_lstm_biases(plain, every=8, amt=AMT)[0], plain


def _census(c, what):
    """the share of c words that are exactly +5 and exactly -5"""
    c = np.asarray(c)
    hi, lo = float((c == 5).mean()), float((c == -5).mean())
    print("%s: %.2f %% of the c words are +5, %.2f %% are -5" % (what, 100 * hi, 100 * lo))
    assert hi >= SHARE and lo >= SHARE, "%s: clipped shares %.4f / %.4f" % (what, hi, lo)


@pytest.mark.parametrize("kind", ["real", "seeded"])
@pytest.mark.parametrize("n,scale", [(16, 1.0), (45, 0.5)])
def test_ten_steps_from_the_zero_state_reach_the_clip(ctx, lstm, kind, n, scale):
    blob, _ = _bundle(kind)
    ctx.load_lstm_blob(blob)
    rng = np.random.default_rng(n)
    vecs = [_inputs(rng, n, scale) for _ in range(10)]
    s64 = None
    for i_frame, vec in enumerate(vecs, 1):  # float64 first: the inputs do clip
        _, s64 = lstm.lstm_forward64(blob, vec, s64, QP, i_frame)
    _census(s64[:, 0], "float64 chain")
    g_state = o_state = s64 = None
    for i_frame, vec in enumerate(vecs, 1):
        ctx.set_thresholds(-1.0, -1.0)  # gates open: raw probabilities against float64
        raw_p, _ = ctx.lstm_step(vec, g_state, QP, i_frame)
        p64, s64 = lstm.lstm_forward64(blob, vec, s64, QP, i_frame)
        ctx.set_thresholds(0.5, 0.5)
        got_p, g_state = ctx.lstm_step(vec, g_state, QP, i_frame)
        want_p, o_state = lstm.lstm_step(blob, vec, o_state, QP, i_frame, 0.5, 0.5, mode=0)
        _same(g_state, o_state, "state after step %d" % i_frame)
        _same(got_p, want_p, "probabilities of step %d" % i_frame)
        print("step %2d: probs %.3e  state %.3e from float64" % (i_frame, np.abs(raw_p - p64).max(), np.abs(g_state - s64).max()))
        assert np.abs(raw_p - p64).max() <= 1e-4 and np.abs(g_state - s64).max() <= 1e-4, i_frame
    _census(g_state[:, 0], "state after step 10")


@pytest.fixture(params=["real", "seeded"])
def seq(request, pkg, oracle):
    c = pkg.EthCnn(device=0)
    c.load_blob(oracle.synth_blob(21, 1.0))
    c.load_lstm_blob(_bundle(request.param)[0])
    c.set_thresholds(0.5, 0.5)
    c.kind = request.param
    yield c
    c.close()


def test_sequence_equals_the_step_loop_with_the_clip_active(seq, oracle, lstm):
    w, h, nf = 416, 240, 12
    lum = _frames(416, w, h, nf)
    blob, s64 = _bundle(seq.kind)[0], None
    cblob = seq.get_blob()
    for t in range(nf):  # float64 first, on the residual CNN's vectors: they do not keep the push from clipping
        _, s64 = lstm.lstm_forward64(blob, oracle.resi_vectors(cblob, lum[t], w, h).reshape(-1, 448), s64, QP, 1 + t)
    _census(s64[:, 0], "float64 chain")
    want_p = np.stack([seq.ldp_step(lum[t], w, h, QP, 1 + t).copy() for t in range(nf)])
    want_s = seq.ldp_get_state(w, h)
    _census(want_s[:, 0], "ldp_step loop, final state")
    got_p = seq.ldp_sequence(lum, w, h, nf, QP, i_frame_first=1)
    _same(got_p, want_p, "probabilities")
    _same(seq.ldp_get_state(w, h), want_s, "final state")


def test_ldp_group_of_a_pushed_and_a_plain_member(pkg, ctx, oracle):
    """K = 2: member 0 has the pushed real bundle, member 1 the plain one; each equals ldp_sequence on a context with its bundle"""
    w, h, nf = 416, 240, 12
    lums = [_frames(416, w, h, nf), _frames(417, w, h, nf)]
    blobs = list(_bundle("real"))
    qps = [QP, 27]
    ctx.load_blob(oracle.synth_blob(21, 1.0))
    ctx.set_thresholds(0.5, 0.5)
    solo = []
    for m in range(2):
        ctx.load_lstm_blob(blobs[m])
        solo.append((ctx.ldp_sequence(lums[m], w, h, nf, qps[m], i_frame_first=1).copy(), ctx.ldp_get_state(w, h)))
    with pkg.LdpGroup(ctx, 2) as g:
        for m in range(2):
            g.load_lstm_blob(m, blobs[m])
        got = g.sequence(lums, w, h, qps, i_frame_first=1)
        for m in range(2):
            _same(got[m], solo[m][0], "member %d: probabilities" % m)
            _same(g.get_state(m), solo[m][1], "member %d: final state" % m)
        _census(g.get_state(0)[:, 0], "pushed member, final state")
        assert not (np.abs(g.get_state(1)[:, 0]) == 5).any()
