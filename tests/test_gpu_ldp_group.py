"""-m gpu: K Low-Delay-P residual sequences through one recurrence launch (include/ethcnn.h "config #5 offline, group form") against
the definition: member m's probabilities and resident state are what ethcnn_ldp_sequence_device gives on a context loaded with m's
bundle, for m's input and QP.  Every comparison is array_equal on the raw 32-bit words.  Bundles are seeded, with a seed, head gain
and QP of their own per member; one member of one case is the reference's real QP-32 bundle.  That call runs the group's kernels as
a group of one, so the block and member arithmetic is also held to the per-frame ethcnn_ldp_step loop and to the CPU oracle.

Shapes: the smallest at which a part of the block mapping can go wrong -- 1 CTU; 12 CTUs (one ragged 16-CTU group); 17 (a full group
and a ragged one: the level-32 block owns both, the level-64 block has two surplus groups); 65 (a second level-64 block with one
group of four); 1056 (the gates' second 1024-CTU mini-batch).  Frames 1, 2, 5 (parity of the h double buffer, the i_frame % 4 wrap);
i_frame_first 0, 1, 3 (a run split at frame 1 inside the call); K 1, 2, 3, 4, 8."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldp_buffers import frames as _frames

import replay_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
DRIVER = os.path.join(ROOT, "hevc-complexity-reduction_amd", "resi_video_to_cu_depth_LDP.py")
ERR_ARG, ERR_NOWEIGHTS = -1, -5
# (LSTM seed, head gain, QP) per member position; "real" stands for the reference's bundle
BUNDLES = [(41, 3.0, 22), (42, 0.5, 37), (43, 6.0, 27), (44, 1.0, 32), (45, 2.0, 24), (46, 4.0, 35), (47, 1.5, 30), (48, 5.0, 40)]
REAL_B = ("real", None, 32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d words differ, max |d| = %g" % (what, int((_bits(got) != _bits(want)).sum()), np.abs(got - want).max())


def _state(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-5, 5, (n, 448)), rng.uniform(-1, 1, (n, 448))], 1).astype(np.float32)


def _nctu(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def _load_ctx(c, b):
    if b[0] == "real":
        c.load_lstm_checkpoint(REAL)
    else:
        c.load_lstm_synthetic(b[0], b[1])


def _load_member(g, m, b):
    if b[0] == "real":
        g.load_lstm_checkpoint(m, REAL)
    else:
        g.load_lstm_synthetic(m, b[0], b[1])


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    c = pkg.EthCnn(device=0)
    c.load_blob(oracle.synth_blob(21, 1.0))
    c.set_thresholds(0.5, 0.5)
    yield c
    c.close()


def _solo(c, b, lum, w, h, first, state_in=None, resident=False):
    """the reference: ldp_sequence_device on the context loaded with the member's bundle -> (probs, final state).  resident: continue
    from whatever state the context holds"""
    nf, n = lum.shape[0], _nctu(w, h)
    if not resident:
        _load_ctx(c, b)
    d_l, d_p = c.alloc(lum.size), c.alloc(nf * n * 21 * 4)
    d_s = None
    try:
        d_l.upload(lum)
        if state_in is not None:
            d_s = c.alloc(state_in.nbytes)
            d_s.upload(state_in)
        c.ldp_sequence_device(d_l, w, h, nf, b[2], first, d_p, d_state_in=d_s)
        return d_p.download(np.float32, nf * n * 21).reshape(nf, n, 21), c.ldp_get_state(w, h)
    finally:
        c.synchronize()
        for x in (d_l, d_p, d_s):
            if x is not None:
                x.free()


def _group(pkg, c, bundles):
    g = pkg.LdpGroup(c, len(bundles))
    for m, b in enumerate(bundles):
        _load_member(g, m, b)
    return g


# (width, height, frames, i_frame_first, bundles)
CASES = [
    (64, 64, 1, 1, BUNDLES[:1]),
    (64, 64, 5, 0, BUNDLES[2:4]),
    (200, 136, 2, 1, BUNDLES[:2]),
    (200, 136, 5, 3, [BUNDLES[4], REAL_B, BUNDLES[0]]),
    (1088, 64, 5, 0, BUNDLES[:4]),
    (1088, 64, 1, 3, BUNDLES[5:7]),
    (832, 320, 2, 1, BUNDLES),
    (4160, 64, 5, 1, BUNDLES[1:4]),
    (2112, 2048, 3, 1, BUNDLES[:2]),
]


@pytest.mark.parametrize("w,h,nf,first,bundles", CASES, ids=["%dx%d-f%d-i%d-k%d" % (c[0], c[1], c[2], c[3], len(c[4])) for c in CASES])
def test_every_member_equals_its_solo_call(pkg, ctx, w, h, nf, first, bundles):
    n, k = _nctu(w, h), len(bundles)
    lums = [_frames(1000 + 10 * w + m, w, h, nf) for m in range(k)]
    sins = [_state(70 + m, n) for m in range(k)] if first > 1 else None
    want = [_solo(ctx, b, lums[m], w, h, first, sins[m] if sins else None) for m, b in enumerate(bundles)]
    with _group(pkg, ctx, bundles) as g:
        got = g.sequence(lums, w, h, [b[2] for b in bundles], i_frame_first=first, state_ins=sins)
        for m in range(k):
            _same(got[m], want[m][0], "member %d: probabilities" % m)
            _same(g.get_state(m), want[m][1], "member %d: state" % m)


_LOOPS = {}  # (width, height, member) -> (frames, probabilities, final state) of the per-frame loop: computed once, never changed


def _loop(c, w, h, m):
    """the definition, independent of the sequence kernels: ethcnn_ldp_step frame after frame from i_frame 0 on the context loaded
    with member m's bundle (tests/test_gpu_ldp_sequence.py) -> (frames, probabilities, final state)"""
    if (w, h, m) not in _LOOPS:
        b, lum = BUNDLES[m], _frames(2000 + 10 * w + m, w, h, 5)
        _load_ctx(c, b)
        probs = np.stack([c.ldp_step(lum[t], w, h, b[2], t).copy() for t in range(5)])
        _LOOPS[(w, h, m)] = (lum, probs, c.ldp_get_state(w, h))
    return _LOOPS[(w, h, m)]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 64), (1088, 64)])
def test_every_member_equals_its_per_frame_loop(pkg, ctx, w, h, k):
    """The solo call runs the group's kernel as a group of one, so "member equals solo" does not hold the kernel's member and block
    arithmetic to anything of its own: this does.  64x64: 1 CTU, one ragged column group, every level's block has surplus slots;
    1088x64: 17 CTUs, a second column group with one valid column, surplus column groups in the level-32 and level-64 blocks.  Five
    frames from i_frame 0: runs of 1 + 4 frames, the state zeroed twice."""
    loops = [_loop(ctx, w, h, m) for m in range(k)]
    with _group(pkg, ctx, BUNDLES[:k]) as g:
        got = g.sequence([lp[0] for lp in loops], w, h, [b[2] for b in BUNDLES[:k]], i_frame_first=0)
        for m in range(k):
            _same(got[m], loops[m][1], "member %d of %d: probabilities" % (m, k))
            _same(g.get_state(m), loops[m][2], "member %d of %d: state" % (m, k))


def test_a_member_moved_and_four_equal_members(pkg, ctx):
    w, h, nf = 1088, 64, 2
    bundles = BUNDLES[:3]
    lums = [_frames(300 + m, w, h, nf) for m in range(3)]
    with _group(pkg, ctx, bundles) as g:
        a = g.sequence(lums, w, h, [b[2] for b in bundles])
    order = [2, 0, 1]
    with _group(pkg, ctx, [bundles[j] for j in order]) as g:
        b = g.sequence([lums[j] for j in order], w, h, [bundles[j][2] for j in order])
    for pos, j in enumerate(order):
        _same(b[pos], a[j], "member %d at position %d" % (j, pos))
    want, _ = _solo(ctx, bundles[0], lums[0], w, h, 1)
    _same(a[0], want, "member 0 against its solo call")
    with _group(pkg, ctx, [bundles[1]] * 4) as g:
        four = g.sequence([lums[1]] * 4, w, h, [bundles[1][2]] * 4)
    for m in range(4):
        _same(four[m], a[1], "equal member %d" % m)


def test_gates_close_for_one_member_and_stay_open_for_another(pkg, ctx):
    """thresholds (0.6, 0.85), chosen on the CPU (oracle lstm_step on these frames with open gates): the y64 maxima of member 0 are
    0.81 / 0.74 / 0.77, of member 1 below 0.53, of member 2 0.58 on frame 0 and 0.99 afterwards; member 2's y32 maximum on frame 1 is
    0.81.  So on frame 0 the first gate closes for members 1 and 2 and stays open for member 0, and member 2's second gate closes on
    frame 1 -- asserted on the solo results before anything is compared."""
    w, h, nf = 200, 136, 3
    bundles = BUNDLES[:3]
    lums = [_frames(500 + m, w, h, nf) for m in range(3)]
    ctx.set_thresholds(0.6, 0.85)
    try:
        want = [_solo(ctx, b, lums[m], w, h, 1)[0] for m, b in enumerate(bundles)]
        assert (want[1][0][:, 1:] == 0).all() and (want[2][0][:, 1:] == 0).all(), "first gate closed on frame 0 for members 1 and 2"
        assert (want[0][0][:, 1:5] != 0).any() and (want[0][0][:, 5:] != 0).any(), "both gates open on frame 0 for member 0"
        assert (want[2][1][:, 1:5] != 0).any() and (want[2][1][:, 5:] == 0).all(), "second gate closed on frame 1 for member 2"
        with _group(pkg, ctx, bundles) as g:
            got = g.sequence(lums, w, h, [b[2] for b in bundles])
        for m in range(3):
            _same(got[m], want[m], "member %d" % m)
    finally:
        ctx.set_thresholds(0.5, 0.5)


def test_states_given_resident_continued_and_chunked(pkg, ctx):
    w, h, nf = 1088, 64, 5
    n = _nctu(w, h)
    bundles = BUNDLES[:2]
    qps = [b[2] for b in bundles]
    lums = [_frames(600 + m, w, h, nf) for m in range(2)]
    whole = [_solo(ctx, b, lums[m], w, h, 1) for m, b in enumerate(bundles)]
    with _group(pkg, ctx, bundles) as g:
        # two calls in a row equal one call
        first = g.sequence([a[:2] for a in lums], w, h, qps, i_frame_first=1)
        rest = g.sequence([a[2:] for a in lums], w, h, qps, i_frame_first=3)
        for m in range(2):
            _same(np.concatenate([first[m], rest[m]]), whole[m][0], "member %d: two calls" % m)
            _same(g.get_state(m), whole[m][1], "member %d: state after two calls" % m)
        # a state for member 1, the resident one for member 0
        sin = _state(9, n)
        g.sequence([a[:2] for a in lums], w, h, qps, i_frame_first=1)
        mixed = g.sequence([a[2:] for a in lums], w, h, qps, i_frame_first=3, state_ins=[None, sin])
        _same(mixed[0], whole[0][0][2:], "member 0 continues from its resident state")
        want1 = _solo(ctx, bundles[1], lums[1][2:], w, h, 3, state_in=sin)
        _same(mixed[1], want1[0], "member 1 starts from the given state")
        _same(g.get_state(1), want1[1], "member 1: state")
        # chunk 2 over 5 frames equals unchunked
        g.set_chunk_frames(2)
        chunked = g.sequence(lums, w, h, qps, i_frame_first=1)
        for m in range(2):
            _same(chunked[m], whole[m][0], "member %d: chunk 2" % m)
            _same(g.get_state(m), whole[m][1], "member %d: state, chunk 2" % m)


def test_a_chunked_group_from_frame_zero_and_its_continuation(pkg, ctx):
    """K = 3 from i_frame_first 0, four frames in chunks of 3: the recurrence launches fall at frame 0 (a run of its own), at frame 1
    (the state zeroed again) and at the chunk boundary (frame 3, from the resident state).  200x136: 12 CTUs, one ragged column
    group; then, in the same group (its state buffers grow), 1088x64: 17 CTUs, two column groups with the second ragged.  Then the
    group goes on at frame 4 from its resident states.  The reference is the solo call per member: of the first four frames for
    the first call, frames 4 onward of a run of six for the second."""
    bundles = BUNDLES[:3]
    qps = [b[2] for b in bundles]
    with _group(pkg, ctx, bundles) as g:
        g.set_chunk_frames(3)
        for w, h in ((200, 136), (1088, 64)):
            lums = [_frames(1200 + 10 * w + m, w, h, 6) for m in range(3)]
            head = [_solo(ctx, b, lums[m][:4], w, h, 0) for m, b in enumerate(bundles)]
            whole = [_solo(ctx, b, lums[m], w, h, 0) for m, b in enumerate(bundles)]
            got = g.sequence([a[:4] for a in lums], w, h, qps, i_frame_first=0)
            for m in range(3):
                _same(got[m], head[m][0], "%dx%d, member %d: frames 0..3" % (w, h, m))
                _same(g.get_state(m), head[m][1], "%dx%d, member %d: state behind frame 3" % (w, h, m))
            got = g.sequence([a[4:] for a in lums], w, h, qps, i_frame_first=4)
            for m in range(3):
                _same(got[m], whole[m][0][4:], "%dx%d, member %d: frames 4..5 from the resident state" % (w, h, m))
                _same(g.get_state(m), whole[m][1], "%dx%d, member %d: state behind frame 5" % (w, h, m))


def test_the_context_keeps_its_bundle_and_state(pkg, ctx):
    w, h = 200, 136
    own = BUNDLES[7]
    lum = _frames(700, w, h, 5)
    whole, _ = _solo(ctx, own, lum, w, h, 1)
    head, state2 = _solo(ctx, own, lum[:2], w, h, 1)
    blob = ctx.get_lstm_blob()
    with _group(pkg, ctx, BUNDLES[:2]) as g:
        g.sequence([_frames(701 + m, w, h, 3) for m in range(2)], w, h, [22, 37])
        _same(ctx.ldp_get_state(w, h), state2, "the context's resident state behind a group call")
        assert np.array_equal(_bits(ctx.get_lstm_blob()), _bits(blob))
        tail, _ = _solo(ctx, own, lum[2:], w, h, 3, resident=True)
    _same(np.concatenate([head, tail]), whole, "solo calls around a group call")


def test_group_against_the_oracle(pkg, ctx, oracle):
    import ethcnn_lstm_np as lstm
    w, h, nf = 200, 136, 3
    bundles = [BUNDLES[3], BUNDLES[0]]
    lums = [_frames(800 + m, w, h, nf) for m in range(2)]
    cblob = ctx.get_blob()
    with _group(pkg, ctx, bundles) as g:
        got = g.sequence(lums, w, h, [b[2] for b in bundles])
        for m, b in enumerate(bundles):
            lblob, st = g.get_lstm_blob(m), None
            assert np.array_equal(_bits(lblob), _bits(lstm.synth_lstm_blob(b[0], b[1])))
            for t in range(nf):
                vec = oracle.resi_vectors(cblob, lums[m][t], w, h).reshape(-1, 448)
                p, st = lstm.lstm_step(lblob, vec, st, b[2], 1 + t, 0.5, 0.5, mode=0)
                _same(got[m][t], p, "member %d, frame %d" % (m, t))
            _same(g.get_state(m), st, "member %d: state" % m)


def test_refusals_enqueue_nothing_and_keep_the_states(pkg, ctx):
    w, h, nf = 200, 136, 2
    n = _nctu(w, h)

    def refused(fn, code):
        with pytest.raises(pkg.EthCnnError) as e:
            fn()
        assert e.value.code == code and str(e.value).split(":", 1)[1].strip(), str(e.value)
        return str(e.value)

    for k in (0, 9):
        refused(lambda: pkg.LdpGroup(ctx, k), ERR_ARG)
    lums = [_frames(900 + m, w, h, nf) for m in range(2)]
    d_l, d_p = [ctx.alloc(a.size) for a in lums], [ctx.alloc(nf * n * 21 * 4) for _ in range(2)]
    mark = np.full(nf * n * 21, 7.0, np.float32)

    def untouched():
        ctx.synchronize()
        return all(np.array_equal(b.download(np.float32, mark.size), mark) for b in d_p)

    try:
        for b, a in zip(d_l, lums):
            b.upload(a)
        for b in d_p:
            b.upload(mark)
        with pkg.LdpGroup(ctx, 2) as g:
            g.load_lstm_synthetic(0, 41, 3.0)
            assert "member 1" in refused(lambda: g.sequence_device(d_l, w, h, nf, [22, 37], 1, d_p), ERR_NOWEIGHTS)
            refused(lambda: g.load_lstm_blob(1, np.zeros(1000, np.float32)), ERR_ARG)
            refused(lambda: g.load_lstm_blob(2, g.get_lstm_blob(0)), ERR_ARG)
            assert "member 1" in refused(lambda: g.sequence_device(d_l, w, h, nf, [22, 37], 1, d_p), ERR_NOWEIGHTS)
            g.load_lstm_synthetic(1, 42, 0.5)
            refused(lambda: g.sequence_device(d_l, w, h, nf, [22, 37], 3, d_p), ERR_ARG)  # no resident state yet
            refused(lambda: g.sequence_device(d_l, w, h, 0, [22, 37], 1, d_p), ERR_ARG)
            refused(lambda: g.sequence_device(d_l, w, h, nf, [22, 37], -1, d_p), ERR_ARG)
            refused(lambda: g.sequence_device([d_l[0], None], w, h, nf, [22, 37], 1, d_p), ERR_ARG)
            refused(lambda: g.sequence_device(d_l, w, h, nf, [22, 37], 1, d_p, pitch=w - 1), ERR_ARG)
            refused(lambda: g.get_state(0), ERR_ARG)
            assert untouched()
            g.sequence_device(d_l, w, h, nf, [22, 37], 1, d_p)
            states = [g.get_state(m) for m in range(2)]
            for b in d_p:
                b.upload(mark)
            # the resident states belong to 12 CTUs: another geometry cannot continue from them
            refused(lambda: g.sequence_device(d_l, 136, 136, 1, [22, 37], 3, d_p), ERR_ARG)
            assert untouched()
            for m in range(2):
                _same(g.get_state(m), states[m], "member %d: state behind the refusals" % m)
    finally:
        ctx.synchronize()
        for b in d_l + d_p:
            b.free()


# ---------------------------------------------------------------------------------------------------------------------- replay ---
RUNS = ((0, 128, 64, 1, 3), (1, 192, 128, 2, 2))  # seq, width, height, first frame number, frames
SLOT_QPS = (22, 27, 32, 37)


def _records():
    """an inter record set by hand: two sequences of different geometry, four QP slots, records in reverse order"""
    rng = np.random.default_rng(91)
    recs = []
    for seq, w, h, f0, nf in RUNS:
        for f in range(f0, f0 + nf):
            for line in range(h // 64):
                for col in range(w // 64):
                    r = np.full(replay_ref.REC, 255, np.uint8)
                    r[2:6] = np.array([w, h], "<u2").view(np.uint8)
                    r[10:14] = np.array([f], "<u4").view(np.uint8)
                    r[14:20] = np.array([line, col, seq], "<u2").view(np.uint8)
                    for s, qp in enumerate(SLOT_QPS):
                        at = replay_ref.SLOT_BASE + replay_ref.SLOT_BYTES * s
                        r[at] = qp
                        r[at + 1:at + 17] = rng.integers(0, 4, 16)
                        r[at + 17:at + 17 + 4096] = rng.integers(0, 256, 4096)
                    recs.append(r)
    return np.stack(recs[::-1])


def test_replay_of_several_slots_equals_the_replay_of_each(pkg, ctx):
    rec = _records()
    plan = replay_ref.plan(rec)
    assert [(r["w"], r["h"], r["f0"], r["frames"]) for r in plan] == [(128, 64, 1, 3), (192, 128, 2, 2)]
    bundles = BUNDLES[:4]  # member / slot s: its own bundle
    with pkg.Replay(ctx) as rp:
        rp.open(rec)
        want = []
        for i in range(len(plan)):
            want.append([])
            for s in range(4):
                _load_ctx(ctx, bundles[s])
                want[-1].append(rp.run(i, s))
                resi, labels = replay_ref.planes(rec, plan[i], s)
                assert np.array_equal(want[-1][-1][1], labels)
        with _group(pkg, ctx, bundles) as g4, _group(pkg, ctx, [bundles[2], bundles[0]]) as g2:
            for chunk in (0, 1):
                rp.set_chunk_frames(chunk)
                for i in range(len(plan)):
                    got = rp.run_group(i, [0, 1, 2, 3], g4)
                    for s in range(4):
                        _same(got[s][0], want[i][s][0], "run %d, slot %d, chunk %d" % (i, s, chunk))
                        assert np.array_equal(got[s][1], want[i][s][1])
                    got = rp.run_group(i, [2, 0], g2)
                    for j, s in enumerate((2, 0)):
                        _same(got[j][0], want[i][s][0], "run %d, slots [2, 0], slot %d, chunk %d" % (i, s, chunk))
                        assert np.array_equal(got[j][1], want[i][s][1])
            # the records, four slots' planes of a chunk (1 frame of 6 CTUs), the source table, the zero state (the run starts at frame 2)
            assert rp.run_group_bytes(1, 4) == rec.nbytes + 4 * 1 * 6 * 4096 + 2 * 6 * 8 + 6 * 3584
            with pytest.raises(pkg.EthCnnError) as e:
                rp.run_group(0, [0, 1, 2], g4)
            assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------- driver ---
def _write_resi(path, lum):
    nf, h, w = lum.shape
    with open(path, "wb") as f:
        for k in range(nf + 1):  # frame 0 is the intra picture
            f.write((lum[k - 1] if k else np.zeros((h, w), np.uint8)).tobytes())
            f.write(np.full(w * h // 2, 128, np.uint8).tobytes())


def test_driver_with_two_sequences(tmp_path):
    import shutil
    w, h = 200, 136
    a, b, short = str(tmp_path / "resi_32.yuv"), str(tmp_path / "resi_22.yuv"), str(tmp_path / "short.yuv")
    _write_resi(a, _frames(31, w, h, 4))
    _write_resi(b, _frames(32, w, h, 4))
    _write_resi(short, _frames(33, w, h, 3))
    for ext in (".index", ".data-00000-of-00001"):
        shutil.copy(REAL + ext, str(tmp_path / ("model_LDP_200000_qp32.dat" + ext)))  # QP 32: the real bundle; QP 22: seeded
    env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="21")

    def run(*args):
        return subprocess.run([sys.executable, DRIVER] + [str(x) for x in args] + ["--model-dir", str(tmp_path)], capture_output=True, text=True,
                              env=env, timeout=300)

    out = {k: str(tmp_path / (k + ".dat")) for k in ("a1", "b1", "a2", "b2", "bad")}
    for r in (run(a, w, h, 32, "--out", out["a1"]), run(b, w, h, 22, "--out", out["b1"]),
              run(a, w, h, 32, "--out", out["a2"], "--also", b, 22, out["b2"])):
        assert r.returncode == 0, r.stderr[-800:]
    assert os.path.getsize(out["a1"]) == 4 * 12 * 21 * 4
    assert open(out["a2"], "rb").read() == open(out["a1"], "rb").read()
    assert open(out["b2"], "rb").read() == open(out["b1"], "rb").read()
    r = run(a, w, h, 32, "--out", out["bad"], "--also", short, 22, out["bad"] + ".2")
    assert r.returncode != 0 and "frame" in r.stderr
    assert not os.path.exists(out["bad"]) and not os.path.exists(out["bad"] + ".2")
