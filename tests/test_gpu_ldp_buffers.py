"""-m gpu: the Low-Delay-P chain's device entries (ethcnn_resi_vectors_device, ethcnn_lstm_step_device, ethcnn_ldp_sequence_device,
ethcnn_ldp_group_sequence_device, ethcnn_ldp_batch_run_device) and the host entry ethcnn_ldp_sequence on the buffers a caller really
has: luma at a pitch, a frame stride and a byte offset of its own, outputs at their smallest legal alignment inside guard bands,
inputs inside two different poisons, members' buffers back to back in one allocation ("Caller-owned buffers
the suite reaches"; helpers and case lists: tests/ldp_buffers.py).

The reference is the definition in include/ethcnn.h: ethcnn_ldp_step frame after frame on PACKED host frames, on a context that
holds the member's bundle; one case also runs against the CPU oracle.  Every comparison is equality of 32-bit words."""
import os

import numpy as np
import pytest

import ldp_buffers as lb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
ERR_ARG = -1
NF = 5
# (LSTM seed, head gain, QP) per bundle; "real" stands for the reference's QP-32 bundle
BUNDLES = [(41, 3.0, 22), ("real", None, 32), (43, 6.0, 27)]
PROBS_LEAD = lb.GUARD + 4    # 4-byte aligned, not 16-byte aligned: the smallest alignment d_probs and d_vec (front-end) may have
STATE_LEAD = lb.GUARD + 16   # 16-byte aligned, not 32-byte aligned: the smallest a state or the step's d_vec may have


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d words differ, max |d| = %g" % (what, int((_bits(got) != _bits(want)).sum()), np.abs(got - want).max())


def _load_ctx(c, b):
    if b[0] == "real":
        c.load_lstm_checkpoint(REAL)
    else:
        c.load_lstm_synthetic(b[0], b[1])


def _load_place(obj, i, b):
    if b[0] == "real":
        obj.load_lstm_checkpoint(i, REAL)
    else:
        obj.load_lstm_synthetic(i, b[0], b[1])


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    c = pkg.EthCnn(device=0)
    c.load_blob(oracle.synth_blob(21, 1.0))
    c.set_thresholds(0.5, 0.5)
    c.bundle = None
    yield c
    c.close()


def _use(c, bi):
    if c.bundle != bi:
        _load_ctx(c, BUNDLES[bi])
        c.bundle = bi


_LOOPS = {}  # (seed, w, h, nf, first, bundle) -> (frames, state_in, probabilities, final state): computed once, never changed


def _loop(c, seed, w, h, nf, first, bi=0):
    """the definition: ethcnn_ldp_step frame after frame on the packed frames of lb.frames(seed, ...), frame t carrying first + t, from
    the state lb.state(seed + 1, nctu) when first > 1"""
    key = (seed, w, h, nf, first, bi)
    if key not in _LOOPS:
        _use(c, bi)
        lum = lb.frames(seed, w, h, nf)
        sin = lb.state(seed + 1, lb.nctu(w, h)) if first > 1 else None
        probs = np.stack([c.ldp_step(lum[t], w, h, BUNDLES[bi][2], first + t, state_in=sin if t == 0 else None).copy() for t in range(nf)])
        _LOOPS[key] = (lum, sin, probs, c.ldp_get_state(w, h))
    return _LOOPS[key]


class _Bufs(object):
    """device allocations of one test, freed together"""

    def __init__(self, c):
        self.c, self.held = c, []

    def guarded(self, *a, **kw):
        self.held.append(lb.guarded(self.c, *a, **kw))
        return self.held[-1]

    def alloc(self, nbytes):
        self.held.append(self.c.alloc(nbytes))
        return self.held[-1]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.c.synchronize()
        for x in self.held:
            x.free()


def _luma_on_device(bufs, host_bytes):
    d = bufs.alloc(host_bytes.size)
    d.upload(host_bytes)
    return d


# ------------------------------------------------------------------------------------------------------- geometry, solo ---
@pytest.mark.parametrize("w,h", lb.SHAPES[:4], ids=["%dx%d" % s for s in lb.SHAPES[:4]])
def test_solo_entries_at_a_callers_pitch_stride_and_offset(ctx, w, h):
    """ethcnn_ldp_sequence_device and ethcnn_ldp_sequence over the 36 layouts of lb.solo_geometries: each with both poisons in the
    bytes that are no pixels, the device entry's d_probs inside guards at a 4-byte aligned address.  Chunks of 2 frames put the second
    and third chunk at f0 * frame_stride, with a stride that is neither w * h nor pitch * h."""
    n, seed = lb.nctu(w, h), 7000 + w
    try:
        for pitch, fs, off, chunk, first in lb.solo_geometries(w, h):
            lum, sin, want_p, want_s = _loop(ctx, seed, w, h, NF, first)
            _use(ctx, 0)
            ctx.ldp_set_sequence_chunk(chunk)
            what = "pitch %d, stride %d, offset %d, chunk %d, first %d" % (pitch, fs, off, chunk, first)
            for fill in lb.LUMA_FILL:
                host = lb.lay_out(lum, pitch, fs, off, fill)
                with _Bufs(ctx) as bufs:
                    d_l = _luma_on_device(bufs, host)
                    d_p = bufs.guarded(NF * n * 21 * 4, lead=PROBS_LEAD)
                    d_s = None
                    if sin is not None:
                        d_s = bufs.guarded(sin.nbytes, lead=STATE_LEAD, pattern=lb.NAN_WORD if fill == lb.LUMA_FILL[0] else lb.ALT_WORD)
                        d_s.upload(sin)
                    ctx.ldp_sequence_device(d_l.ptr + off, w, h, NF, BUNDLES[0][2], first, d_p.ptr, d_state_in=d_s.ptr if d_s else None,
                                            pitch=pitch, frame_stride=fs)
                    got = lb.check_guards(d_p, what=what).reshape(NF, n, 21)
                    _same(got, want_p, "device entry, fill %#x, %s: probabilities" % (fill, what))
                    _same(ctx.ldp_get_state(w, h), want_s, "device entry, fill %#x, %s: state" % (fill, what))
                got = ctx.ldp_sequence(host[off:], w, h, NF, BUNDLES[0][2], i_frame_first=first, state_in=sin, pitch=pitch, frame_stride=fs)
                _same(got, want_p, "host entry, fill %#x, %s: probabilities" % (fill, what))
                _same(ctx.ldp_get_state(w, h), want_s, "host entry, fill %#x, %s: state" % (fill, what))
    finally:
        ctx.ldp_set_sequence_chunk(0)


def test_a_pitched_sequence_against_the_oracle(ctx, oracle):
    """203x77 at pitch 210, stride 210 * 77 + 13, offset 5, chunks of 2: the oracle's front-end on the pitched planes themselves
    (oracle.resi_vectors(..., pitch=)) and its LSTM step, frame after frame"""
    import ethcnn_lstm_np as lstm
    w, h, pitch, off = 203, 77, 210, 5
    fs, n = pitch * h + 13, lb.nctu(w, h)
    host, lum = lb.pitched(7300, w, h, NF, pitch, fs, off, lb.LUMA_FILL[0])
    _use(ctx, 0)
    cblob, lblob = ctx.get_blob(), ctx.get_lstm_blob()
    ctx.ldp_set_sequence_chunk(2)
    try:
        with _Bufs(ctx) as bufs:
            d_l = _luma_on_device(bufs, host)
            d_p = bufs.guarded(NF * n * 21 * 4, lead=PROBS_LEAD)
            ctx.ldp_sequence_device(d_l.ptr + off, w, h, NF, BUNDLES[0][2], 1, d_p.ptr, pitch=pitch, frame_stride=fs)
            got = lb.check_guards(d_p).reshape(NF, n, 21)
    finally:
        ctx.ldp_set_sequence_chunk(0)
    st = None
    for t in range(NF):
        vec = oracle.resi_vectors(cblob, host[off + t * fs:], w, h, pitch=pitch).reshape(-1, 448)
        p, st = lstm.lstm_step(lblob, vec, st, BUNDLES[0][2], 1 + t, 0.5, 0.5, mode=0)
        _same(got[t], p, "frame %d" % t)
    _same(ctx.ldp_get_state(w, h), st, "final state")


# ------------------------------------------------------------------------------------------------- guards on outputs, solo ---
@pytest.mark.parametrize("w,h", lb.SHAPES, ids=["%dx%d" % s for s in lb.SHAPES])
def test_solo_probabilities_and_state_inside_guards(ctx, w, h):
    """two frames from a given state: d_probs [2][nctu][21] at a 4-byte aligned address between guards, d_state_in with exactly nctu
    rows at a 16-byte aligned address between two different poisons (the lanes of a ragged 16-CTU group must not read past row
    nctu - 1 into a value); pitched luma at a byte offset"""
    n, nf, first, pitch, off = lb.nctu(w, h), 2, 3, w + 7, 5
    fs = pitch * h + 13
    lum, sin, want_p, want_s = _loop(ctx, 7100 + w, w, h, nf, first)
    _use(ctx, 0)
    for fill, poison in zip(lb.LUMA_FILL, (lb.NAN_WORD, lb.ALT_WORD)):
        with _Bufs(ctx) as bufs:
            d_l = _luma_on_device(bufs, lb.lay_out(lum, pitch, fs, off, fill))
            d_p = bufs.guarded(nf * n * 21 * 4, lead=PROBS_LEAD)
            d_s = bufs.guarded(sin.nbytes, lead=STATE_LEAD, pattern=poison)
            d_s.upload(sin)
            ctx.ldp_sequence_device(d_l.ptr + off, w, h, nf, BUNDLES[0][2], first, d_p.ptr, d_state_in=d_s.ptr, pitch=pitch, frame_stride=fs)
            _same(lb.check_guards(d_p, what="d_probs").reshape(nf, n, 21), want_p, "poison %#x: probabilities" % poison)
            _same(lb.check_guards(d_s, what="d_state_in").reshape(n, 2, 448), sin, "poison %#x: d_state_in is an input" % poison)
            _same(ctx.ldp_get_state(w, h), want_s, "poison %#x: state" % poison)


# ------------------------------------------------------------------------------------------------------------- group ---
@pytest.mark.parametrize("first,chunk", [(3, 2), (0, 0)])
def test_group_members_back_to_back_in_one_allocation(pkg, ctx, first, chunk):
    """K = 3 at 1088x64 (17 CTUs), a common padded pitch and stride; every member's luma at its own byte offset inside ONE allocation,
    all d_probs back to back in ONE guarded allocation that starts 4-byte aligned, all d_state_in back to back in another: a member that
    writes or reads one row too many meets its neighbour or a guard"""
    w, h, k = 1088, 64, 3
    n, pitch = lb.nctu(w, h), w + 7
    fs = pitch * h + pitch * (h // 2)
    offs = (1, 5, 15)
    loops = [_loop(ctx, 7200 + m, w, h, NF, first, m) for m in range(k)]
    pb, sb = NF * n * 21 * 4, n * 2 * 448 * 4
    outs = []
    with pkg.LdpGroup(ctx, k) as g:
        for m in range(k):
            _load_place(g, m, BUNDLES[m])
        g.set_chunk_frames(chunk)
        for fill, poison in zip(lb.LUMA_FILL, (lb.NAN_WORD, lb.ALT_WORD)):
            planes = [lb.lay_out(loops[m][0], pitch, fs, offs[m], fill) for m in range(k)]
            base = np.cumsum([0] + [p.size for p in planes])
            with _Bufs(ctx) as bufs:
                d_l = _luma_on_device(bufs, np.concatenate(planes))
                d_p = bufs.guarded(k * pb, lead=PROBS_LEAD)
                d_s = None
                if first > 1:
                    d_s = bufs.guarded(k * sb, lead=STATE_LEAD, pattern=poison)
                    d_s.upload(np.concatenate([loops[m][1].reshape(-1) for m in range(k)]))
                g.sequence_device([d_l.ptr + int(base[m]) + offs[m] for m in range(k)], w, h, NF, [BUNDLES[m][2] for m in range(k)], first,
                                  [d_p.ptr + m * pb for m in range(k)], [d_s.ptr + m * sb for m in range(k)] if d_s else None, pitch=pitch,
                                  frame_stride=fs)
                got = lb.check_guards(d_p, what="the members' d_probs").reshape(k, NF, n, 21)
                for m in range(k):
                    _same(got[m], loops[m][2], "fill %#x, member %d: probabilities" % (fill, m))
                    _same(g.get_state(m), loops[m][3], "fill %#x, member %d: state" % (fill, m))
                outs.append(got)
    _same(outs[0], outs[1], "the two poisons")


# ------------------------------------------------------------------------------------------------------------- batch ---
# (width, height, pitch - width, frame stride - pitch * height, offset, frames, i_frame_first, bundle)
BATCH = [(203, 77, 7, 13, 1, 5, 3, 0), (1088, 64, 64, 1152 * 32, 5, 3, 1, 1), (200, 136, 1, 13, 15, 1, 2, 2), (64, 64, 7, 71 * 32, 5, 4, 1, 0)]


def test_batch_sequences_back_to_back_in_one_allocation(pkg, ctx):
    """four sequences, each with its own size, pitch, stride, offset, length and first frame number, in chunks of 2 frames (members
    drop out between launches, every chunk start is f0 * the sequence's own stride).  All d_probs lie back to back in table order in
    ONE guarded allocation, the two given d_state_in in another: adjacent is not overlapping, the call must accept it."""
    loops = [_loop(ctx, 7400 + j, w, h, nf, first, bi) for j, (w, h, dp, ds, off, nf, first, bi) in enumerate(BATCH)]
    ns = [lb.nctu(q[0], q[1]) for q in BATCH]
    pbytes = [q[5] * n * 21 * 4 for q, n in zip(BATCH, ns)]
    given = [j for j, q in enumerate(BATCH) if q[6] > 1]
    assert given == [0, 2]
    p_at, s_at = np.cumsum([0] + pbytes), np.cumsum([0] + [ns[j] * 2 * 448 * 4 for j in given])
    outs = []
    with pkg.LdpBatch(ctx, len(BUNDLES)) as b:
        for i, bd in enumerate(BUNDLES):
            _load_place(b, i, bd)
        b.set_chunk(2)
        for fill, poison in zip(lb.LUMA_FILL, (lb.NAN_WORD, lb.ALT_WORD)):
            planes = [lb.lay_out(loops[j][0], q[0] + q[2], (q[0] + q[2]) * q[1] + q[3], q[4], fill) for j, q in enumerate(BATCH)]
            l_at = np.cumsum([0] + [p.size for p in planes])
            with _Bufs(ctx) as bufs:
                d_l = _luma_on_device(bufs, np.concatenate(planes))
                d_p = bufs.guarded(int(p_at[-1]), lead=PROBS_LEAD)
                d_s = bufs.guarded(int(s_at[-1]), lead=STATE_LEAD, pattern=poison)
                d_s.upload(np.concatenate([loops[j][1].reshape(-1) for j in given]))
                seqs = []
                for j, (w, h, dp, ds, off, nf, first, bi) in enumerate(BATCH):
                    seqs.append({"d_luma": d_l.ptr + int(l_at[j]) + off, "width": w, "height": h, "pitch": w + dp, "frame_stride": (w + dp) * h + ds,
                                 "nframes": nf, "qp": BUNDLES[bi][2], "i_frame_first": first, "bundle": bi, "d_probs": d_p.ptr + int(p_at[j]),
                                 "d_state_in": d_s.ptr + int(s_at[given.index(j)]) if j in given else None})
                try:
                    b.run_device(seqs)
                except pkg.EthCnnError as e:
                    pytest.fail("buffers that lie back to back were refused: %s" % e)
                got = lb.check_guards(d_p, what="the sequences' d_probs")
                outs.append(got)
                for j, q in enumerate(BATCH):
                    _same(got[p_at[j] // 4: p_at[j + 1] // 4].reshape(q[5], ns[j], 21), loops[j][2], "fill %#x, sequence %d: probabilities" % (fill, j))
                    _same(b.get_state(j), loops[j][3], "fill %#x, sequence %d: state" % (fill, j))
    _same(outs[0], outs[1], "the two poisons")


# ----------------------------------------------------------------------------------------------- ethcnn_lstm_step_device ---
@pytest.mark.parametrize("n", [1, 17, 1056])
def test_lstm_step_device_inside_guards(ctx, n):
    """every buffer of the step with exactly n rows inside guards, at its smallest legal alignment; the guards around the INPUTS hold
    two different poisons in turn: a read past row n - 1 would decide a value.  With and without a given state."""
    _use(ctx, 0)
    qp = BUNDLES[0][2]
    rng = np.random.default_rng(7500 + n)
    vec = rng.uniform(-2, 2, (n, 448)).astype(np.float32)
    for sin, i_frame in ((lb.state(7600 + n, n), 3), (None, 1)):
        want_p, want_s = ctx.lstm_step(vec, sin, qp, i_frame)
        outs = []
        for poison in (lb.NAN_WORD, lb.ALT_WORD):
            with _Bufs(ctx) as bufs:
                d_v = bufs.guarded(vec.nbytes, lead=STATE_LEAD, pattern=poison)
                d_v.upload(vec)
                d_si = None
                if sin is not None:
                    d_si = bufs.guarded(sin.nbytes, lead=STATE_LEAD, pattern=poison)
                    d_si.upload(sin)
                d_so = bufs.guarded(n * 2 * 448 * 4, lead=STATE_LEAD)
                d_p = bufs.guarded(n * 21 * 4, lead=PROBS_LEAD)
                ctx._chk(ctx.lib.ethcnn_lstm_step_device(ctx.h, d_v.ptr, d_si.ptr if d_si else None, n, qp, i_frame, d_so.ptr, d_p.ptr))
                got_p = lb.check_guards(d_p, what="d_probs").reshape(n, 21)
                got_s = lb.check_guards(d_so, what="d_state_out").reshape(n, 2, 448)
                _same(lb.check_guards(d_v, what="d_vec").reshape(n, 448), vec, "d_vec is an input")
                if d_si:
                    _same(lb.check_guards(d_si, what="d_state_in").reshape(n, 2, 448), sin, "d_state_in is an input")
            _same(got_p, want_p, "i_frame %d, poison %#x: probabilities" % (i_frame, poison))
            _same(got_s, want_s, "i_frame %d, poison %#x: state" % (i_frame, poison))
            outs.append((got_p, got_s))
        _same(outs[0][0], outs[1][0], "the two poisons: probabilities")
        _same(outs[0][1], outs[1][1], "the two poisons: state")


# -------------------------------------------------------------------------------------------- ethcnn_resi_vectors_device ---
@pytest.mark.parametrize("w,h", [(203, 77), (1088, 64)])
def test_resi_vectors_device_inside_guards(ctx, oracle, w, h):
    """d_vec [nctu][448] at a 4-byte aligned address between guards (FC1 computes whole 16-row tiles), a pitched plane at a byte offset
    with both poisons, against the oracle on the packed plane"""
    n, pitch, off = lb.nctu(w, h), w + 7, 5
    lum = lb.frames(7700 + w, w, h, 1)
    want = oracle.resi_vectors(ctx.get_blob(), lum[0], w, h).reshape(n, 448)
    for fill in lb.LUMA_FILL:
        with _Bufs(ctx) as bufs:
            d_l = _luma_on_device(bufs, lb.lay_out(lum, pitch, pitch * h, off, fill))
            d_v = bufs.guarded(n * 448 * 4, lead=PROBS_LEAD)
            ctx._chk(ctx.lib.ethcnn_resi_vectors_device(ctx.h, d_l.ptr + off, w, h, pitch, d_v.ptr))
            _same(lb.check_guards(d_v, what="d_vec").reshape(n, 448), want, "fill %#x" % fill)


# ------------------------------------------------------------------------------------------ staging pieces, host entry ---
def test_host_entry_stages_a_chunk_in_more_than_two_pieces(pkg, oracle):
    """ethcnn_ldp_sequence stages luma in pieces of pf = min(chunk, 64 MB / frame_stride) frames through two buffers in turn.  416x240
    with a frame stride of a third of 64 MB: pf = 3, and 7 frames in one chunk are pieces of 3, 3 and 1 frames -- the second piece's
    vectors go behind the first one's, the third piece waits for the first buffer to be free again.  Everything between the frames
    is poison."""
    w, h, nf, pitch, first = 416, 240, 7, 416 + 7, 1
    fs = lb.STAGE_BYTES // 3
    pf = lb.STAGE_BYTES // fs
    assert pf == 3 and nf > 2 * pf, "the shape must give a third piece"
    n = lb.nctu(w, h)
    assert nf <= (256 << 20) // (n * 448 * 4), "one chunk"
    c = pkg.EthCnn(device=0)
    try:
        c.load_blob(oracle.synth_blob(21, 1.0))
        c.set_thresholds(0.5, 0.5)
        _load_ctx(c, BUNDLES[0])
        host, lum = lb.pitched(7800, w, h, nf, pitch, fs, 0, lb.LUMA_FILL[0])
        want_p = np.stack([c.ldp_step(lum[t], w, h, BUNDLES[0][2], first + t).copy() for t in range(nf)])
        want_s = c.ldp_get_state(w, h)
        got = c.ldp_sequence(host, w, h, nf, BUNDLES[0][2], i_frame_first=first, pitch=pitch, frame_stride=fs)
        _same(got, want_p, "probabilities")
        _same(c.ldp_get_state(w, h), want_s, "state")
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------- alignment refusals ---
def _refusal_case(pkg, ctx, bufs, entry):
    """a small valid call of `entry` on raw addresses -> (call(ptrs) -> None or EthCnnError, ptrs, outputs [(name, Guarded)], obj);
    one CTU, two frames from a given state; the group and the batch with two members, of which member 1's pointer is the one moved"""
    w, h, nf, first, n = 64, 64, 2, 3, 1
    qp = BUNDLES[0][2]
    lum, sin = lb.frames(7900, w, h, nf), lb.state(7901, n)
    _use(ctx, 0)
    if entry == "ethcnn_resi_vectors_device":
        d_l, d_v = _luma_on_device(bufs, lum[0]), bufs.guarded(n * 448 * 4)
        ptrs = {"d_luma": d_l.ptr, "d_vec": d_v.ptr}
        return (lambda p: ctx._chk(ctx.lib.ethcnn_resi_vectors_device(ctx.h, p["d_luma"], w, h, w, p["d_vec"]))), ptrs, [("d_vec", d_v)], None
    if entry == "ethcnn_lstm_step_device":
        d_v, d_si, d_so, d_p = bufs.guarded(n * 448 * 4), bufs.guarded(sin.nbytes), bufs.guarded(sin.nbytes), bufs.guarded(n * 21 * 4)
        d_v.upload(np.ones((n, 448), np.float32))
        d_si.upload(sin)
        ptrs = {"d_vec": d_v.ptr, "d_state_in": d_si.ptr, "d_state_out": d_so.ptr, "d_probs": d_p.ptr}
        call = lambda p: ctx._chk(ctx.lib.ethcnn_lstm_step_device(ctx.h, p["d_vec"], p["d_state_in"], n, qp, first, p["d_state_out"], p["d_probs"]))
        return call, ptrs, [("d_state_out", d_so), ("d_probs", d_p)], None
    k = 1 if entry == "ethcnn_ldp_sequence_device" else 2
    d_l = _luma_on_device(bufs, np.concatenate([lum] * k))
    d_s, d_p = bufs.guarded(k * sin.nbytes), bufs.guarded(k * nf * n * 21 * 4)
    d_s.upload(np.concatenate([sin] * k))
    ptrs = {"d_luma": d_l.ptr + (k - 1) * lum.size, "d_state_in": d_s.ptr + (k - 1) * sin.nbytes, "d_probs": d_p.ptr + (k - 1) * nf * n * 21 * 4}
    if entry == "ethcnn_ldp_sequence_device":
        call = lambda p: ctx.ldp_sequence_device(p["d_luma"], w, h, nf, qp, first, p["d_probs"], d_state_in=p["d_state_in"])
        return call, ptrs, [("d_probs", d_p)], None
    if entry == "ethcnn_ldp_group_sequence_device":
        g = pkg.LdpGroup(ctx, 2)
        for m in range(2):
            _load_place(g, m, BUNDLES[0])
        call = lambda p: g.sequence_device([d_l.ptr, p["d_luma"]], w, h, nf, [qp, qp], first, [d_p.ptr, p["d_probs"]], [d_s.ptr, p["d_state_in"]])
        return call, ptrs, [("d_probs", d_p)], g
    assert entry == "ethcnn_ldp_batch_run_device"
    b = pkg.LdpBatch(ctx, 1)
    _load_place(b, 0, BUNDLES[0])
    seq = lambda l, s, p: {"d_luma": l, "width": w, "height": h, "nframes": nf, "qp": qp, "i_frame_first": first, "bundle": 0, "d_state_in": s, "d_probs": p}
    call = lambda p: b.run_device([seq(d_l.ptr, d_s.ptr, d_p.ptr), seq(p["d_luma"], p["d_state_in"], p["d_probs"])])
    return call, ptrs, [("d_probs", d_p)], b


def _resident(ctx, obj, entry):
    if entry == "ethcnn_ldp_sequence_device":
        return [ctx.ldp_get_state(64, 64)]
    if obj is not None:
        return [obj.get_state(j) for j in range(2)]
    return []


@pytest.mark.parametrize("entry,pointer,align", lb.REFUSAL_ROWS, ids=["%s-%s" % (r[0][7:], r[1]) for r in lb.REFUSAL_ROWS])
def test_a_pointer_below_its_alignment_is_refused(pkg, ctx, entry, pointer, align):
    """the refusal only: ETHCNN_ERR_ARG with the argument's name in the text, nothing written, the resident states as they were, and the
    same call with the pointer where it belongs still right.  No kernel is ever launched on a pointer below its documented alignment."""
    name = pointer.replace("seqs[j].", "").replace("[m]", "")
    with _Bufs(ctx) as bufs:
        call, ptrs, outputs, obj = _refusal_case(pkg, ctx, bufs, entry)
        try:
            call(ptrs)
            ctx.synchronize()
            want = [lb.check_guards(g, what=nm).copy() for nm, g in outputs]
            states = _resident(ctx, obj, entry)
            marks = [lb.pattern_bytes(lb.NAN_WORD, g.nbytes) for nm, g in outputs]
            for step in {16: (4, 8, 1), 4: (1, 2)}[align]:
                for (nm, g), mark in zip(outputs, marks):
                    g.upload(mark)
                with pytest.raises(pkg.EthCnnError) as e:
                    call(dict(ptrs, **{name: ptrs[name] + step}))
                assert e.value.code == ERR_ARG and name in str(e.value) and "%d-byte aligned" % align in str(e.value), (step, str(e.value))
                for (nm, g), mark in zip(outputs, marks):
                    assert np.array_equal(lb.check_guards(g, np.uint8, what=nm), mark), "%s + %d: %s was written" % (name, step, nm)
                for a, b in zip(_resident(ctx, obj, entry), states):
                    _same(a, b, "%s + %d: a resident state behind the refusal" % (name, step))
            call(ptrs)
            for (nm, g), w_ in zip(outputs, want):
                _same(lb.check_guards(g, what=nm), w_, "%s behind the refusals" % nm)
        finally:
            ctx.synchronize()
            if obj is not None:
                obj.close()
