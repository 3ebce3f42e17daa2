"""-m gpu: the gate thresholds as a property of a sequence (include/ethcnn.h: ethcnn_ldp_sessions_set_thresholds, ethcnn_ldp_set_thresholds_batch / _group).
Every result is held against TWO expectations, word for word:
  1. the solo entry (ethcnn_ldp_step for sessions, ethcnn_ldp_sequence_device for batch and group) on a context of its own that holds
     the bundle and, through ethcnn_set_thresholds, the sequence's resolved pair -- state included;
  2. tests/gates_ref.py, the numpy restatement of the reference's two tf.cond gates per 1024-CTU mini-batch, applied to the output of an
     open-gate run (set_thresholds(-1, -1)) of the same frames.
Thresholds are taken FROM that open-gate output, so the zero patterns are known in advance and the tests assert them.

CNN seed 21; bundles (LSTM seed 42, head gain 0.5, QP 37), whose y64 lies around 0.5, and (41, 3.0, QP 22), which saturates -- those of
tests/test_gpu_ldp_sessions.py.  Pictures are ldp_buffers.frames of the seeds below.  The big picture is seed 6000 at 2560x1920 (1200
CTUs: a mini-batch of 1024 and a ragged one of 176), picked with the CPU oracle (oracle resi_vectors + lstm_step with open gates; seeds
6000..6003 tried, 6000 is the first that fits): with bundle 0 its first frame has max y64 0.4970468 in mini-batch 0 and 0.49649906 in
mini-batch 1, max y32 0.5454109 and 0.5459473.  So thr1 = 0.49649906 EXACTLY closes the first gate in mini-batch 1 alone (strict >), and
thr2 = 0.5454109 exactly closes the second gate in mini-batch 0 alone; the tests assert these facts on the GPU's own output before
they rely on them."""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import gates_ref
import ldp_buffers as lb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
DRIVER = os.path.join(ROOT, "hevc-complexity-reduction_amd", "resi_video_to_cu_depth_LDP.py")
GOLD = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
ERR_ARG = -1
BUNDLES = [(42, 0.5, 37), (41, 3.0, 22)]  # (LSTM seed, head gain, QP)
BIG_SEED, BIG_W, BIG_H = 6000, 2560, 1920
OPEN = (-1.0, -1.0)
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d words differ, max |d| = %g" % (what, int((_bits(got) != _bits(want)).sum()), np.abs(got - want).max())


def _pair(t1, t2):
    """a pair as the library holds it: two float32 values, as Python floats"""
    return float(f32(t1)), float(f32(t2))


def _below(x):
    return float(np.nextafter(f32(x), f32(0)))


def _above(x):
    return float(np.nextafter(f32(x), f32(2)))


def _gated(open_probs, pair):
    """expectation 2: the reference's gates on an open-gate output [frames, n, 21] or [n, 21]"""
    a = np.asarray(open_probs, dtype=np.float32)
    n = a.shape[-2]
    return gates_ref.gate_frames(a.reshape(-1, 21), n, pair[0], pair[1]).reshape(a.shape)


def _pattern(p):
    """per 1024-CTU mini-batch of one frame [n, 21]: (y32 survived, y16 survived)"""
    return [(bool((p[c:c + 1024, 1:5] != 0).any()), bool((p[c:c + 1024, 5:] != 0).any())) for c in range(0, p.shape[0], 1024)]


def _make_ctx(pkg, oracle):
    c = pkg.EthCnn(device=0)
    c.load_blob(oracle.synth_blob(21, 1.0))
    c.set_thresholds(0.5, 0.5)
    return c


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    c = _make_ctx(pkg, oracle)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(pkg, oracle):
    """the solo contexts: the same CNN, one per bundle; every solo call sets its thresholds first"""
    out = []
    for seed, gain, qp in BUNDLES:
        c = _make_ctx(pkg, oracle)
        c.load_lstm_synthetic(seed, gain)
        out.append(c)
    yield out
    for c in out:
        c.close()


def _solo_step(ref, pair, luma, w, h, qp, i_frame, state_in=None):
    """expectation 1 for a session: ethcnn_ldp_step on the solo context under `pair` -> (probs, state)"""
    ref.set_thresholds(*pair)
    p = ref.ldp_step(luma, w, h, qp, i_frame, state_in).copy()
    return p, ref.ldp_get_state(w, h)


def _solo_seq(ref, pair, lum, w, h, qp, first, state_in=None):
    """expectation 1 for batch and group: ethcnn_ldp_sequence_device on the solo context under `pair` -> (probs, state)"""
    nf, n = lum.shape[0], lb.nctu(w, h)
    ref.set_thresholds(*pair)
    ref.ldp_set_sequence_chunk(0)
    d_l, d_p, d_s = ref.alloc(lum.size), ref.alloc(nf * n * 21 * 4), None
    try:
        d_l.upload(lum)
        if state_in is not None:
            d_s = ref.alloc(state_in.nbytes)
            d_s.upload(state_in)
        ref.ldp_sequence_device(d_l, w, h, nf, qp, first, d_p, d_state_in=d_s)
        return d_p.download(np.float32, nf * n * 21).reshape(nf, n, 21), ref.ldp_get_state(w, h)
    finally:
        ref.synchronize()
        for x in (d_l, d_p, d_s):
            if x is not None:
                x.free()


def _sessions(pkg, c):
    s = pkg.LdpSessions(c, len(BUNDLES))
    for i, (seed, gain, qp) in enumerate(BUNDLES):
        s.load_lstm_synthetic(i, seed, gain)
    return s


def _dev_step(s, c, frames):
    """step_device with packed pictures: uploads, steps, downloads -> [probs]"""
    bufs, dev, ns = [], [], []
    alloc = lambda nbytes: bufs.append(c.alloc(max(int(nbytes), 4))) or bufs[-1]
    try:
        for f in frames:
            luma = np.ascontiguousarray(f["luma"], dtype=np.uint8)
            n = lb.nctu(luma.shape[1], luma.shape[0])
            d = {k: f[k] for k in ("session", "qp", "i_frame", "bundle")}
            d["d_luma"] = alloc(luma.size)
            d["d_luma"].upload(luma)
            d["d_probs"] = alloc(n * 21 * 4)
            dev.append(d)
            ns.append(n)
        s.step_device(dev)
        c.synchronize()
        return [d["d_probs"].download(np.float32, n * 21).reshape(n, 21) for d, n in zip(dev, ns)]
    finally:
        c.synchronize()
        for b in bufs:
            b.free()


def _host_step(s, c, frames):
    return s.step(frames)


# --------------------------------------------------------------------------------------------------- five sessions in one step ---
# (width, height, bundle, picture seed); the pairs come from the open-gate outputs (_world)
SESS = [(BIG_W, BIG_H, 0, BIG_SEED), (BIG_W, BIG_H, 0, BIG_SEED), (208, 144, 1, 6001), (416, 240, 1, 6002), (208, 144, 0, 6003)]
_W = {}  # pictures, open-gate outputs, states and pairs of SESS: computed once, never changed


def _world(refs):
    if _W:
        return _W
    lums = [lb.frames(seed, w, h, 3)[:2] for (w, h, bi, seed) in SESS]  # (the big one is frames 1, 2 of the batch test's sequence)
    opened, states = [], []
    for j, (w, h, bi, seed) in enumerate(SESS):
        p0, s0 = _solo_step(refs[bi], OPEN, lums[j][0], w, h, BUNDLES[bi][2], 1)
        p1, s1 = _solo_step(refs[bi], OPEN, lums[j][1], w, h, BUNDLES[bi][2], 2, s0)
        opened.append([p0, p1])
        states.append([s0, s1])
    big = opened[0][0]
    m = [float(big[:1024, 0].max()), float(big[1024:, 0].max())]
    q = [float(big[:1024, 1:5].max()), float(big[1024:, 1:5].max())]
    # the precondition the seed was picked for: mini-batch 0 holds the larger y64, and the two y32 maxima differ
    assert m[0] > m[1] and q[0] != q[1], (m, q)
    lo = min(q)
    pairs = [_pair(m[1], lo),            # thr1 EXACTLY the largest y64 of mini-batch 1: closed there, open in mini-batch 0
             _pair(_below(m[1]), lo),    # the next float below: open in both
             _pair(2.0, -1.0),           # y32 zeroed, y16 KEPT: behind a closed first gate the second sees zeros, and 0 > -1
             _pair(-1.0, _above(max(float(p[:, 1:5].max()) for p in opened[3]))),  # thr2 above every y32: only y16 zeroed
             None]                       # inherits the context's
    a, b = _pattern(_gated(big, pairs[0])), _pattern(_gated(big, pairs[1]))
    closed2 = q.index(lo)  # the mini-batch whose y32 maximum IS thr2
    assert a[0][0] and a[1] == (False, False), a
    assert b[0][0] and b[1][0] and b[closed2][1] is False and b[1 - closed2][1] is True, (b, q)
    assert _pattern(_gated(opened[2][0], pairs[2])) == [(False, True)] and _pattern(_gated(opened[3][0], pairs[3])) == [(True, False)]
    _W.update(lums=lums, opened=opened, states=states, pairs=pairs, solo={})
    return _W


def _check(refs, W, got, state, j, t, pair, what):
    """frame t of session j under `pair` against both expectations; state: the session's resident state behind it, or None"""
    w, h, bi, seed = SESS[j]
    key = (j, t, pair)
    if key not in W["solo"]:
        W["solo"][key] = _solo_step(refs[bi], pair, W["lums"][j][t], w, h, BUNDLES[bi][2], t + 1, W["states"][j][0] if t else None)
    want, want_state = W["solo"][key]
    _same(got, want, "%s: session %d, frame %d under (%r, %r): against the solo step" % ((what, j, t + 1) + pair))
    _same(got, _gated(W["opened"][j][t], pair), "%s: session %d, frame %d under (%r, %r): against the gate rule" % ((what, j, t + 1) + pair))
    _same(want_state, W["states"][j][t], "the gates do not touch the state")
    if state is not None:
        _same(state, want_state, "%s: session %d: state behind frame %d" % (what, j, t + 1))


@pytest.mark.parametrize("step", [_dev_step, _host_step], ids=["step_device", "step"])
def test_five_sessions_with_pairs_of_their_own(pkg, ctx, refs, step):
    W = _world(refs)
    frame = lambda j, t: {"session": j, "luma": W["lums"][j][t], "qp": BUNDLES[SESS[j][2]][2], "i_frame": t + 1, "bundle": SESS[j][2]}
    try:
        with _sessions(pkg, ctx) as s:
            assert [s.open(w, h) for (w, h, bi, seed) in SESS] == [0, 1, 2, 3, 4]
            for j, pair in enumerate(W["pairs"]):
                if pair is not None:
                    s.set_thresholds(j, *pair)
                    assert s.thresholds_of(j) == pair + (1,)
            assert s.thresholds_of(4) == (0.5, 0.5, 0)
            ctx.set_thresholds(*OPEN)
            assert s.thresholds_of(4) == OPEN + (0,) and s.thresholds_of(0) == W["pairs"][0] + (1,)
            at = lambda j, t1: W["pairs"][j] or t1
            # all five, the same five in another order, a subset of three: frame 1 each time (it starts from zeros), so every call
            # must give the same words; the pair follows the session id, not the row
            for order in ([0, 1, 2, 3, 4], [3, 1, 4, 0, 2], [4, 1, 2]):
                got = step(s, ctx, [frame(j, 0) for j in order])
                for pos, j in enumerate(order):
                    _check(refs, W, got[pos], s.get_state(j), j, 0, at(j, OPEN), "order %r" % (order,))
                if order[0] == 0:
                    first = [g.copy() for g in got]
                    assert _pattern(first[0]) != _pattern(first[1]), "the two big sessions differ in their pairs only"
                    assert _pattern(first[4]) == [(True, True)]
            # the context's pair changes between two steps: only the inheriting session follows
            ctx.set_thresholds(2.0, 2.0)
            assert s.thresholds_of(4) == (2.0, 2.0, 0) and s.thresholds_of(3) == W["pairs"][3] + (1,)
            order = [2, 0, 4, 3, 1]
            got = step(s, ctx, [frame(j, 1) for j in order])
            for pos, j in enumerate(order):
                _check(refs, W, got[pos], s.get_state(j), j, 1, at(j, (2.0, 2.0)), "behind the context's change")
            assert _pattern(got[2]) == [(False, False)] and _pattern(got[0]) == [(False, True)] and _pattern(got[3]) == [(True, False)]
            # close and open of the same id: the pair is forgotten, the session inherits
            s.close(2)
            assert s.open(208, 144) == 2 and s.thresholds_of(2) == (2.0, 2.0, 0)
            got = step(s, ctx, [frame(2, 0), frame(3, 0)])
            _check(refs, W, got[0], s.get_state(2), 2, 0, (2.0, 2.0), "the reopened id")
            _check(refs, W, got[1], s.get_state(3), 3, 0, W["pairs"][3], "beside the reopened id")
            assert _pattern(got[0]) == [(False, False)], "session 2 had (2, -1) before it was closed: its y16 would have survived"
            s.clear_thresholds(3)
            assert s.thresholds_of(3) == (2.0, 2.0, 0)
    finally:
        ctx.set_thresholds(0.5, 0.5)


def test_the_last_slot_of_32_sessions(pkg, ctx, refs):
    """32 sessions of 208x144 in one step, each with a pair of its own: rows 0 and 31 of the table (and all between)"""
    w, h, k = 208, 144, 32
    lums = [lb.frames(6100 + j, w, h, 1)[0] for j in range(k)]
    opened = [_solo_step(refs[j % 2], OPEN, lums[j], w, h, BUNDLES[j % 2][2], 1) for j in range(k)]
    pairs, kinds = [], []
    for j in range(k):
        m64, m32 = float(opened[j][0][:, 0].max()), float(opened[j][0][:, 1:5].max())
        pairs.append([_pair(m64, -1.0), _pair(_below(m64), m32), _pair(-1.0, _below(m32)), _pair(2.0, 2.0)][j % 4])
        kinds.append([(False, True), (True, False), (True, True), (False, False)][j % 4])
    want = [_solo_step(refs[j % 2], pairs[j], lums[j], w, h, BUNDLES[j % 2][2], 1) for j in range(k)]
    for j in range(k):
        assert _pattern(want[j][0]) == [kinds[j]], (j, pairs[j])
    frame = lambda j: {"session": j, "luma": lums[j], "qp": BUNDLES[j % 2][2], "i_frame": 1, "bundle": j % 2}
    with _sessions(pkg, ctx) as s:
        assert [s.open(w, h) for _ in range(k)] == list(range(k))
        for j in range(k):
            s.set_thresholds(j, *pairs[j])
        # row = session id; rows reversed (row 0 is session 31); three rows, the other 29 slots of the table filled from row 0
        for order in (list(range(k)), list(range(k))[::-1], [31, 0, 17]):
            got = _dev_step(s, ctx, [frame(j) for j in order])
            for pos, j in enumerate(order):
                _same(got[pos], want[j][0], "row %d of %d, session %d: against the solo step" % (pos, len(order), j))
                _same(got[pos], _gated(opened[j][0], pairs[j]), "row %d of %d, session %d: against the gate rule" % (pos, len(order), j))
            for j in (0, 17, 31):
                _same(s.get_state(j), want[j][1], "session %d: state" % j)


# ---------------------------------------------------------------------------------------------------------------------- batch ---
def test_a_batch_with_a_pair_per_sequence_index(pkg, ctx, refs):
    """1200 CTUs x 3 frames from frame 1, 12 x 5 from frame 3, 28 x 2 from frame 2.  In one chunk the gate grid is 6 blocks wide (3 frames
    x 2 mini-batches of the big row); the rows of 5 and 2 blocks return early in the rest.  Under set_chunk(1) it is 2 wide."""
    case = [(BIG_W, BIG_H, 3, 1, 0, BIG_SEED), (208, 144, 5, 3, 1, 6001), (416, 240, 2, 2, 1, 6002)]  # width, height, frames, first, bundle, seed
    lums = [lb.frames(seed, w, h, nf) for (w, h, nf, first, bi, seed) in case]
    sins = [None, lb.state(81, 12), lb.state(82, 28)]
    solo = lambda j, pair: _solo_seq(refs[case[j][4]], pair, lums[j], case[j][0], case[j][1], BUNDLES[case[j][4]][2], case[j][3], sins[j])
    opened = [solo(j, OPEN) for j in range(3)]
    big = opened[0][0][0]
    m1, lo = float(big[1024:, 0].max()), min(float(big[:1024, 1:5].max()), float(big[1024:, 1:5].max()))
    inherited = _pair(-1.0, _above(float(opened[2][0][:, :, 1:5].max())))  # the context's pair: only y16 zeroed
    pairs = [_pair(m1, lo), _pair(2.0, -1.0), inherited]
    want = [solo(j, pairs[j]) for j in range(3)]
    pat = _pattern(want[0][0][0])
    assert pat[0][0] and pat[1] == (False, False), pat
    assert all(_pattern(p) == [(False, True)] for p in want[1][0]) and all(_pattern(p) == [(True, False)] for p in want[2][0])
    assert _pattern(opened[2][0][0]) == [(True, True)]
    for j in range(3):
        _same(want[j][0], _gated(opened[j][0], pairs[j]), "sequence %d: the solo call against the gate rule" % j)
        _same(want[j][1], opened[j][1], "the gates do not touch the state")
    seqs = [{"luma": lums[j], "width": w, "height": h, "qp": BUNDLES[bi][2], "i_frame_first": first, "bundle": bi, "state_in": sins[j]}
            for j, (w, h, nf, first, bi, seed) in enumerate(case)]
    try:
        ctx.set_thresholds(*inherited)
        with pkg.LdpBatch(ctx, len(BUNDLES)) as b:
            for i, (seed, gain, qp) in enumerate(BUNDLES):
                b.load_lstm_synthetic(i, seed, gain)
            b.set_thresholds(0, *pairs[0])
            b.set_thresholds(1, *pairs[1])
            b.set_thresholds(2, *OPEN)
            b.set_thresholds(31, 0.25, 0.75)
            assert [b.thresholds_of(j) for j in (0, 1, 2, 31)] == [pairs[0] + (1,), pairs[1] + (1,), OPEN + (1,), (0.25, 0.75, 1)]
            b.clear_thresholds(2)  # cleared again before the run: it inherits
            assert b.thresholds_of(2) == inherited + (0,) and b.thresholds_of(3) == inherited + (0,)
            for chunk in (1, 0):  # (the pairs are sticky: set once, they hold for both calls)
                b.set_chunk(chunk)
                got = b.run(seqs)
                for j in range(3):
                    _same(got[j], want[j][0], "chunk %d, sequence %d: against the solo call" % (chunk, j))
                    _same(got[j], _gated(opened[j][0], pairs[j]), "chunk %d, sequence %d: against the gate rule" % (chunk, j))
                    _same(b.get_state(j), want[j][1], "chunk %d, sequence %d: state" % (chunk, j))
            assert b.thresholds_of(0) == pairs[0] + (1,)
    finally:
        ctx.set_thresholds(0.5, 0.5)


# ---------------------------------------------------------------------------------------------------------------------- group ---
def test_a_group_with_a_pair_per_member(pkg, ctx, refs):
    w, h, nf = 416, 240, 4
    lums = [lb.frames(6200 + m, w, h, nf) for m in range(2)]
    opened = [_solo_seq(refs[m], OPEN, lums[m], w, h, BUNDLES[m][2], 1) for m in range(2)]
    tops = sorted(float(p[:, 0].max()) for p in opened[0][0])
    assert tops[1] < tops[2], tops
    # member 0: the frames with the two smallest y64 maxima are closed, the two others open; member 1: only y16 zeroed
    pairs = [_pair(tops[1], -1.0), _pair(-1.0, _above(float(opened[1][0][:, :, 1:5].max())))]
    want = [_solo_seq(refs[m], pairs[m], lums[m], w, h, BUNDLES[m][2], 1) for m in range(2)]
    assert sorted(_pattern(p)[0] for p in want[0][0]) == [(False, True)] * 2 + [(True, True)] * 2
    assert all(_pattern(p) == [(True, False)] for p in want[1][0])
    with pkg.LdpGroup(ctx, 2) as g:
        for m, (seed, gain, qp) in enumerate(BUNDLES):
            g.load_lstm_synthetic(m, seed, gain)
        assert g.thresholds_of(1) == (0.5, 0.5, 0)
        for m in range(2):
            g.set_thresholds(m, *pairs[m])
        assert [g.thresholds_of(m) for m in range(2)] == [pairs[0] + (1,), pairs[1] + (1,)]
        for chunk in (0, 3):
            g.set_chunk_frames(chunk)
            got = g.sequence(lums, w, h, [b[2] for b in BUNDLES])
            for m in range(2):
                _same(got[m], want[m][0], "chunk %d, member %d: against the solo call" % (chunk, m))
                _same(got[m], _gated(opened[m][0], pairs[m]), "chunk %d, member %d: against the gate rule" % (chunk, m))
                _same(g.get_state(m), want[m][1], "chunk %d, member %d: state" % (chunk, m))
        g.clear_thresholds(0)  # member 0 under the context's (0.5, 0.5) again, member 1 as before
        got = g.sequence(lums, w, h, [b[2] for b in BUNDLES])
        _same(got[0], _gated(opened[0][0], (0.5, 0.5)), "member 0 cleared: against the gate rule")
        _same(got[1], want[1][0], "member 1 beside the cleared one")


# --------------------------------------------------------------------------------------------------------------------- replay ---
def _records(rng):
    """the four records of a 128x64 x 2-frame inter set (the set of __graft_entry__.smoke)"""
    rec = np.full((2, 2, 16516), 255, dtype=np.uint8)
    for f in range(2):
        for col in range(2):
            r = rec[f, col]
            r[2:6] = np.array([128, 64], "<u2").view(np.uint8)
            r[10:14] = np.array([f + 1], "<u4").view(np.uint8)
            r[14:20] = np.array([0, col, 0], "<u2").view(np.uint8)
            for s, qp in enumerate((22, 27, 32, 37)):
                at = 64 + 4113 * s
                r[at] = qp
                r[at + 1:at + 17] = rng.integers(0, 4, 16)
                r[at + 17:at + 4113] = rng.integers(0, 256, 4096)
    return rec.reshape(4, 16516)


def test_the_feed_entries_need_open_gates(pkg):
    c = pkg.EthCnn(device=0)
    try:
        c.load_synthetic(5, 8.0)
        c.load_lstm_synthetic(6, 3.0)
        c.set_thresholds(0.0, 0.0)
        rec = _records(np.random.default_rng(95))
        with pkg.Replay(c) as rp, pkg.LdpBatch(c, 1) as b, pkg.Calibrator(c) as cal, pkg.PartitionSim(c) as sim, pkg.Calibrator(c) as cal0, \
                pkg.PartitionSim(c) as sim0:
            rp.open(rec)
            b.load_lstm_synthetic(0, 6, 3.0)
            rp.feed(cal0, runs=[0], slot=2)
            rp.feed(sim0, runs=[0], slot=2)
            plain = rp.run_batch([(0, 2, 0)], b)[0][0]
            for index in (5, 0):  # an index the call would not even use, and the one it would
                b.set_thresholds(index, 2.0, 2.0)
                for consumer in (cal, sim):
                    c.synchronize()
                    c.reset_stage_times()
                    with pytest.raises(pkg.EthCnnError) as e:
                        rp.feed(consumer, runs=[0], slot=2, batch=b)
                    assert e.value.code == ERR_ARG and "sequence index %d " % index in str(e.value), str(e.value)
                    c.synchronize()
                    assert sum(c.stage_times()["launches"].values()) == 0, "a refused feed enqueued something"
                assert int(cal.histogram()[0].sum()) == 0 and sim.info()["labelled_ctus"] == 0
                # the device entry uses the batch as it is
                got = rp.run_batch([(0, 2, 0)], b)[0][0]
                _same(got, _gated(plain, (2.0, 2.0)) if index == 0 else plain, "run_batch with a pair on index %d" % index)
                b.clear_thresholds(index)
            rp.feed(cal, runs=[0], slot=2, batch=b)
            rp.feed(sim, runs=[0], slot=2, batch=b)
            assert np.array_equal(cal.histogram(), cal0.histogram()) and int(cal.histogram()[0].sum()) == 4
            assert sim.info() == sim0.info() and sim.info()["labelled_ctus"] == 4
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------ refusals ---
def test_refusals(pkg, ctx):
    fl, it = ctypes.c_float(7.0), ctypes.c_int(7)
    odd = [float("nan"), float("inf"), float("-inf"), 3.0e38, -0.0]
    with _sessions(pkg, ctx) as s, pkg.LdpBatch(ctx, 1) as b, pkg.LdpGroup(ctx, 2) as g:
        sid = s.open(208, 144)
        objs = [(s, "sessions", sid), (b, "batch", 0), (g, "group", 0)]

        def refused(fn, text):
            with pytest.raises(pkg.EthCnnError) as e:
                fn()
            assert e.value.code == ERR_ARG and text in str(e.value), str(e.value)

        # a session that is not open; an index out of range
        for bad in (7, -1, 32):
            for fn in (lambda: s.set_thresholds(bad, 0.5, 0.5), lambda: s.clear_thresholds(bad), lambda: s.thresholds_of(bad)):
                refused(fn, "session %d is not open" % bad)
        for o, bad, word in ((b, 32, "sequence index 32"), (b, -1, "sequence index -1"), (g, 2, "member 2"), (g, -1, "member -1")):
            for fn in (lambda: o.set_thresholds(bad, 0.5, 0.5), lambda: o.clear_thresholds(bad), lambda: o.thresholds_of(bad)):
                refused(fn, word)
        b.set_thresholds(31, 0.5, 0.5)  # the last index is one
        # a value ethcnn_set_thresholds refuses is refused with its code: it refuses no float, and neither do these
        for v in odd:
            assert pkg.ethcnn.load_library().ethcnn_set_thresholds(ctx.h, v, -v) == 0
            held = ctx.get_thresholds()
            for o, form, j in objs:
                o.set_thresholds(j, v, -v)
                got = o.thresholds_of(j)
                assert np.array_equal(_bits(got[:2]), _bits(held)) and got[2] == 1, (form, v)
        ctx.set_thresholds(0.5, 0.5)
        # a null output pointer
        for o, form, j in objs:
            get = o._gates_fn("get")
            for args in ((None, ctypes.byref(fl), ctypes.byref(it)), (ctypes.byref(fl), None, ctypes.byref(it)), (ctypes.byref(fl), ctypes.byref(fl), None)):
                assert get(o.h, j, *args) == ERR_ARG, form
                assert "null output pointer" in o._fn("last_error")(o.h).decode()
            assert fl.value == 7.0 and it.value == 7
            assert o._gates_fn("set")(None, j, 0.5, 0.5) == ERR_ARG
        # during an open streamed call every entry is refused, and the pairs stay what they were
        for o, form, j in objs:
            o.set_thresholds(j, 0.25, 0.75)
        w, h = 416, 240
        pin = ctx.host_buffer(w * h)
        pprobs = ctx.host_buffer(lb.nctu(w, h) * 84).view(np.float32)
        pin[:] = lb.frames(6300, w, h, 1).reshape(-1)
        ctx.predict_luma_begin(pin, w, h, 30, pprobs)
        try:
            ctx.rows_ready(0, 4)
            for o, form, j in objs:
                for fn in (lambda: o.set_thresholds(j, 0.5, 0.5), lambda: o.clear_thresholds(j), lambda: o.thresholds_of(j)):
                    refused(fn, "a streamed call has not been ended")
        finally:
            ctx.predict_luma_end()
        for o, form, j in objs:
            assert o.thresholds_of(j) == (0.25, 0.75, 1), form
        ctx.free_host_buffers()


# --------------------------------------------------------------------------------------------------------------------- server ---
# three directories, two sizes, two QP bands, three different files: gates [1] / [3] = (2, 0.7): everything behind y64 zeroed;
# (-1, 2): only y16 zeroed; (-1, -1): open
SERVER_THR = ["0.4 2.0 0.3 0.7 0.2 0.8", "0.1 -1 0.9 2.0 0.3 0.9", "0.4 -1 0.3 -1 0.2 0.8"]


def _workdir(path, thr):
    os.makedirs(path)
    open(os.path.join(path, "Thr_info.txt"), "w").write(thr)
    for ext in (".index", ".data-00000-of-00001"):
        shutil.copy(GOLD + ext, os.path.join(path, "model_LDP_200000_qp32.dat" + ext))  # QP 32: the real bundle; QP 22: seeded
    return path


def test_one_server_with_the_gates_of_each_directory(tmp_path):
    jobs = [(416, 240, 22, 11), (416, 240, 32, 12), (200, 136, 32, 13)]  # width, height, QP, the client's seed
    frames = 3
    env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="21")
    client = os.path.join(BIN, "ldp_client")
    solo = [_workdir(str(tmp_path / ("solo%d" % k)), SERVER_THR[k]) for k in range(3)]
    many = [_workdir(str(tmp_path / ("many%d" % k)), SERVER_THR[k]) for k in range(3)]
    daemon = lambda args, cwd, out=subprocess.DEVNULL: subprocess.Popen([sys.executable, LAUNCHER] + args + ["--idle-timeout", "120"], cwd=cwd, env=env,
                                                                        stdout=out, stderr=subprocess.PIPE, text=True)
    start = lambda dirs: [subprocess.Popen([client, d, str(w), str(h), str(qp), str(frames), "--seed", str(seed), "--digest", os.path.join(d, "digest.txt")],
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for d, (w, h, qp, seed) in zip(dirs, jobs)]
    # the references: three solo `serve` processes, each in its own directory under that directory's file; beside them ONE server
    daemons = [daemon(["--python", "--max-frames", str(frames)], d) for d in solo]
    clients = []
    try:
        clients += start(solo) + start(many)
        deadline = time.monotonic() + 60
        while not all(os.path.exists(os.path.join(d, "pred_start.sig")) for d in many):
            assert time.monotonic() < deadline and all(c.poll() is None for c in clients[3:]), "the clients did not reach their first handshake"
            time.sleep(0.001)
        server = daemon(["--sessions"] + many + ["--gates-per-dir", "--max-frames", str(3 * frames)], str(tmp_path), subprocess.PIPE)
        daemons.append(server)
        said, err = server.communicate(timeout=240)
        assert server.returncode == 0, err[-800:]
        for c in clients:
            assert c.wait(timeout=240) == 0, c.stderr.read()[-500:]
        for d in daemons[:3]:
            assert d.wait(timeout=120) == 0, d.stderr.read()[-800:]
    finally:
        for p in clients + daemons:
            if p.poll() is None:
                p.kill()
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    for k, (w, h, qp, seed) in enumerate(jobs):
        want = open(os.path.join(solo[k], "digest.txt")).read()
        assert len(want.splitlines()) == frames
        assert open(os.path.join(many[k], "digest.txt")).read() == want, "directory %d: per-frame cu_depth.dat digests differ" % k
        assert md5(os.path.join(many[k], "state.dat")) == md5(os.path.join(solo[k], "state.dat")), "directory %d: state.dat differs" % k
        assert md5(os.path.join(many[k], "cu_depth.dat")) == md5(os.path.join(solo[k], "cu_depth.dat"))
    # the zero patterns of the last frame: each directory's own gates, in one server
    last = [np.fromfile(os.path.join(many[k], "cu_depth.dat"), dtype="<f4").reshape(-1, 21) for k in range(3)]
    assert [_pattern(p) for p in last] == [[(False, False)], [(True, False)], [(True, True)]]
    assert all((p[:, 0] > 0).all() for p in last)


# -------------------------------------------------------------------------------------------------------------------- offline ---
def _write_resi(path, lum):
    nf, h, w = lum.shape
    with open(path, "wb") as f:
        for k in range(nf + 1):  # frame 0 is the intra picture
            f.write((lum[k - 1] if k else np.zeros((h, w), np.uint8)).tobytes())
            f.write(np.full(w * h // 2, 128, np.uint8).tobytes())


def test_offline_list_with_a_file_for_one_qp(tmp_path):
    files = [("a", 200, 136, 32, 3), ("b", 128, 64, 22, 2), ("c", 416, 240, 32, 2)]  # name, width, height, QP, residual frames
    for name, w, h, qp, nf in files:
        _write_resi(str(tmp_path / (name + ".yuv")), lb.frames(6400 + nf, w, h, nf))
    # the model directory's own file: only y16 zeroed; the file of QP 32: everything behind y64 zeroed.  All models are seeded
    models, other = tmp_path / "models", tmp_path / "models32"
    for d, thr in ((models, SERVER_THR[1]), (other, SERVER_THR[0])):
        d.mkdir()
        (d / "Thr_info.txt").write_text(thr)
    env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="21")
    run = lambda *args: subprocess.run([sys.executable, DRIVER] + [str(x) for x in args], capture_output=True, text=True, env=env, timeout=300)
    lst = tmp_path / "set.txt"
    lst.write_text("".join("%s %d %d %d %s\n" % (tmp_path / (name + ".yuv"), w, h, qp, tmp_path / (name + ".list.dat")) for name, w, h, qp, nf in files))
    # each line alone, with the file that holds for its QP as <model-dir>/Thr_info.txt
    runs = [run(tmp_path / (name + ".yuv"), w, h, qp, "--out", tmp_path / (name + ".solo.dat"), "--model-dir", other if qp == 32 else models)
            for name, w, h, qp, nf in files]
    runs.append(run("--list", lst, "--piece-frames", 2, "--model-dir", models, "--thr-info-qp", 32, other / "Thr_info.txt"))
    # the option with a single sequence: the pair is simply the context's
    runs.append(run(tmp_path / "a.yuv", 200, 136, 32, "--out", tmp_path / "a.single.dat", "--model-dir", models, "--thr-info-qp", 32, other / "Thr_info.txt"))
    for r in runs:
        assert r.returncode == 0, r.stderr[-800:]
    for name, w, h, qp, nf in files:
        solo = open(str(tmp_path / (name + ".solo.dat")), "rb").read()
        assert len(solo) == nf * lb.nctu(w, h) * 21 * 4
        assert open(str(tmp_path / (name + ".list.dat")), "rb").read() == solo, name
        p = np.frombuffer(solo, dtype="<f4").reshape(nf, -1, 21)
        assert all(_pattern(f) == [(False, False) if qp == 32 else (True, False)] for f in p), name
    assert open(str(tmp_path / "a.single.dat"), "rb").read() == open(str(tmp_path / "a.solo.dat"), "rb").read()
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
