"""-m gpu: several live Low-Delay-P encoders on one context (include/ethcnn.h "config #5 online, several live encoders") against the
definition: every frame of a step, and the state it leaves resident, are what ethcnn_ldp_step gives on a context of its own that holds
the same CNN, the same thresholds and the frame's bundle.  Every comparison is array_equal on the raw 32-bit words, or byte equality
of files.  The reference contexts are separate contexts, one per bundle; a session's solo loop runs there from its first frame to its
last before the next session's, so the context is that session's own for the length of the loop.

CNN, bundles, gains and thresholds are those of tests/test_gpu_ldp_batch.py (seed 21; bundle (42, 0.5) whose y64 lies around the first
threshold 0.5, bundle (41, 3.0) which saturates), so closed and open gates both occur; the tests assert that they do.

Shapes: 72x72 (4 CTUs); 200x136 (12, width no multiple of 16: the slow load form); 1040x64 (17: a full group and one CTU); 416x240
(28); 1x1; 2560x1920 (1200: a second gate mini-batch); 2112x64 (33 CTUs = 3 groups: 24 of them are 72 groups).

Pass cuts: ethcnn_create rounds max_ctus_per_pass up to a multiple of 1024, at least 1024, so the smallest pass a context can run
holds 64 groups (the cap of 32 in the CPU plan test describes the planner alone).  The context asked for with max_ctus_per_pass = 32
therefore runs the 7 groups of the five-picture table in ONE pass; a real cut needs more than 64 groups.  The tests count the
CTU-load launches of a step (one per pass) and assert the number."""
import hashlib
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import ldp_buffers as lb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
GOLD = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
ERR_ARG, ERR_NOWEIGHTS = -1, -5
BUNDLES = [(42, 0.5, 37), (41, 3.0, 22)]  # (LSTM seed, head gain, QP)
# (width, height, bundle)
TABLE = [(72, 72, 0), (200, 136, 1), (1040, 64, 0), (416, 240, 1), (1, 1, 0)]
NF = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d words differ, max |d| = %g" % (what, int((_bits(got) != _bits(want)).sum()), np.abs(got - want).max())


def _make_ctx(pkg, oracle, **kw):
    c = pkg.EthCnn(device=0, **kw)
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
    """the reference contexts: the same CNN and thresholds, one per bundle"""
    out = []
    for seed, gain, qp in BUNDLES:
        c = _make_ctx(pkg, oracle)
        c.load_lstm_synthetic(seed, gain)
        out.append(c)
    yield out
    for c in out:
        c.close()


def _sessions(pkg, c, places=None):
    s = pkg.LdpSessions(c, places or len(BUNDLES))
    for i, (seed, gain, qp) in enumerate(BUNDLES):
        s.load_lstm_synthetic(i, seed, gain)
    return s


def _solo(ref, w, h, qp, steps):
    """the reference: ethcnn_ldp_step per (luma, i_frame, state_in) on a context that is this loop's own -> ([probs], [state behind
    each step])"""
    probs, states = [], []
    for luma, i_frame, state_in in steps:
        probs.append(ref.ldp_step(luma, w, h, qp, i_frame, state_in).copy())
        states.append(ref.ldp_get_state(w, h))
    return probs, states


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
            if f.get("state_in") is not None:
                d["d_state_in"] = alloc(n * 2 * 448 * 4)
                d["d_state_in"].upload(np.ascontiguousarray(f["state_in"], dtype=np.float32))
            dev.append(d)
            ns.append(n)
        s.step_device(dev)
        c.synchronize()
        return [d["d_probs"].download(np.float32, n * 21).reshape(n, 21) for d, n in zip(dev, ns)]
    finally:
        c.synchronize()
        for b in bufs:
            b.free()


_T1 = {}  # the pictures of TABLE and their solo loops: computed once, never changed


def _table(refs):
    if not _T1:
        lums = [lb.frames(5000 + j, w, h, NF) for j, (w, h, bi) in enumerate(TABLE)]
        want = [_solo(refs[bi], w, h, BUNDLES[bi][2], [(lums[j][t], t + 1, None) for t in range(NF)]) for j, (w, h, bi) in enumerate(TABLE)]
        _T1.update(lums=lums, want=want)
    return _T1["lums"], _T1["want"]


def _run_table(pkg, c, refs, step):
    """four steps over the five sessions, the order of the frames permuted from call to call -> checked against the solo loops"""
    lums, want = _table(refs)
    with _sessions(pkg, c) as s:
        ids = [s.open(w, h) for (w, h, bi) in TABLE]
        assert ids == [0, 1, 2, 3, 4]
        for t, order in enumerate([(0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (1, 3, 4, 0, 2), (3, 0, 1, 2, 4)]):
            got = step(s, c, [{"session": ids[j], "luma": lums[j][t], "qp": BUNDLES[TABLE[j][2]][2], "i_frame": t + 1, "bundle": TABLE[j][2]} for j in order])
            for pos, j in enumerate(order):
                _same(got[pos], want[j][0][t], "session %d, frame %d: probabilities" % (j, t + 1))
            if t in (0, NF - 1):
                for j in range(5):
                    _same(s.get_state(ids[j]), want[j][1][t], "session %d: state behind frame %d" % (j, t + 1))
        assert [s.state_ctus(i) for i in ids] == [4, 12, 17, 28, 1]


def test_mixed_table_equals_the_solo_loops(pkg, ctx, refs):
    lums, want = _table(refs)
    # both gate states occur in the reference itself (every picture here is one mini-batch): a gate launch that does nothing, or
    # zeroes everything, cannot pass
    closed = [(j, t) for j in range(5) for t in range(NF) if (want[j][0][t][:, 1:] == 0).all()]
    opened = [(j, t) for j in range(5) for t in range(NF) if (want[j][0][t][:, 1:5] != 0).any()]
    assert closed and opened, (closed, opened)
    _run_table(pkg, ctx, refs, _dev_step)


def test_host_step_equals_the_solo_loops(pkg, ctx, refs):
    _run_table(pkg, ctx, refs, lambda s, c, frames: s.step(frames))


def test_subsets_resets_and_reopened_sessions(pkg, ctx, refs):
    lums, _ = _table(refs)
    extra = lb.frames(5100, 136, 72, 2)  # the picture size session 4 is reopened at: 6 CTUs
    given = lb.state(77, 12)
    qp = lambda j: BUNDLES[TABLE[j][2]][2]
    # per session: the (luma, i_frame, state_in) it sees, in order
    seen = {0: [(lums[0][0], 1, None), (lums[0][1], 2, None), (lums[0][2], 1, None), (lums[0][3], 2, None)],
            1: [(lums[1][0], 1, None), (lums[1][1], 2, None), (lums[1][2], 3, given)],
            2: [(lums[2][0], 1, None), (lums[2][1], 2, None), (lums[2][2], 3, None)],
            3: [(lums[3][0], 1, None), (lums[3][1], 2, None)],
            4: [(lums[4][0], 1, None), (lums[4][1], 2, None)]}
    want = {j: _solo(refs[TABLE[j][2]], TABLE[j][0], TABLE[j][1], qp(j), seen[j]) for j in seen}
    want_re = _solo(refs[1], 136, 72, BUNDLES[1][2], [(extra[0], 1, None), (extra[1], 2, None)])
    at = {j: 0 for j in seen}

    def frame(j):
        luma, i_frame, sin = seen[j][at[j]]
        return {"session": j, "luma": luma, "qp": qp(j), "i_frame": i_frame, "bundle": TABLE[j][2], "state_in": sin}

    with _sessions(pkg, ctx) as s:
        assert [s.open(w, h) for (w, h, bi) in TABLE] == [0, 1, 2, 3, 4]

        def step(js):
            kept = {j: s.get_state(j) for j in range(5) if j not in js and s.state_ctus(j)}
            got = s.step([frame(j) for j in js])
            for pos, j in enumerate(js):
                _same(got[pos], want[j][0][at[j]], "session %d, its step %d: probabilities" % (j, at[j]))
                _same(s.get_state(j), want[j][1][at[j]], "session %d, its step %d: state" % (j, at[j]))
                at[j] += 1
            for j, st in kept.items():
                _same(s.get_state(j), st, "session %d was not in the call: its state" % j)

        with pytest.raises(pkg.EthCnnError) as e:  # nothing resident yet
            s.step([dict(frame(3), i_frame=2)])
        assert e.value.code == ERR_ARG and "needs the previous frame's state" in str(e.value) and "28 CTUs" in str(e.value)
        step([0, 2])
        step([1])
        step([4, 3, 2, 1, 0])     # 0, 1, 2: frame 2; 3, 4: frame 1
        step([2, 0, 1, 3, 4])     # 0 restarts at frame 1; 1 gets an explicit state; 2: frame 3; 3, 4: frame 2
        before = {j: s.get_state(j) for j in range(4)}
        s.close(4)
        with pytest.raises(pkg.EthCnnError) as e:
            s.get_state(4)
        assert e.value.code == ERR_ARG
        assert s.open(136, 72) == 4 and s.state_ctus(4) == 0  # the id is reused, the state is not
        with pytest.raises(pkg.EthCnnError) as e:
            s.step([{"session": 4, "luma": extra[1], "qp": BUNDLES[1][2], "i_frame": 2, "bundle": 1}])
        assert e.value.code == ERR_ARG and "6 CTUs" in str(e.value)
        got = s.step([{"session": 4, "luma": extra[0], "qp": BUNDLES[1][2], "i_frame": 1, "bundle": 1}])
        _same(got[0], want_re[0][0], "the reopened session, frame 1")
        for j in range(4):
            _same(s.get_state(j), before[j], "session %d beside the reopened one: its state" % j)
        got = s.step([{"session": 4, "luma": extra[1], "qp": BUNDLES[1][2], "i_frame": 2, "bundle": 1}, frame(0)])
        _same(got[0], want_re[0][1], "the reopened session, frame 2")
        _same(s.get_state(4), want_re[1][1], "the reopened session: state")
        _same(got[1], want[0][0][3], "session 0 beside the reopened one")
        _same(s.get_state(0), want[0][1][3], "session 0 beside the reopened one: state")


def _passes(c, fn):
    """the CTU-load launches (one per pass) that fn() enqueues on context c"""
    c.synchronize()
    c.reset_stage_times()
    out = fn()
    c.synchronize()
    return out, int(c.stage_times()["launches"]["tile"])


def test_a_context_created_with_a_cap_of_32_equals_the_default(pkg, oracle, refs):
    """the issue's case as stated: the table of the first test on a context created with max_ctus_per_pass = 32.  The library clamps
    that cap to 1024 CTUs, so the 112 rows are one pass (asserted); cuts that do happen: the two tests below"""
    small = _make_ctx(pkg, oracle, max_ctus_per_pass=32)
    try:
        counted = []

        def step(s, c, frames):
            got, passes = _passes(c, lambda: _dev_step(s, c, frames))
            counted.append(passes)
            return got
        _run_table(pkg, small, refs, step)
        assert counted == [1, 1, 1, 1]
    finally:
        small.close()


def test_small_pictures_across_a_pass_cut(pkg, oracle, ctx, refs):
    """24 pictures of 33 CTUs (3 groups each, 72 groups) in one step, two frames.  On a context of 1024 CTUs per pass that is a pass of
    64 groups and one of 8: picture 21 (groups 63..65) lies across the cut, pictures 22 and 23 start inside the second pass."""
    w, h, n, k = 2112, 64, 33, 24
    assert pkg.ethcnn.ldp_sessions_plan([n] * k, 1024) == {"first_group": [3 * j for j in range(k)], "pass_groups": [64, 8]}
    lums = [lb.frames(5400 + j, w, h, 2) for j in range(k)]
    want = [_solo(refs[j % 2], w, h, BUNDLES[j % 2][2], [(lums[j][t], t + 1, None) for t in range(2)]) for j in range(k)]
    small = _make_ctx(pkg, oracle, max_ctus_per_pass=1024)
    try:
        for c, passes in ((small, 2), (ctx, 1)):
            with _sessions(pkg, c) as s:
                ids = [s.open(w, h) for _ in range(k)]
                for t in range(2):
                    frames = [{"session": ids[j], "luma": lums[j][t], "qp": BUNDLES[j % 2][2], "i_frame": t + 1, "bundle": j % 2} for j in range(k)]
                    got, ran = _passes(c, lambda: _dev_step(s, c, frames))
                    assert ran == passes, (ran, passes)
                    for j in range(k):
                        _same(got[j], want[j][0][t], "%d passes: picture %d, frame %d" % (passes, j, t + 1))
                for j in (0, 20, 21, 22, 23):
                    _same(s.get_state(ids[j]), want[j][1][1], "%d passes: picture %d: state" % (passes, j))
    finally:
        small.close()


def test_a_caller_state_is_used_at_any_frame_number(pkg, ctx, refs):
    """ethcnn_ldp_step uses state_in whenever it is given; i_frame then only carries the phase.  One session stepped with a state at
    i_frame = 1, 0 and 2, through the device and the host entry, beside a session that starts from zeros at the same frame number."""
    w, h, bi = 200, 136, 1
    n, qp = lb.nctu(w, h), BUNDLES[bi][2]
    lum = lb.frames(5500, w, h, 3)
    for step in (_dev_step, lambda s, c, frames: s.step(frames)):
        with _sessions(pkg, ctx) as s:
            a, b = s.open(w, h), s.open(w, h)
            for t, i_frame in enumerate((1, 0, 2)):
                given = lb.state(90 + t, n)
                want = _solo(refs[bi], w, h, qp, [(lum[t], i_frame, given)])
                zeros = _solo(refs[bi], w, h, qp, [(lum[t], 1, None)])
                assert not np.array_equal(_bits(want[0][0]), _bits(zeros[0][0])), "the state must matter for this check to mean anything"
                got = step(s, ctx, [{"session": a, "luma": lum[t], "qp": qp, "i_frame": i_frame, "bundle": bi, "state_in": given},
                                    {"session": b, "luma": lum[t], "qp": qp, "i_frame": 1, "bundle": bi}])
                _same(got[0], want[0][0], "state_in at i_frame %d: probabilities" % i_frame)
                _same(s.get_state(a), want[1][0], "state_in at i_frame %d: state" % i_frame)
                _same(got[1], zeros[0][0], "no state_in at i_frame 1: probabilities")
                _same(s.get_state(b), zeros[1][0], "no state_in at i_frame 1: state")


def test_two_gate_mini_batches_beside_a_small_picture(pkg, oracle, ctx, refs):
    """2560x1920 (1200 CTUs: mini-batches of 1024 and 176) with 72x72, two frames; thresholds between the two mini-batches' largest
    y64 of frame 1, taken from the reference's own open-gate output, close one and not the other.  Also on a context of 1024 CTUs per
    pass (created with a cap of 32, which the library rounds up to 1024), where the 76 groups of the table are two passes -- counted --
    and the cut falls inside the large picture."""
    w, h, bi = 2560, 1920, 0
    big, tiny = lb.frames(5200, w, h, 2), lb.frames(5201, 72, 72, 2)
    ref, qp = refs[bi], BUNDLES[bi][2]
    ref.set_thresholds(0.0, 0.0)
    small = None
    try:
        y64 = ref.ldp_step(big[0], w, h, qp, 1)[:, 0]
        m0, m1 = float(y64[:1024].max()), float(y64[1024:].max())
        assert m0 != m1
        thr = (m0 + m1) / 2
        ref.set_thresholds(thr, thr)
        ctx.set_thresholds(thr, thr)
        want_big = _solo(ref, w, h, qp, [(big[t], t + 1, None) for t in range(2)])
        want_tiny = _solo(ref, 72, 72, qp, [(tiny[t], t + 1, None) for t in range(2)])
        p = want_big[0][0]
        gone = [bool((p[:1024, 1:] == 0).all()), bool((p[1024:, 1:] == 0).all())]
        assert sorted(gone) == [False, True], (m0, m1, thr, gone)
        small = _make_ctx(pkg, oracle, max_ctus_per_pass=32)
        small.set_thresholds(thr, thr)
        assert pkg.ethcnn.ldp_sessions_plan([4, 1200], 1024)["pass_groups"] == [64, 12]
        for c, what, passes in ((ctx, "default cap", 1), (small, "cap clamped to 1024", 2)):
            with _sessions(pkg, c) as s:
                a, b = s.open(72, 72), s.open(w, h)
                for t in range(2):
                    frames = [{"session": a, "luma": tiny[t], "qp": qp, "i_frame": t + 1, "bundle": bi},
                              {"session": b, "luma": big[t], "qp": qp, "i_frame": t + 1, "bundle": bi}]
                    got, ran = _passes(c, lambda: _dev_step(s, c, frames))
                    assert ran == passes, (what, ran)
                    _same(got[0], want_tiny[0][t], "%s: 72x72, frame %d" % (what, t + 1))
                    _same(got[1], want_big[0][t], "%s: 2560x1920, frame %d" % (what, t + 1))
                _same(s.get_state(b), want_big[1][1], "%s: 2560x1920: state" % what)
                _same(s.get_state(a), want_tiny[1][1], "%s: 72x72: state" % what)
    finally:
        ref.set_thresholds(0.5, 0.5)
        ctx.set_thresholds(0.5, 0.5)
        if small is not None:
            small.close()


def test_caller_buffers_and_refusals(pkg, ctx, refs):
    w, h, bi = 200, 136, 1
    n, qp = lb.nctu(w, h), BUNDLES[bi][2]
    pitch, offset = w + 7, 5
    buf, lum = lb.pitched(5300, w, h, 2, pitch, pitch * h + 13, offset, lb.LUMA_FILL[0])
    want = _solo(refs[bi], w, h, qp, [(lum[0], 1, None), (lum[1], 2, None)])
    d_luma = ctx.alloc(buf.size)
    d_state = ctx.alloc(n * 2 * 448 * 4 + 16)
    probs = lb.guarded(ctx, n * 21 * 4, lead=lb.GUARD + 4)  # 4-byte, not 16-byte aligned
    other = ctx.alloc(4 * 21 * 4)
    try:
        d_luma.upload(buf)
        assert (d_luma.ptr + offset) % 16 != 0 and probs.ptr % 16 == 4
        with _sessions(pkg, ctx, places=3) as s:  # (bundle 2 stays empty)
            a, b = s.open(w, h), s.open(72, 72)
            base = {"session": a, "qp": qp, "bundle": bi, "pitch": pitch, "d_probs": probs.ptr}
            for t in range(2):
                s.step_device([dict(base, d_luma=d_luma.ptr + offset + t * (pitch * h + 13), i_frame=t + 1)])
                _same(lb.check_guards(probs, what="frame %d" % (t + 1)).reshape(n, 21), want[0][t], "pitched, offset luma: frame %d" % (t + 1))
            _same(s.get_state(a), want[1][1], "pitched, offset luma: state")
            mark = np.full(n * 21, 7.0, np.float32)
            probs.upload(mark)
            frame = dict(base, d_luma=d_luma.ptr + offset, i_frame=3)
            tiny = {"session": b, "qp": qp, "bundle": bi, "d_luma": d_luma.ptr, "i_frame": 1, "d_probs": other}
            refusals = [("a misaligned state_in", [dict(frame, d_state_in=d_state.ptr + 4)], ERR_ARG, "state_in of frame 0"),
                        ("a misaligned probs", [dict(frame, d_probs=probs.ptr + 2)], ERR_ARG, "probs of frame 0"),
                        ("a repeated session", [tiny, frame, dict(frame, d_probs=other)], ERR_ARG, "session %d is named by frames 1 and 2" % a),
                        ("an empty bundle", [dict(frame, bundle=2)], ERR_NOWEIGHTS, "bundle 2 is empty"),
                        ("a bundle out of range", [dict(frame, bundle=3)], ERR_NOWEIGHTS, "bundle 3"),
                        ("an unknown session", [dict(frame, session=7)], ERR_ARG, "session 7 is not open"),
                        ("a pitch below the width", [dict(frame, pitch=w - 1)], ERR_ARG, "pitch"),
                        ("null luma", [dict(frame, d_luma=None)], ERR_ARG, "frame 0"),
                        ("overlapping probs", [frame, dict(tiny, d_probs=probs.ptr + 84)], ERR_ARG, "overlaps"),
                        ("probs on its own state_in", [dict(frame, d_state_in=d_state.ptr, d_probs=d_state.ptr + 16)], ERR_ARG, "probs of frame 0 overlaps a buffer of frame 0"),
                        ("probs on its own picture", [dict(frame, d_probs=d_luma.ptr + 4)], ERR_ARG, "probs of frame 0 overlaps a buffer of frame 0"),
                        ("probs on another's picture", [frame, dict(tiny, d_probs=d_luma.ptr + 6400)], ERR_ARG, "probs of frame 1 overlaps a buffer of frame 0"),
                        ("no frames", [], ERR_ARG, "0 frames"),
                        ("33 frames", [frame] * 33, ERR_ARG, "33 frames")]
            for what, bad, code, text in refusals:
                with pytest.raises(pkg.EthCnnError) as e:
                    s.step_device(bad)
                assert e.value.code == code and text in str(e.value), (what, str(e.value))
                assert np.array_equal(lb.check_guards(probs, what=what), mark), what
                _same(s.get_state(a), want[1][1], "%s: the state behind the refusal" % what)
                assert s.state_ctus(b) == 0, what
    finally:
        ctx.synchronize()
        for x in (d_luma, d_state, other, probs):
            x.free()


# ---------------------------------------------------------------------------------------------------------------------- server ---
def _workdir(path):
    os.makedirs(path)
    open(os.path.join(path, "Thr_info.txt"), "w").write("0.4 0.6 0.3 0.7 0.2 0.8")
    for ext in (".index", ".data-00000-of-00001"):
        shutil.copy(GOLD + ext, os.path.join(path, "model_LDP_200000_qp32.dat" + ext))  # QP 32: the real bundle; QP 22: seeded
    return path


def test_one_server_for_three_directories(tmp_path):
    jobs = [(416, 240, 22, 11), (416, 240, 32, 12), (200, 136, 32, 13)]  # width, height, QP, the client's seed
    frames = 5
    env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="21")
    client = os.path.join(BIN, "ldp_client")
    needed = subprocess.check_output(["readelf", "-d", client]).decode()
    assert "amdhip64" not in needed and "ethcnn" not in needed, "ldp_client must be host only"
    solo = [_workdir(str(tmp_path / ("solo%d" % k))) for k in range(3)]
    many = [_workdir(str(tmp_path / ("many%d" % k))) for k in range(3)]
    daemon = lambda args, cwd, out=subprocess.DEVNULL: subprocess.Popen([sys.executable, LAUNCHER] + args + ["--idle-timeout", "120"], cwd=cwd, env=env,
                                                                        stdout=out, stderr=subprocess.PIPE, text=True)
    start = lambda dirs: [subprocess.Popen([client, d, str(w), str(h), str(qp), str(frames), "--seed", str(seed), "--digest", os.path.join(d, "digest.txt")],
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for d, (w, h, qp, seed) in zip(dirs, jobs)]
    # the references: three solo `serve` processes; beside them ONE --sessions process for its three directories.  The clients are
    # host-only programs, so that one process is the only one that opens the GPU for those directories.
    daemons = [daemon(["--python", "--max-frames", str(frames)], d) for d in solo]
    clients = []
    try:
        clients += start(solo) + start(many)
        # the server starts once all three of its encoders stand in their first handshake: its first round must take the three
        # together, whatever the timing afterwards
        deadline = time.monotonic() + 60
        while not all(os.path.exists(os.path.join(d, "pred_start.sig")) for d in many):
            assert time.monotonic() < deadline and all(c.poll() is None for c in clients[3:]), "the clients did not reach their first handshake"
            time.sleep(0.001)
        server = daemon(["--sessions"] + many + ["--max-frames", str(3 * frames)], str(tmp_path), subprocess.PIPE)
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
    # directories that wait in the same round share ONE step: the server says how many each step held
    steps = [int(ln.split("(")[1].split()[0]) for ln in said.splitlines() if "in this step" in ln]
    assert sum(steps) == 3 * frames and steps[0] == 3, steps
    for k, (w, h, qp, seed) in enumerate(jobs):
        want = open(os.path.join(solo[k], "digest.txt")).read()
        assert len(want.splitlines()) == frames
        assert open(os.path.join(many[k], "digest.txt")).read() == want, "directory %d: per-frame cu_depth.dat digests differ" % k
        md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
        assert md5(os.path.join(many[k], "state.dat")) == md5(os.path.join(solo[k], "state.dat")), "directory %d: state.dat differs" % k
        assert open(os.path.join(many[k], "state.dat.idx")).read().split() == [str(frames), str(w), str(h)]
        assert not [f for f in os.listdir(many[k]) if ".tmp." in f]
