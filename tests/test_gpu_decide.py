"""-m gpu: the partition decisions (include/ethcnn.h "partition decisions") on the GPU.  Every test compares the library's bytes with
the numpy restatement (tests/decide_ref.py) byte for byte, and ethcnn_decide_counts_from_codes of the library's codes with
ethcnn_sim_eval of the same candidate: two independent kernels and one restatement in agreement.  Probabilities are synthetic
(calib_ref.edge_probs: a seeded spread over the k / 1024 grid with exact grid values and their neighbours); no predictor runs.
Integers only: every comparison is equality.

On "the planes fed back as labels give bad_ctus == 0": that holds when the preferred partition is the deepest one the search can reach
(mid_k = 0 with down_k >= 0), and it is asserted there.  For mid_k = 512 it does not hold and cannot: the simulator judges every decided
node by its own flag whatever happened above it, so a SPLIT ONLY node below a BOTH node at which the preferred partition stops is a
wrong_split (tests/test_decide_cpu.py holds the smallest such CTU).  What does hold for every mid_k, and is asserted: no wrong_stop
anywhere, every block's reach holds its label's bit, and the bad CTUs are exactly those with a SPLIT ONLY node below the label's leaf."""
import os
import subprocess
import sys

import numpy as np
import pytest

import calib_ref
import decide_ref as dref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "decide_partition.py")
GATES = {"none": ref.GATES_NONE, "ai": ref.GATES_AI, "ldp": ref.GATES_LDP}
MID = ref.thr((600, 700, 800), (400, 300, 200))
KEYS = ("codes", "reach", "depth")
_CASES = {}


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


def _cands():
    return dref.candidates(np.random.default_rng(77), 6)


def _per_ctu_case(n):
    """(probs, depth) of n CTUs; with n > 1 the last carries a NaN, a -0.5 and a 1.5 and is rejected"""
    if n not in _CASES:
        rng = np.random.default_rng(200 + n)
        probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
        if n > 1:
            probs[-1, 0], probs[-1, 3], probs[-1, 20] = np.nan, -0.5, 1.5
        probs.setflags(write=False)
        depth.setflags(write=False)
        _CASES[n] = (probs, depth)
    return _CASES[n]


def _same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == np.uint8 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _agree(pkg, sim, s, cand, gates="none", mid=512):
    """host form over the whole set == restatement; its codes' counters == ethcnn_sim_eval == the simulator's restatement"""
    want = dref.decide(s, cand, GATES[gates], mid)
    got = sim.decide(cand, gates, mid)
    _same(got, want)
    counts = pkg.ethcnn.sim_counts_from_codes(got["codes"])
    assert ref.equal(counts, sim.eval(cand, gates)[0]) and ref.equal(counts, s.evaluate(cand, GATES[gates])[0])
    return got


@pytest.mark.parametrize("labelled", [True, False])
@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_per_ctu_layout(pkg, sim, n, labelled):
    probs, depth = _per_ctu_case(n)
    s = ref.Set()
    s.add(probs, depth if labelled else None)
    sim.add(probs, depth if labelled else None)
    filled = np.zeros(6, ref.COUNTS)
    for i, c in enumerate(_cands()):
        got = _agree(pkg, sim, s, c, "ldp" if i == 0 else "none", (512, 0, 1024)[i % 3])  # (the per-CTU layout is never gated)
        filled[i] = pkg.ethcnn.sim_counts_from_codes(got["codes"])
        assert ((got["codes"][:, 21] & 2) != 0).sum() == s.info()["labelled_ctus"]
    if n >= 63:
        assert ref.fills_every_field(filled, edges=0, labels=labelled)
    else:
        assert all(filled[f].any() for f in ("checked", "split_only", "current_only", "both"))


def test_rejected_rows(pkg, sim):
    probs, depth = (a.copy() for a in _per_ctu_case(65))
    probs[-1] = probs[0]
    probs[3, 5], probs[40, 0], probs[64, 20], probs[17, 2] = np.nan, np.float32(1.0000001), -0.25, np.inf
    rows = [3, 17, 40, 64]
    s = ref.Set()
    s.add(probs, depth)
    sim.add(probs, depth)
    assert sim.info()["rejected_ctus"] == 4 == s.info()["rejected_ctus"]
    got = _agree(pkg, sim, s, MID)
    assert not got["codes"][rows, :21].any() and (got["codes"][rows, 21] == 4).all() and not got["codes"][rows, 22:].any()
    assert not got["reach"][rows].any() and (got["depth"][rows] == 255).all() and (np.delete(got["depth"], rows, 0) <= 3).all()


def test_windows_null_outputs_host_device_and_pieces(pkg, ctx, sim):
    probs, depth = _per_ctu_case(1025)
    s = ref.Set()
    s.add(probs, depth)
    sim.add(probs, depth)
    whole = _agree(pkg, sim, s, MID)
    for first, n in ((3, 700), (256, 513), (1024, 1), (1025, 0), (0, 0)):
        _same(sim.decide(MID, "none", 512, first, n), dref.decide(s, MID, first=first, n=n))
        _same(sim.decide(MID, "none", 512, first, n), {k: whole[k][first:first + n] for k in KEYS})
    # the device form, NULL output pointers in every combination; buffers that are not given stay as they were
    first, n = 130, 777
    size = {"codes": 24, "reach": 16, "depth": 16}
    bufs = {k: ctx.alloc(n * size[k]) for k in KEYS}
    try:
        for mask in range(8):
            given = [k for i, k in enumerate(KEYS) if mask >> i & 1]
            for k in KEYS:
                bufs[k].upload(np.full(n * size[k], 0xAB, np.uint8))
            sim.decide_device(MID, "none", 512, first, n, *[bufs[k] if k in given else None for k in KEYS])
            for k in KEYS:
                got = bufs[k].download(np.uint8, n * size[k]).reshape(n, size[k])
                assert np.array_equal(got, whole[k][first:first + n]) if k in given else (got == 0xAB).all(), (mask, k)
            host = sim.decide(MID, "none", 512, first, n, want=given)
            assert sorted(host) == sorted(given)
            _same(host, {k: whole[k][first:first + n] for k in KEYS}, given)
    finally:
        for b in bufs.values():
            b.free()
    # pieces of 300 CTUs: four of them, the same bytes
    sim.set_decide_piece(300)
    _same(sim.decide(MID), whole)
    _same(sim.decide(MID, first=1, n=1000), {k: whole[k][1:1001] for k in KEYS})
    sim.set_decide_piece(0)
    _same(sim.decide(MID), whole)


def _frame_set(w, h, frames, skip, labelled, seed):
    rng = np.random.default_rng(seed)
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    probs = calib_ref.edge_probs(rng, frames * nctu).reshape(frames, nctu, 21)
    labels = None
    if labelled:
        labels = rng.integers(0, 4, size=(frames + skip, h // 16, w // 16)).astype(np.uint8)
        labels[skip:, :4, :4] = np.array([3, 0, 2], np.uint8)[:frames, None, None]
    return probs, labels


def test_frame_layout_ragged_without_planes(pkg, sim):
    w, h, frames = 200, 136, 2
    probs, _ = _frame_set(w, h, frames, 0, False, 200)
    s = ref.Set()
    s.add_frames(probs, None, w, h)
    sim.add_frames(probs, None, w, h)
    full = dref.decide(s, ref.thr(*ref.FULL))
    # all three levels cross the edge, and the bottom right CTU holds one 8 x 8 CU: the corner case
    assert (full["codes"][:, 0] == 4).any() and (full["codes"][:, 1:5] == 4).any() and (full["codes"][:, 5:21] == 4).any()
    assert full["codes"][11, 22] == 1 and full["codes"][23, 22] == 1
    for cand, gates in ((ref.thr(*ref.FULL), "none"), (MID, "ai"), (MID, "ldp"), (_cands()[3], "none")):
        want = _agree(pkg, sim, s, cand, gates)
        got = sim.decide_frames(cand, gates, w, h, planes=False)
        assert sorted(got) == ["codes", "reach"]
        _same(got, want, ("codes", "reach"))
        _same(sim.decide_frames(cand, gates, w, h, first_frame=1, nframes=1, planes=False), {k: want[k][12:] for k in KEYS}, ("codes", "reach"))
    with pytest.raises(pkg.EthCnnError) as e:  # no label planes for a size that is no multiple of 16
        sim.decide_frames(MID, "none", w, h)
    assert e.value.code == pkg.ethcnn.ERR_ARG


def test_frame_layout_with_labels_and_guarded_planes(pkg, ctx, sim):
    w, h, frames, skip = 208, 144, 3, 1
    probs, labels = _frame_set(w, h, frames, skip, True, 208)
    s = ref.Set()
    s.add(*_per_ctu_case(63))  # the frames do not start the set
    s.add_frames(probs, labels, w, h, skip)
    sim.add(*_per_ctu_case(63))
    sim.add_frames(probs, labels, w, h, skip_label_frames=skip)
    counts = np.zeros(3, ref.COUNTS)
    for i, (cand, gates) in enumerate(((MID, "none"), (_cands()[3], "ai"), (_cands()[4], "ldp"))):
        want = _agree(pkg, sim, s, cand, gates)
        counts[i] = dref.counts_from_codes(want["codes"])
        planes = dref.planes_of(want["depth"][63:], w, h)
        assert planes.shape == (3, 9, 13) and planes.max() <= 3
        got = sim.decide_frames(cand, gates, w, h, first=63)
        _same(got, {k: want[k][63:] for k in KEYS}, ("codes", "reach"))
        assert np.array_equal(got["planes"], planes)
        # frames 1..2 into the middle of a guarded buffer, at an odd address
        size = 2 * 9 * 13
        buf = ctx.alloc(size + 64)
        try:
            buf.upload(np.full(size + 64, 0xCD, np.uint8))
            sim.decide_frames_device(cand, gates, 512, 63 + 12, w, h, 2, None, None, buf.ptr + 31)
            raw = buf.download(np.uint8, size + 64)
        finally:
            buf.free()
        assert (raw[:31] == 0xCD).all() and (raw[31 + size:] == 0xCD).all() and np.array_equal(raw[31:31 + size].reshape(2, 9, 13), planes[1:])
    assert ref.fills_every_field(counts, edges=2)


def test_gates_over_two_sub_batches_a_frame(pkg, sim):
    w, h = 2112, 2048
    probs, labels = dref.gate_case(np.random.default_rng(2112))
    s = ref.Set()
    s.add_frames(probs, labels, w, h)
    sim.add_frames(probs, labels, w, h)
    assert sim.info() == s.info() and s.info()["sub_batches"] == 4
    cand = ref.thr(*dref.GATE_CAND)
    for gates in ("ai", "ldp"):
        want = _agree(pkg, sim, s, cand, gates)
        flags = want["codes"][:, 21]
        gate1, gate2 = (flags & dref.GATE1_CLOSED) != 0, (flags & dref.GATE2_CLOSED) != 0
        assert gate1[1024:1056].all() and gate1.sum() == 32 and (gate2 & ~gate1)[2080:].all() and (gate2 & ~gate1).sum() == 32
        got = sim.decide_frames(cand, gates, w, h)
        _same(got, want, ("codes", "reach"))
        assert np.array_equal(got["planes"], dref.planes_of(want["depth"], w, h))
    none = _agree(pkg, sim, s, cand, "none")
    assert not (none["codes"][:, 21] & 24).any() and not np.array_equal(none["codes"], want["codes"])


def test_mid_k_moves_the_preferred_partition_inside_reach(pkg, sim):
    probs, depth = _per_ctu_case(1025)
    s = ref.Set()
    s.add(probs, depth)
    sim.add(probs, depth)
    got = {mid: _agree(pkg, sim, s, MID, "none", mid) for mid in (0, 512, 1024)}
    assert ((got[512]["codes"][:, :21] & 7) == 3).any()
    assert not np.array_equal(got[0]["depth"], got[512]["depth"]) and not np.array_equal(got[512]["depth"], got[1024]["depth"])
    for g in got.values():
        has = g["depth"] != 255
        assert np.array_equal(g["codes"], got[0]["codes"]) and np.array_equal(g["reach"], got[0]["reach"])
        assert ((g["reach"][has].astype(np.int64) >> g["depth"][has]) & 1).all() and not g["reach"][~has].any()


def test_bad_arguments_leave_the_outputs_untouched(pkg, ctx, sim):
    e = pkg.ethcnn
    w, h, frames = 208, 144, 3
    probs, labels = _frame_set(w, h, frames, 0, True, 9)
    sim.add(*_per_ctu_case(65))
    sim.add_frames(probs, labels, w, h)
    lib, thr = sim.lib, np.asarray(MID).reshape(1).copy()
    n = 65 + 36
    host = {k: np.full((n, 24 if k == "codes" else 16), 0xEE, np.uint8) for k in KEYS}
    dev = ctx.alloc(n * 24 + 64)
    dev.upload(np.full(n * 24 + 64, 0xEE, np.uint8))
    bad_thr = [e.sim_thr((0, 0, 1025), (0, 0, 0)), e.sim_thr((0, 0, 0), (-2, 0, 0)), e.sim_thr((-1, 0, 0), (0, 0, 0))]
    p = lambda a: a.ctypes.data
    try:
        calls = [(t.reshape(1), 0, 512, 0, n) for t in bad_thr] + [(thr, 3, 512, 0, n), (thr, -1, 512, 0, n), (thr, 0, 1025, 0, n), (thr, 0, -1, 0, n),
                                                                   (thr, 0, 512, 0, n + 1), (thr, 0, 512, -1, 5), (thr, 0, 512, 5, -1), (thr, 0, 512, n + 1, 0)]
        for t, gates, mid, first, count in calls:
            assert lib.ethcnn_decide(sim.h, p(t), gates, mid, first, count, p(host["codes"]), p(host["reach"]), p(host["depth"])) == e.ERR_ARG
            assert lib.ethcnn_decide_device(sim.h, p(t), gates, mid, first, count, dev.ptr, dev.ptr, dev.ptr) == e.ERR_ARG
        assert lib.ethcnn_decide(sim.h, None, 0, 512, 0, n, p(host["codes"]), None, None) == e.ERR_ARG
        assert lib.ethcnn_decide_device(sim.h, p(thr), 0, 512, 0, n, dev.ptr + 2, None, None) == e.ERR_ARG  # not 4-byte aligned
        # the frame form: off a frame boundary, beyond the add, another geometry, frames that were added per CTU, planes for 200 x 136
        for first, ww, hh, nf, planes in ((66, w, h, 1, 0), (65, w, h, 4, 0), (65 + 24, w, h, 2, 0), (65, 144, 208, 1, 0), (0, w, h, 1, 0),
                                          (65, 200, 136, 1, dev.ptr), (65, w, 0, 1, 0), (65, w, h, -1, 0)):
            assert lib.ethcnn_decide_frames_device(sim.h, p(thr), 0, 512, first, ww, hh, nf, dev.ptr, None, planes or None) == e.ERR_ARG, (first, ww, hh, nf)
        assert lib.ethcnn_decide_frames_device(sim.h, p(thr), 0, 512, 65 + 36, w, h, 0, dev.ptr, None, None) == 0  # no frames: a no-op
        assert all((a == 0xEE).all() for a in host.values()) and (dev.download(np.uint8, n * 24 + 64) == 0xEE).all()
        with pytest.raises(pkg.EthCnnError) as err:
            sim.decide(MID, "none", 2000)
        assert err.value.code == e.ERR_ARG and "mid_k" in str(err.value)
    finally:
        dev.free()
    # after a reset the frames are gone
    sim.reset()
    with pytest.raises(pkg.EthCnnError):
        sim.decide_frames(MID, "none", w, h, nframes=1)


def test_the_planes_fed_back_as_labels(pkg, sim):
    w, h, frames = 256, 192, 4  # whole CTUs, so that every CTU is labelled
    probs, _ = _frame_set(w, h, frames, 0, False, 31)
    sim.add_frames(probs, None, w, h)
    cand = MID  # down_k >= 0
    seen_bad = 0
    for mid in (0, 512):
        planes = sim.decide_frames(cand, "ai", w, h, mid_k=mid)["planes"]
        assert planes.max() <= 3
        with pkg.PartitionSim(sim.ctx) as fresh:
            fresh.add_frames(probs, planes, w, h)
            assert fresh.info()["labelled_ctus"] == frames * 12
            counts = fresh.eval(cand, "ai")[0]
            out = fresh.decide(cand, "ai", mid)
        s = ref.Set()
        s.add_frames(probs, planes, w, h)
        _same(out, dref.decide(s, cand, ref.GATES_AI, mid))
        depth16 = out["depth"]
        assert np.array_equal(dref.planes_of(depth16, w, h), planes)       # the preferred partition of its own labels is itself
        assert not counts["wrong_stop"].any()                                # it never wants to go below a CURRENT ONLY node
        assert not dref.label_leaf_lacks(out["reach"], depth16).any()        # and is always reachable
        bad = (out["codes"][:, 21] & 1) != 0
        assert np.array_equal(bad, dref.split_only_below_label(out["codes"], depth16)) and int(counts["bad_ctus"]) == int(bad.sum())
        if mid == 0:
            assert int(counts["bad_ctus"]) == 0                              # the deepest reachable partition: nothing is visited below it
        seen_bad += int(counts["bad_ctus"])
    assert seen_bad  # (the mid_k = 512 case is not vacuous: see the module's docstring)


def test_tool_writes_a_label_file_that_the_restatement_reproduces(pkg, tmp_path):
    cases = ((208, 144, 3, 1, True, 41), (128, 64, 2, 0, False, 42))
    s, args, per_case = ref.Set(), [], []
    for i, (w, h, frames, skip, labelled, seed) in enumerate(cases):
        probs, labels = _frame_set(w, h, frames, skip, labelled, seed)
        pp, lp = str(tmp_path / ("cu_depth_%d.dat" % i)), str(tmp_path / ("Info_%d_CUDepth.dat" % i))
        probs.tofile(pp)
        if labelled:
            labels.tofile(lp)
        args += ["--case", lp if labelled else "-", pp, str(w), str(h)] + (["--skip-label-frames", str(skip)] if skip else [])
        s.add_frames(probs, labels, w, h, skip)
        per_case.append((w, h, frames, probs))
    thr_file = str(tmp_path / "Thr_info.txt")
    pkg.ethcnn.sim_write_thr_info(thr_file, MID, "ldp")
    outs = {k: str(tmp_path / (k + ".bin")) for k in ("depth", "codes", "reach")}
    r = subprocess.run([sys.executable, TOOL, "--thr-info", thr_file, "--order", "ldp", "--mid", "0.25", "--depth-out", outs["depth"], "--codes-out",
                        outs["codes"], "--reach-out", outs["reach"], "--per-frame"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = dref.decide(s, MID, ref.GATES_LDP, 256)
    planes = [dref.planes_of(want["depth"][:36], 208, 144), dref.planes_of(want["depth"][36:], 128, 64)]
    assert open(outs["depth"], "rb").read() == planes[0].tobytes() + planes[1].tobytes()
    assert open(outs["codes"], "rb").read() == want["codes"].tobytes() and open(outs["reach"], "rb").read() == want["reach"].tobytes()
    rows = [line.split(",") for line in r.stdout.strip().splitlines()]
    assert rows[0][:4] == ["case", "frame", "ctus", "checked64"] and len(rows) == 1 + 3 + 2
    full = dref.decide(s, ref.thr(*ref.FULL))
    spans = [(0, 0, 0, 12), (0, 1, 12, 24), (0, 2, 24, 36), (1, 0, 36, 38), (1, 1, 38, 40)]
    for row, (case, frame, a, b) in zip(rows[1:], spans):
        c, f = dref.counts_from_codes(want["codes"][a:b]), dref.counts_from_codes(full["codes"][a:b])
        cost, full_cost = (sum(wt * int(x) for wt, x in zip((64, 16, 4, 1), v["checked"])) for v in (c, f))
        assert [int(x) for x in row[:8]] == [case, frame, b - a] + c["checked"].tolist() + [cost] and row[8] == "%.6f" % (cost / full_cost)
        assert [int(x) for x in row[9:]] == [int(c["bad_ctus"])] + [int(((want["codes"][a:b, 21] & bit) != 0).sum()) for bit in (2, 8, 16)]
    # the second case's planes are a label file for the scorer
    lab = str(tmp_path / "Info_pred_128x64_CUDepth.dat")
    planes[1].tofile(lab)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "score_cu_depth.py"), lab, str(tmp_path / "cu_depth_1.dat"), "128", "64"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # refusals: a size that is no multiple of 16, a rejected CTU
    probs = _frame_set(200, 136, 1, 0, False, 43)[0]
    probs.tofile(str(tmp_path / "ragged.dat"))
    bad = per_case[1][3].copy()
    bad[0, 0, 0] = np.nan
    bad.tofile(str(tmp_path / "nan.dat"))
    for case, word in ((["--case", "-", str(tmp_path / "ragged.dat"), "200", "136"], "200x136"), (["--case", "-", str(tmp_path / "nan.dat"), "128", "64"], "rejected")):
        r = subprocess.run([sys.executable, TOOL, "--thr-info", thr_file, "--order", "ldp", "--depth-out", str(tmp_path / "no.dat")] + case,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(str(tmp_path / "no.dat")), r.stderr
