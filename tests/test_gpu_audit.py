"""-m gpu: the comparison of two predictions and the plan audit (include/ethcnn.h "comparing two predictions") on the GPU against the
numpy restatement (tests/audit_ref.py).  The comparator is integer and bit arithmetic, so every comparison with the restatement is
EXACT equality of every field of the struct and of the flag bytes; the one tolerance in this file is the plans' own contract
(max |dp| <= 1e-4 against the exact plan, TOL of tests/test_gpu_fast_plan.py) in the audit tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import audit_caps
import audit_ref as ref
import calib_ref
import grid_caps
import sim_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "audit_plan.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
NATIVE = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "video_to_cu_depth")
TOL = 1e-4  # the plans' contract
THR = sim_ref.thr((600, 700, 800), (400, 300, 200))
ERR_ARG, ERR_PLAN_REFUSED = -1, -8

_CASES = {}


def _case(n, seed=None):
    """(a, b, reference with THR, reference without) of n random CTUs, 1 % of them moved by one ulp and 0.1 % by 1e-3; made once"""
    if n not in _CASES:
        rng = np.random.default_rng(900 + (n if seed is None else seed))
        a = calib_ref.edge_probs(rng, n)
        b = ref.perturbed(rng, a, 0.01, 0.001, 1e-3)
        want = ref.compare(a, b, TOL, THR), ref.compare(a, b, TOL)
        for x in (a, b):
            x.setflags(write=False)
        _CASES[n] = (a, b) + want
    return _CASES[n]


class Dev(object):
    """an array in HBM at `offset` bytes behind a 256-byte aligned allocation"""

    def __init__(self, ctx, arr=None, nbytes=None, offset=0):
        self.ctx = ctx
        self.nbytes = arr.nbytes if arr is not None else nbytes
        self.buf = ctx.alloc(self.nbytes + 64)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + offset
        if arr is not None and arr.nbytes:
            arr = np.ascontiguousarray(arr)
            ctx._chk(ctx.lib.ethcnn_memcpy_h2d(ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))

    def get(self, dtype, count):
        out = np.empty(count, dtype)
        if out.nbytes:
            self.ctx._chk(self.ctx.lib.ethcnn_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        self.buf.free()


def _f32(pair):
    return tuple(np.float32(x) for x in pair)


def _same(got, want, flags=None):
    assert ref.stats_equal(got, want), ref.mismatch(got, want)
    if flags is not None:
        assert np.array_equal(flags, want["flags"]), np.flatnonzero(flags != want["flags"])[:8]


def _device_compare(ctx, a, b, tol, thr, width=None, height=None, offset=0):
    """the device entry over a, b uploaded at `offset` -> (stats, flags)"""
    n = a.size // 21
    da, db, df = Dev(ctx, a, offset=offset), Dev(ctx, b, offset=offset), Dev(ctx, np.full(n, 0xEE, np.uint8))   # (every flag byte is written)
    try:
        if width is None:
            st = ctx.compare_probs_device(da.ptr, db.ptr, n, tol, thr, df.ptr)
        else:
            st = ctx.compare_frames_device(da.ptr, db.ptr, width, height, n // (((width + 63) // 64) * ((height + 63) // 64)), tol, thr, df.ptr)
        return st, df.get(np.uint8, n)
    finally:
        for d in (da, db, df):
            d.free()


@pytest.mark.parametrize("n", [1, audit_caps.TILE - 1, audit_caps.TILE, audit_caps.TILE + 1])
def test_sizes_around_the_tile(ctx, n):
    a, b, want_thr, want = _case(n)
    assert want["rejected_ctus"] == 0
    st, flags = _device_compare(ctx, a, b, TOL, THR)
    _same(st, want_thr, flags)
    st, flags = _device_compare(ctx, a, b, TOL, None)
    _same(st, want, flags)
    assert st["with_thr"] == 0 and st["class_diff"] == [0, 0, 0] and st["search_diff_ctus"] == 0 and st["checked_a"] == st["checked_b"] == [0, 0, 0, 0]


def test_past_one_trip_of_the_grid(ctx):
    """one CTU more than the largest input that fits one trip: some block runs the loop twice, with a tile of one CTU"""
    cap = audit_caps.compare(grid_caps.cus(ctx))
    n = cap + 1
    assert n > cap
    a, b, want_thr, _ = _case(n, seed=1)
    assert want_thr["rejected_ctus"] == 0 and want_thr["search_diff_ctus"] > 0 and min(want_thr["over_tol"]) > 0
    st, flags = _device_compare(ctx, a, b, TOL, THR)
    _same(st, want_thr, flags)


@pytest.mark.parametrize("flags_in", ["hbm", "page-locked"])
def test_prefetched_tiles_on_the_second_and_third_trip(pkg, ctx, flags_in):
    """16-byte aligned arrays of 2 x cap + 1 CTUs: every block stages a tile on its first trip and issues the loads of its next one
    before it compares; on the second trip every block stages THAT tile from the registers, and the first block then finds a partial
    third tile of one CTU, which it must not have prefetched.  An eighth of the values differ, so every tile has something to find.
    With and without a candidate; flags in HBM, and, through the host entry over ethcnn_host_alloc buffers (read and written in
    place, one launch), in page-locked memory."""
    cap = audit_caps.compare(grid_caps.cus(ctx))
    n = 2 * cap + 1
    assert n > cap + audit_caps.TILE and n >= cap + 2 * audit_caps.TILE + 1 and (n - 1) % audit_caps.TILE == 0
    if "dense" not in _CASES:
        rng = np.random.default_rng(77)
        a = calib_ref.edge_probs(rng, n)
        b = np.where(rng.integers(0, 8, size=a.shape) == 0, calib_ref.edge_probs(rng, n), a).astype(np.float32)
        a[-1, 0], b[-1, 0] = np.float32(0.9), np.float32(0.1)   # the CTU of the partial tile: SPLIT ONLY against CURRENT ONLY at its root
        _CASES["dense"] = (a, b, ref.compare(a, b, TOL, THR), ref.compare(a, b, TOL))
    a, b, want_thr, want = _CASES["dense"]
    assert want["rejected_ctus"] == 0 and want_thr["flags"][-1] == ref.OVER_TOL | ref.CLASS | ref.SEARCH
    tiles = want_thr["flags"][:n - 1].reshape(-1, audit_caps.TILE)
    assert (tiles & ref.SEARCH).any(axis=1).all() and (tiles & ref.OVER_TOL).any(axis=1).all()   # in every tile of both trips
    if flags_in == "hbm":
        st, flags = _device_compare(ctx, a, b, TOL, THR)
        _same(st, want_thr, flags)
        st, flags = _device_compare(ctx, a, b, TOL, None)
        _same(st, want, flags)
    else:
        c = pkg.EthCnn(device=0)
        try:
            pa, pb = c.host_buffer(a.nbytes).view(np.float32).reshape(a.shape), c.host_buffer(b.nbytes).view(np.float32).reshape(b.shape)
            pf = c.host_buffer(n)
            assert pa.ctypes.data % 16 == 0 and pb.ctypes.data % 16 == 0
            pa[:], pb[:] = a, b
            for thr, w in ((THR, want_thr), (None, want)):
                pf[:] = 0xEE
                _same(c.compare_probs(pa, pb, TOL, thr, want_flags=pf), w, pf)
        finally:
            c.close()


@pytest.mark.parametrize("offset", [4, 8])
def test_any_four_byte_aligned_base(ctx, offset):
    """the same arrays at a base 4 and 8 bytes behind a 16-byte boundary (the dword loads) equal those on it (the 16-byte loads)"""
    a, b, want_thr, _ = _case(1000)
    st, flags = _device_compare(ctx, a, b, TOL, THR, offset=offset)
    _same(st, want_thr, flags)
    st0, flags0 = _device_compare(ctx, a, b, TOL, THR, offset=0)
    _same(st0, want_thr, flags0)
    da = Dev(ctx, a, offset=2)
    try:
        with pytest.raises(Exception) as ei:
            ctx.compare_probs_device(da.ptr, da.ptr, 10, TOL)
        assert ei.value.code == ERR_ARG
    finally:
        da.free()


@pytest.mark.parametrize("case", ref.crafted_cases(), ids=lambda c: c["name"])
def test_edge_cases_of_the_definition(ctx, case):
    want = ref.compare(case["a"], case["b"], case["tol"], case["thr"], case["width"], case["height"])
    if case["name"] != "rejected on one side":
        assert want["rejected_ctus"] == 0
    for field, v in case["expect"].items():
        assert want[field] == v
    st, flags = _device_compare(ctx, case["a"], case["b"], case["tol"], case["thr"], case["width"], case["height"])
    _same(st, want, flags)
    for field, v in case["expect"].items():
        assert st[field] == v, field
    if case["width"] is None:
        host = ctx.compare_probs(case["a"], case["b"], case["tol"], case["thr"], want_flags=True)
    else:
        host = ctx.compare_frames(case["a"], case["b"], case["width"], case["height"], case["tol"], case["thr"], want_flags=True)
    _same(host, want, host["flags"])


def test_random_ctus_under_several_candidates(ctx):
    import decide_ref
    a, b, want_thr, want = _case(4000)
    assert want["rejected_ctus"] == 0
    assert sum(want["bits_diff"]) >= 40 and 1 <= sum(want["over_tol"]) <= 8   # 1 % by one ulp, 0.1 % by 1e-3
    st, flags = _device_compare(ctx, a, b, TOL, THR)
    _same(st, want_thr, flags)
    rng = np.random.default_rng(5)
    b2 = np.where(rng.integers(0, 4, size=b.shape) == 0, calib_ref.edge_probs(rng, 4000), b).astype(np.float32)   # a quarter of the values afresh
    differ = []
    for cand in decide_ref.candidates(rng, 6):   # (the second one is the full search: every node lands in BOTH on both sides)
        w = ref.compare(a, b2, TOL, cand)
        assert w["rejected_ctus"] == 0
        differ.append(w["search_diff_ctus"])
        st, flags = _device_compare(ctx, a, b2, TOL, cand)
        _same(st, w, flags)
    assert differ[1] == 0 and min(differ[:1] + differ[2:]) > 0


def test_a_set_split_over_two_calls(ctx):
    """one call over n CTUs = two calls over a split at an odd index, combined: sums add, a maximum goes by (value, lowest index)"""
    a, b, want_thr, _ = _case(1000)
    cut = 333
    whole, _ = _device_compare(ctx, a, b, TOL, THR)
    da, db = Dev(ctx, a), Dev(ctx, b)   # the second part starts 333 * 84 bytes in: 4 bytes behind a 16-byte boundary
    try:
        parts = [ctx.compare_probs_device(da.ptr + lo * 84, db.ptr + lo * 84, hi - lo, TOL, THR) for lo, hi in ((0, cut), (cut, 1000))]
    finally:
        da.free()
        db.free()
    assert parts[0]["ctus"] == cut and parts[1]["ctus"] == 1000 - cut
    both = ref.combine(*parts)
    _same(whole, want_thr)
    assert ref.stats_equal(both, whole), ref.mismatch(both, whole)


@pytest.mark.parametrize("thr", [None, THR], ids=["no thr", "thr"])
@pytest.mark.parametrize("w,h,frames", [(200, 136, 3), (64, 64, 1)])
def test_frame_layout(ctx, w, h, frames, thr):
    per = ((w + 63) // 64) * ((h + 63) // 64)
    rng = np.random.default_rng(w + frames)
    a = calib_ref.edge_probs(rng, frames * per)
    b = np.where(rng.integers(0, 3, size=a.shape) == 0, calib_ref.edge_probs(rng, frames * per), a).astype(np.float32)
    a[0, 0], b[0, 0] = np.float32(0.9), np.float32(0.1)   # SPLIT ONLY against CURRENT ONLY at the root of the first CTU under THR
    want = ref.compare(a, b, TOL, thr, w, h)
    assert want["rejected_ctus"] == 0 and sum(want["over_tol"]) > 0
    if thr is not None:
        assert want["search_diff_ctus"] > 0
        if per > 1:  # partial CTUs: the per-CTU layout counts other checks
            assert want["checked_a"] != ref.compare(a, b, TOL, thr)["checked_a"]
    st, flags = _device_compare(ctx, a, b, TOL, thr, w, h)
    _same(st, want, flags)
    host = ctx.compare_frames(a, b, w, h, TOL, thr, want_flags=True)
    _same(host, want, host["flags"])


def test_refusals_and_the_empty_call(ctx):
    a, b, _, _ = _case(255)
    da, db = Dev(ctx, a), Dev(ctx, b)
    try:
        def refused(fn):
            with pytest.raises(Exception) as ei:
                fn()
            assert ei.value.code == ERR_ARG, ei.value

        refused(lambda: ctx.compare_frames_device(da.ptr, db.ptr, 100, 64, 1, TOL))            # a width that is no multiple of 8
        refused(lambda: ctx.compare_frames_device(da.ptr, db.ptr, 64, 100, 1, TOL))
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, 2 ** 31, TOL))                 # 2^31 CTUs
        refused(lambda: ctx.compare_frames_device(da.ptr, db.ptr, 4096, 4096, 2 ** 19, TOL))    # 4096 CTUs a frame x 2^19 frames
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, -1, TOL))
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, 255, -1.0))
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, 255, float("nan")))
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, 255, TOL, ((1025, 0, 0), (0, 0, 0))))
        refused(lambda: ctx.compare_probs_device(da.ptr, db.ptr, 255, TOL, ((5, 5, 5), (-2, 0, 0))))
        refused(lambda: ctx.compare_probs_device(None, db.ptr, 255, TOL))
        for st in (ctx.compare_probs_device(da.ptr, db.ptr, 0, TOL, THR), ctx.compare_frames_device(None, None, 200, 136, 0, TOL),
                   ctx.compare_probs(a[:0], b[:0], TOL, THR, want_flags=True)):
            assert st["worst_ctu"] == [-1, -1, -1] and st["ctus"] == 0 and st["max_abs"] == [0.0, 0.0, 0.0] and sum(st["over_tol"] + st["bits_diff"]) == 0
    finally:
        da.free()
        db.free()


def test_host_entries_from_pageable_and_page_locked_memory(pkg):
    """the host entries equal the device entries, from pageable memory (staged) and from ethcnn_host_alloc memory (read and written in
    place), and with one side of each"""
    c = pkg.EthCnn(device=0)
    try:
        a, b, want_thr, want = _case(1000)
        dev, dflags = _device_compare(c, a, b, TOL, THR)
        _same(dev, want_thr, dflags)
        host = c.compare_probs(a, b, TOL, THR, want_flags=True)
        _same(host, want_thr, host["flags"])
        pa, pb = c.host_buffer(a.nbytes).view(np.float32).reshape(a.shape), c.host_buffer(b.nbytes).view(np.float32).reshape(b.shape)
        pf = c.host_buffer(1000)
        pa[:], pb[:], pf[:] = a, b, 0xEE
        pinned = c.compare_probs(pa, pb, TOL, THR, want_flags=pf)
        _same(pinned, want_thr, pf)
        mixed = c.compare_probs(pa, b, TOL, None, want_flags=True)
        _same(mixed, want, mixed["flags"])
        pf[:] = 0xEE
        mixed = c.compare_probs(a, pb, TOL, THR, want_flags=pf)
        _same(mixed, want_thr, pf)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------- the audit ---
@pytest.fixture(scope="module")
def audit_case(oracle):
    import bench
    w, h, frames = 1920, 1088, 5   # 510 CTUs a frame: 2,550 CTUs in one pass, above the 2,304 of the single-launch path
    return {"w": w, "h": h, "frames": frames, "qp": 27, "luma": bench.synth_luma(w, h, frames, seed=4027), "blob": oracle.synth_blob(11, 8.0)}


@pytest.mark.parametrize("plan", [2, 3])
def test_audit_of_a_plan(pkg, audit_case, plan):
    k = audit_case
    w, h, frames, qp = k["w"], k["h"], k["frames"], k["qp"]
    n = frames * 510
    c = pkg.EthCnn(device=0)
    try:
        c.load_blob(k["blob"])
        c.set_thresholds(0.45, 0.6)
        before = c.predict_luma(k["luma"], w, h, frames, qp)
        d_luma, d_a, d_b = c.alloc(k["luma"].nbytes), c.alloc(n * 84), c.alloc(n * 84)
        d_luma.upload(k["luma"])
        # two predictions of the test's own, open gates
        c.set_thresholds(-1.0, -1.0)
        c.predict_luma_device(d_luma, w, h, frames, qp, d_a)
        c.set_fc1_plan(plan)
        c.predict_luma_device(d_luma, w, h, frames, qp, d_b)
        c.synchronize()
        own = c.compare_frames_device(d_a, d_b, w, h, frames, TOL, THR)
        host = ref.compare(d_a.download(np.float32, n * 21), d_b.download(np.float32, n * 21), TOL, THR, w, h)
        _same(own, host)
        c.set_fc1_plan(0)
        c.set_thresholds(0.45, 0.6)
        times = c.stage_times()
        assert c.audit_plan_bytes(w, h, frames) == (n * 84 + 15) // 16 * 16 + n * 84 and (n * 84) % 16 == 8   # side b is moved up to 16 bytes
        c.set_debug_capture(False)
        assert c.debug_fetch(pkg.ethcnn.DBG_FC1, 4).shape == (4, 448)
        r = c.audit_plan(d_luma, w, h, frames, qp, plan, TOL, THR)
        assert r["plan"] == plan and r["passes"] >= 1 and r["fast_passes"] >= 1
        assert ref.stats_equal(r, own), ref.mismatch(r, own)
        assert r["rejected_ctus"] == 0 and sum(r["bits_diff"]) > 0           # the plans are not bit-identical: the audit saw the fast run
        for level in range(3):
            assert r["max_abs"][level] <= TOL, (level, r["max_abs"])         # the project's contract
        assert sum(r["over_tol"]) == 0
        # the context is what it was
        assert c.fc1_plan() == 0 and _f32(c.get_thresholds()) == _f32((0.45, 0.6)) and c.stage_times() == times
        # ... but for the workspace, which holds the audit's last pass: its intermediates are refused until the caller's next pass
        with pytest.raises(pkg.EthCnnError) as ei:
            c.debug_fetch(pkg.ethcnn.DBG_FC1, 4)
        assert ei.value.code == ERR_ARG and "audit" in str(ei.value)
        after = c.predict_luma(k["luma"], w, h, frames, qp)
        assert c.debug_fetch(pkg.ethcnn.DBG_FC1, 4).shape == (4, 448)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        # the host form uploads the planes itself
        r2 = c.audit_plan(k["luma"], w, h, frames, qp, plan, TOL, THR)
        assert ref.stats_equal(r2, own) and r2["fast_passes"] == r["fast_passes"]
        with pytest.raises(pkg.EthCnnError) as ei:
            c.audit_plan(d_luma, w, h, frames, qp, 1)
        assert ei.value.code == ERR_ARG
        for d in (d_luma, d_a, d_b):
            d.free()
    finally:
        c.close()


def test_audit_of_a_small_geometry_says_so(pkg, audit_case):
    """one 768 x 512 frame runs as a single-launch pass, which computes exactly under every plan: fast_passes == 0, and the zeros are
    not passed off as agreement"""
    c = pkg.EthCnn(device=0)
    try:
        c.load_blob(audit_case["blob"])
        luma = np.ascontiguousarray(audit_case["luma"].reshape(-1)[:768 * 512])
        r = c.audit_plan(luma, 768, 512, 1, 32, 3, TOL, THR)
        assert r["fast_passes"] == 0 and r["passes"] >= 1 and r["ctus"] == 96 and r["rejected_ctus"] == 0
        assert r["max_abs"] == [0.0, 0.0, 0.0] and r["bits_diff"] == [0, 0, 0] and r["over_tol"] == [0, 0, 0] and r["search_diff_ctus"] == 0
        assert r["checked_a"] == r["checked_b"] and sum(r["checked_a"]) > 0
    finally:
        c.close()


def test_audit_of_a_refused_plan_changes_nothing(pkg, oracle, audit_case):
    import adversarial_blobs as ab
    c = pkg.EthCnn(device=0)
    try:
        c.load_blob(ab.cancelling_pairs(oracle, 21, 8.0, 1e6))
        c.set_thresholds(0.3, 0.7)
        c.set_fc1_plan(2)
        luma = np.ascontiguousarray(audit_case["luma"].reshape(-1)[:832 * 480 * 8])
        times = c.stage_times()
        with pytest.raises(pkg.EthCnnError, match="refused") as ei:
            c.audit_plan(luma, 832, 480, 8, 32, 3, TOL, THR)
        assert ei.value.code == ERR_PLAN_REFUSED
        assert not c.check_fc1_plan(3)["accepted"]
        assert c.fc1_plan() == 2 and _f32(c.get_thresholds()) == _f32((0.3, 0.7)) and c.stage_times() == times
    finally:
        c.close()


def test_audit_file_entry(pkg, audit_case, tmp_path):
    """frames 1, 3 and 5 of a 7-frame 768 x 512 file = the device entry on those planes; with the single-launch pass off the plans do run"""
    w, h = 768, 512
    rng = np.random.default_rng(17)
    fsz = w * h * 3 // 2
    yuv = rng.integers(0, 256, size=7 * fsz, dtype=np.uint8)
    planes = audit_case["luma"].reshape(-1)[:7 * w * h].reshape(7, w * h)
    for f in range(7):
        yuv[f * fsz:f * fsz + w * h] = planes[f]
    path = str(tmp_path / "seq.yuv")
    yuv.tofile(path)
    c = pkg.EthCnn(device=0)
    try:
        c.load_blob(audit_case["blob"])
        c.set_small_pass_launch(False)
        want = c.audit_plan(np.ascontiguousarray(planes[[1, 3, 5]]), w, h, 3, 27, 3, TOL, THR)
        got = c.audit_plan_yuv_file(path, w, h, 27, 3, first=1, step=2, count=3, tol=TOL, thr=THR)
        assert got["fast_passes"] >= 1 and sum(got["bits_diff"]) > 0 and got["ctus"] == 3 * 96
        assert ref.stats_equal(got, want) and got["passes"] == want["passes"] and got["fast_passes"] == want["fast_passes"]
        other = c.audit_plan_yuv_file(path, w, h, 27, 3, first=0, step=2, count=3, tol=TOL, thr=THR)
        assert other["max_abs"] != got["max_abs"] or other["bits_diff"] != got["bits_diff"]   # other frames, other numbers
        for kw in (dict(first=1, step=2, count=4), dict(first=7, step=1, count=1), dict(first=-1, step=1, count=1), dict(first=0, step=0, count=2)):
            with pytest.raises(pkg.EthCnnError) as ei:
                c.audit_plan_yuv_file(path, w, h, 27, 3, tol=TOL, **kw)
            assert ei.value.code == ERR_ARG, kw
        c.set_source_format(10, 420)
        with pytest.raises(pkg.EthCnnError) as ei:
            c.audit_plan_yuv_file(path, w, h, 27, 3, first=1, step=2, count=3)
        assert ei.value.code == ERR_ARG
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- tool and launchers ---
def _tool(*argv):
    return subprocess.run([sys.executable, TOOL] + [str(a) for a in argv], capture_output=True, text=True)


def test_tool_compares_two_files(tmp_path):
    rng = np.random.default_rng(23)
    a = calib_ref.edge_probs(rng, 24)           # 200 x 136 x 2 frames
    b = a.copy()
    b[17, 0] = a[17, 0] + np.float32(1e-3) if a[17, 0] < 0.5 else a[17, 0] - np.float32(1e-3)   # frame 1, CTU (1, 1)
    pa, pb = tmp_path / "a.dat", tmp_path / "b.dat"
    a.tofile(str(pa))
    b.tofile(str(pb))
    (tmp_path / "Thr_info.txt").write_text("0.6 0.4 0.7 0.3 0.8 0.2\n")
    r = _tool("--case", pa, pa, 200, 136)
    assert r.returncode == 0 and "max |dp|" in r.stdout, r.stderr
    r = _tool("--case", pa, pb, 200, 136, "--thr-info", tmp_path / "Thr_info.txt", "--order", "ai", "--flags-out", tmp_path / "flags.bin")
    assert r.returncode == 2, r.stderr
    row = [ln for ln in r.stdout.splitlines() if ln.startswith("64x64")][0]
    assert "(1, 1, 1)" in row and row.split()[-2] == "1", r.stdout
    assert "checks per CU size" in r.stdout
    flags = np.fromfile(str(tmp_path / "flags.bin"), np.uint8)
    assert flags.size == 24 and flags[17] & ref.OVER_TOL and not flags[np.arange(24) != 17].any()
    assert _tool("--case", pa, pb, 200, 136, "--tol", 0.01).returncode == 0
    assert _tool("--case", pa, pb, 100, 136).returncode == 1 and _tool("--bogus").returncode == 1


def test_tool_audits_a_file(tmp_path):
    """--yuv on a geometry that runs exactly says so with exit status 3; a bigger one audits the plan"""
    rng = np.random.default_rng(29)
    env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="11", ETHCNN_HEAD_GAIN="8")
    small = tmp_path / "small.yuv"
    rng.integers(0, 256, size=2 * 768 * 512 * 3 // 2, dtype=np.uint8).tofile(str(small))
    r = subprocess.run([sys.executable, TOOL, "--yuv", str(small), "768", "512", "32", "--plan", "3", "--model-dir", str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 3 and "fast passes / passes: 0 / 1" in r.stdout and "say nothing" in r.stdout, r.stdout + r.stderr
    big = tmp_path / "big.yuv"
    rng.integers(0, 256, size=3 * 2560 * 1600 * 3 // 2, dtype=np.uint8).tofile(str(big))   # 1,000 CTUs a frame: 3 frames are above the 2,304
    r = subprocess.run([sys.executable, TOOL, "--yuv", str(big), "2560", "1600", "32", "--plan", "3", "--model-dir", str(tmp_path), "--count", "3"],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "(plan 3)" in r.stdout and "fast passes / passes: 0" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("form", ["python", "native"])
def test_launchers_audit_before_they_trust_a_plan(tmp_path, form):
    w, h, frames, qp = 832, 480, 4, 37
    rng = np.random.default_rng(31)
    rng.integers(0, 256, size=frames * w * h * 3 // 2, dtype=np.uint8).tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text("0.6 0.4 0.7 0.3 0.8 0.2\n")
    cmd = [sys.executable, LAUNCHER] if form == "python" else [NATIVE]

    def run(**env):
        e = dict(os.environ, ETHCNN_SYNTHETIC_SEED="9", ETHCNN_HEAD_GAIN="8")
        e.pop("ETHCNN_FC1_PLAN_AUDIT", None)
        e.pop("ETHCNN_DEVICES", None)
        e.update(env)
        return subprocess.run(cmd + ["seq.yuv", str(w), str(h), str(qp)], cwd=str(tmp_path), capture_output=True, text=True, env=e)

    r = run(ETHCNN_FC1_PLAN="3")
    assert r.returncode == 0 and "audit" not in r.stderr, r.stderr
    plain = (tmp_path / "cu_depth.dat").read_bytes()
    os.remove(str(tmp_path / "cu_depth.dat"))
    r = run(ETHCNN_FC1_PLAN="3", ETHCNN_FC1_PLAN_AUDIT="2")
    assert r.returncode == 0 and "plan 3 audit over 2 frames (step 2)" in r.stderr and "fast passes" in r.stderr, r.stderr
    assert (tmp_path / "cu_depth.dat").read_bytes() == plain
    os.remove(str(tmp_path / "cu_depth.dat"))
    r = run(ETHCNN_FC1_PLAN="3", ETHCNN_FC1_PLAN_AUDIT="x")
    assert r.returncode == 1 and "ETHCNN_FC1_PLAN_AUDIT" in r.stderr and not (tmp_path / "cu_depth.dat").exists()
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    r = run(ETHCNN_FC1_PLAN_AUDIT="x")            # no plan: the variable is not read
    assert r.returncode == 0 and (tmp_path / "cu_depth.dat").exists(), r.stderr
