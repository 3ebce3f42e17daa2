"""-m gpu: every capped-grid kernel of the tool chain past its cap, and the narrowing kernel past 1024 columns.  The kernels around
the predictor launch min(work, k * CUs) blocks and walk the rest in a grid-stride loop; what the loop carries from one trip to the next
runs only when the input is larger than one trip of the device in hand.  Every case here computes its size from tests/grid_caps.py,
asserts that it exceeds the cap, and compares with the numpy restatement of the operation.  The kernels move bytes or count integers:
every comparison is equality, there is no tolerance anywhere."""
import os

import numpy as np
import pytest

import calib_ref
import extract_cases
import grid_caps
import replay_ref
import replay_world
import sim_ref
from sim_checks import SIM_CANDS, sim_checks as _sim_checks
from test_gpu_narrow import FILL, GUARD, rule, samples

pytestmark = pytest.mark.gpu
REC_AI, REC_INTER, REC_LSTM = 4992, 16516, 37264
SLOT_BASE, SLOT_BYTES = 64, 4113  # an inter record: 64 info bytes, then four slots of [QP | 16 labels | 4096 residual bytes]
IO_PIECE = 64 << 20               # the read-back piece of a sample set: one gather launch covers a read below it


@pytest.fixture(scope="module")
def cus(ctx):
    return grid_caps.cus(ctx)


# --------------------------------------------------------------------------------------------------------------------- narrowing ---
def _narrow_against_numpy(c, w, h, frames, bd, seed):
    """the layout of test_narrow_luma_device_against_numpy: a source pitch of 2 w + 6 bytes (no multiple of 16: the rows of a frame start
    at different offsets from a 16-byte boundary), a frame stride, junk between the rows, the base 2 / 6 / 14 / 0 bytes off a boundary;
    the guard bytes around every destination frame stay, the pad columns [w, roundup16(w)) are zero"""
    rng = np.random.default_rng(seed)
    rw = (w + 15) // 16 * 16
    pitch = 2 * w + 6            # bytes
    fstride = pitch * h + 10     # bytes
    words = (frames * fstride + 32) // 2
    planes = samples(rng, (frames, h, w), bd)
    junk = samples(rng, (words,), 16)  # what lies between the rows must not matter
    want = np.zeros((frames, h, rw), dtype=np.uint8)
    want[:, :, :w] = rule(planes, bd)
    host = junk.copy()
    at = (np.arange(frames)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch) // 2 + np.arange(w)[None, None, :]
    host[at] = planes
    plane = rw * h
    dfs = plane + GUARD
    d_src = c.alloc(2 * words + 16)
    d_dst = c.alloc(GUARD + frames * dfs)
    try:
        for off in (2, 6, 14, 0):
            shifted = np.zeros(2 * words + 16, dtype=np.uint8)
            shifted[off:off + host.nbytes] = host.view(np.uint8)
            d_src.upload(shifted)
            d_dst.upload(np.full(GUARD + frames * dfs, FILL, dtype=np.uint8))
            c.narrow_luma_device(d_src.ptr + off, w, h, frames, bd, d_dst.ptr + GUARD, pitch_bytes=pitch, frame_stride_bytes=fstride,
                                 dst_pitch=rw, dst_frame_stride=dfs)
            c.synchronize()
            got = d_dst.download(np.uint8, GUARD + frames * dfs)
            assert np.all(got[:GUARD] == FILL), off
            body = got[GUARD:].reshape(frames, dfs)
            assert np.all(body[:, plane:] == FILL), off                                          # the guards are intact
            assert not body[:, :plane].reshape(frames, h, rw)[:, :, w:].any(), off               # the pad columns are zero
            assert np.array_equal(body[:, :plane].reshape(frames, h, rw), want), off
    finally:
        d_src.free()
        d_dst.free()


# 1025: chunk 1 holds one segment with one valid sample; 1040: that segment is whole; 2047: chunk 1 is full but for one sample; 3840:
# four chunks, the last one of 48 segments
@pytest.mark.parametrize("bd", [10, 16])
@pytest.mark.parametrize("w", [1025, 1040, 2047, 3840])
def test_narrow_rows_wider_than_one_chunk(ctx, w, bd):
    assert w > grid_caps.NARROW_CHUNK_SAMPLES
    _narrow_against_numpy(ctx, w, 3, 2, bd, 1000 * bd + w)


def test_narrow_second_trip_with_the_last_slot_empty(ctx, cus):
    """rows of one chunk; the second trip holds 37 to 39 units: ten blocks, the last of them partly filled, and the second in-flight slot
    of every wave is off the end"""
    cap, frames = grid_caps.narrow_units(cus), 3
    h = -(-(cap + 37) // frames)
    units = frames * h
    assert units > cap and 0 < units % cap <= cap // 2  # (a whole grid takes `cap` units a trip)
    _narrow_against_numpy(ctx, 17, h, frames, 10, 17)


def test_narrow_second_trip_of_two_chunk_rows(ctx, cus):
    """the trip loop and the chunk index together: a unit of the second trip is chunk 0 or 1 of its row"""
    cap, frames, w = grid_caps.narrow_units(cus), 3, 1041
    chunks = ((w + 15) // 16 + 63) // 64
    h = -(-(cap + 75) // (frames * chunks))
    assert chunks == 2 and frames * h * chunks > cap
    _narrow_against_numpy(ctx, w, h, frames, 10, 1041)


# ------------------------------------------------------------------------------------------------------------- permuted gather ---
W_G, H_G = 1984, 1088  # 31 x 17 = 527 CTUs a frame
PER_G = (W_G // 64) * (H_G // 64)


def _seeded_files(rng, directory, tag, nfiles, frames):
    yuvs, labs = [], []
    for i in range(nfiles):
        yuvs.append(str(directory / ("%s_%d.yuv" % (tag, i))))
        labs.append(str(directory / ("%s_%d_CUDepth.dat" % (tag, i))))
        with open(yuvs[-1], "wb") as f:
            f.write(extract_cases.synth_yuv(rng, W_G, H_G, frames))
        with open(labs[-1], "wb") as f:
            f.write(rng.integers(0, 4, int(np.prod(extract_cases.label_shape(W_G, H_G, frames))), dtype=np.uint8).tobytes())
    return yuvs, labs


@pytest.mark.parametrize("kind", ["ai", "inter"])
def test_permuted_read_past_the_gather_cap(pkg, ctx, cus, kind, tmp_path):
    """k_gather<uint4> (All-Intra records) and k_gather<uint32_t> (inter records): a set of just above 8 * cus records read in the order
    of a seed, whole and as a range that starts inside the first trip and ends inside the second"""
    cap = grid_caps.gather(cus)
    frames = cap // PER_G + 1  # cut frames (MI355X: 4 frames, 2108 records > 2048)
    rng = np.random.default_rng(41 + (kind == "ai"))
    if kind == "ai":
        yuvs, labs = _seeded_files(rng, tmp_path, "ai", 1, frames)
        s = pkg.SampleSet(ctx, "ai", [32])
        s.add_sequence(W_G, H_G, yuvs[0], labs)
    else:
        yuvs, labs = _seeded_files(rng, tmp_path, "resi", 4, frames + 1)  # (frame 0 is the intra picture: not cut)
        s = pkg.SampleSet(ctx, "inter", [22, 27, 32, 37])
        s.add_sequence(W_G, H_G, yuvs, labs)
    with s:
        count, rb = s.count, s.record_bytes
        assert count == frames * PER_G > cap and rb == (REC_AI if kind == "ai" else REC_INTER)
        assert count * rb <= IO_PIECE  # one launch covers the whole read
        s.build()
        nat = s.read()
        if kind == "ai":
            lab = np.fromfile(labs[0], dtype=np.uint8).reshape(extract_cases.label_shape(W_G, H_G, frames))
            assert np.array_equal(nat, extract_cases.np_cut_ai(extract_cases.read_luma(yuvs[0], W_G, H_G), [lab], [32]))
        perm = pkg.ethcnn.sample_permutation(3, count)
        assert sorted(perm.tolist()) == list(range(count)) and not np.array_equal(perm, np.arange(count))
        assert np.array_equal(s.read(seed=3), nat[perm])
        first, n = 5, count - 7
        assert n > cap  # output records [0, cap) are the first trip of this launch, [cap, n) its second
        assert np.array_equal(s.read(first, n, seed=3), nat[perm[first:first + n]])
    for p in yuvs + labs:  # (up to 65 MB: not kept with the test's directory)
        os.remove(p)


# ---------------------------------------------------------------------------------------------------------------- replay un-cut ---
@pytest.fixture(scope="module")
def world(pkg, tmp_path_factory):
    w = replay_world.build(pkg, tmp_path_factory.mktemp("second_trip_replay"))
    yield w
    w.close()


def test_uncut_past_its_cap_from_a_callers_table(pkg, world, cus):
    """3 x 5 CTUs a frame and an odd number of CTU-frames above 2 * 8 * cus: the last trip's last block has its second slot off the end.
    The table draws from the 30 records, with entries of -1 and of nrecords (zeros come back) in both trips and at the very last CTU"""
    rows, cols, nrec = 3, 5, len(world.records)
    cap = grid_caps.uncut(cus)
    frames = (cap + 60) // (rows * cols) + 1
    frames += 1 - frames % 2
    total = rows * cols * frames
    assert total % 2 == 1 and total > cap + 60 and nrec == 30
    rng = np.random.default_rng(9)
    table = rng.integers(0, nrec, total).astype(np.int64)
    table[cap:cap + nrec] = rng.permutation(nrec)
    outside = np.concatenate([rng.choice(cap, 6, replace=False), cap + nrec + rng.choice(total - 1 - cap - nrec, 6, replace=False), [total - 1]])
    table[outside] = np.where(np.arange(outside.size) % 2 == 0, -1, nrec)
    assert (table[cap:] == -1).any() and (table[cap:] == nrec).any() and (table[:cap] < 0).any() and (table[:cap] == nrec).any()
    assert table[total - 1] == -1
    valid = (table >= 0) & (table < nrec)
    assert set(table[cap:][valid[cap:]].tolist()) == set(range(nrec))  # every record is read by the second trip
    run = dict(frames=frames, rows=rows, cols=cols, src=np.where(valid, table, 0))
    ctx = world.ctx
    exact, shifted = ctx.alloc(nrec * REC_INTER), ctx.alloc(nrec * REC_INTER + 16)
    d_src, d_resi, d_lab = ctx.alloc(total * 8), ctx.alloc(total * 4096), ctx.alloc(total * 16)
    try:
        exact.upload(world.records)  # (the last record ends with its allocation)
        shifted.upload(np.concatenate([np.zeros(4, np.uint8), world.records.reshape(-1)]))  # the inter records' own alignment: 4 bytes
        assert exact.ptr % 16 == 0 and shifted.ptr % 16 == 0
        d_src.upload(table)
        for slot in range(4):
            want_resi, want_lab = replay_ref.planes(world.records, run, slot)
            keep = valid.reshape(frames, rows, 1, cols, 1)
            want_resi = (want_resi.reshape(frames, rows, 64, cols, 64) * keep).reshape(frames, 64 * rows, 64 * cols)
            want_lab = (want_lab.reshape(frames, rows, 4, cols, 4) * keep).reshape(frames, 4 * rows, 4 * cols)
            for base in (exact.ptr, shifted.ptr + 4):
                d_resi.upload(np.full(total * 4096, 0x5A, np.uint8))
                d_lab.upload(np.full(total * 16, 0x5A, np.uint8))
                pkg.ethcnn.replay_uncut_device(ctx, base, nrec, d_src, frames, rows, cols, slot, d_resi, d_lab)
                ctx.synchronize()
                got_resi = d_resi.download(np.uint8, total * 4096).reshape(frames, 64 * rows, 64 * cols)
                got_lab = d_lab.download(np.uint8, total * 16).reshape(frames, 4 * rows, 4 * cols)
                assert np.array_equal(got_resi, want_resi), (slot, base % 16)
                assert np.array_equal(got_lab, want_lab), (slot, base % 16)
    finally:
        for b in (exact, shifted, d_src, d_resi, d_lab):
            b.free()


# ------------------------------------------------------------------------------------------------------------ calibration count ---
@pytest.fixture
def cal(pkg, ctx):
    k = pkg.Calibrator(ctx)
    yield k
    k.close()


def _calib_per_ctu_case(cus):
    """n CTUs, n above the cap and no multiple of the tile; two fully split CTUs inside the second trip carry NaN, -0.0, 1.0 and 1.5"""
    cap = grid_caps.calib_count(cus)
    n = cap + 3 * 64 + 37
    assert n > cap and n % 64 != 0
    rng = np.random.default_rng(cus)
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    depth[cap + 5], depth[cap + 70] = 3, 3
    probs[cap + 5, 0], probs[cap + 5, 2], probs[cap + 5, 9] = np.nan, -0.0, 1.0
    probs[cap + 70, 1] = 1.5
    return cap, n, probs, depth


def test_calib_per_ctu_layout_past_the_cap(ctx, cal, cus):
    cap, n, probs, depth = _calib_per_ctu_case(cus)
    want_hist, want_rej = calib_ref.histogram(probs, depth)
    assert want_rej.tolist() == [1, 1, 0]  # the NaN and the 1.5; -0.0 lands in bin 0 and 1.0 in bin 1024
    dp, dd = ctx.alloc(probs.nbytes), ctx.alloc(depth.nbytes)
    try:
        dp.upload(probs)
        dd.upload(depth)
        cal.add_device(dp, dd, n)  # one launch
        hist, rej, skipped = cal.get()
    finally:
        dp.free()
        dd.free()
    assert int(hist[0].sum()) + int(rej[0]) == n  # every CTU is a level-0 sample
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej) and skipped == 0
    cal.reset()
    cal.add(probs, depth)
    hist, rej, skipped = cal.get()
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej) and skipped == 0


@pytest.mark.parametrize("w,h", [(4928, 3264), (4944, 3264)])
def test_calib_frame_layout_past_the_cap(ctx, cal, cus, w, h):
    """label rows of 308 bytes (a CTU's four rows are aligned dwords) and of 309 bytes (byte loads); 4944 also has a partial CTU column"""
    cap = grid_caps.calib_count(cus)
    per = ((w + 63) // 64) * ((h + 63) // 64)
    frames = (cap + (w + 63) // 64) // per + 1  # MI355X: 17 frames; the last CTU row of the last frame lies in the second trip
    assert frames * per - (w + 63) // 64 >= cap and (w // 16) % 4 == (0 if w == 4928 else 1)
    rng = np.random.default_rng(w)
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16)).astype(np.uint8)
    probs = calib_ref.edge_probs(rng, frames * per).reshape(frames, per, 21)
    labels[-1, -4:, :4] = 3  # the first CTU of the last CTU row of the last frame (second trip) is fully split and rejected at level 1
    probs[-1, per - (w + 63) // 64, 3] = np.nan
    want_hist, want_rej, want_skipped = calib_ref.histogram_frames(probs, labels, w, h)
    assert want_rej.tolist() == [0, 1, 0] and want_skipped == (0 if w == 4928 else frames * (h // 64))
    dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes)
    try:
        dp.upload(probs)
        dl.upload(labels)
        assert dl.ptr % 4 == 0
        cal.add_frames_device(dp, dl, w, h, frames)  # one launch
        hist, rej, skipped = cal.get()
    finally:
        dp.free()
        dl.free()
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej) and skipped == want_skipped


def test_calib_bad_depth_that_only_the_second_trip_reads(pkg, ctx, cal, cus):
    """k_calib_commit's contract: a call with a depth byte above 3 adds nothing, wherever the byte lies"""
    cap, n, probs, depth = _calib_per_ctu_case(cus)
    cal.add(probs[:300], depth[:300])
    before = cal.get()
    assert int(before[0].sum()) > 300
    bad = depth.copy()
    bad[cap + 10, 7] = 4
    dp, dd = ctx.alloc(probs.nbytes), ctx.alloc(depth.nbytes)
    try:
        dp.upload(probs)
        dd.upload(bad)
        with pytest.raises(pkg.EthCnnError) as e:
            cal.add_device(dp, dd, n)
        assert e.value.code == pkg.ethcnn.ERR_FORMAT and "1 CTU(s)" in str(e.value) and "above 3" in str(e.value)
        after = cal.get()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and after[2] == before[2]
        dd.upload(depth)  # the next valid call works, and counts what the restatement counts
        cal.reset()
        cal.add_device(dp, dd, n)
    finally:
        dp.free()
        dd.free()
    want_hist, want_rej = calib_ref.histogram(probs, depth)
    hist, rej, _ = cal.get()
    assert np.array_equal(hist, want_hist) and np.array_equal(rej, want_rej)


# --------------------------------------------------------------------------------------------------------------- simulator pack ---
@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


# SIM_CANDS and what is checked around the cap: tests/sim_checks.py (shared with tests/test_gpu_host_pieces.py)


def test_sim_pack_per_ctu_layout_past_the_cap(ctx, sim, cus):
    cap = grid_caps.sim_pack(cus)
    n = cap + 2 * 256 + 77
    assert n > cap and n % 256 != 0
    rng = np.random.default_rng(cus + 1)
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    probs[cap + 300, 0], probs[cap + 300, 3], probs[cap + 300, 20] = np.nan, -0.5, 1.5
    s = sim_ref.Set()
    s.add(probs, depth)
    dp, dd = ctx.alloc(probs.nbytes), ctx.alloc(depth.nbytes)
    try:
        dp.upload(probs)
        dd.upload(depth)
        sim.add_device(dp, dd, n)  # one launch
    finally:
        dp.free()
        dd.free()
    _sim_checks(sim, s, cap, cap + 300, cap + 301)


def test_sim_pack_frame_layout_past_the_cap(ctx, sim, cus):
    """4928x3264: 3927 CTUs = four sub-batches a frame; a frame starts on no wave boundary, so waves straddle sub-batches.  The last
    sub-batch of every frame has its p64 capped at 500 / 1024 and the second its p32 at 600 / 1024: the gates of the second candidate
    depend on the M1 / M2 that the pack kernel reduced, in both trips"""
    w, h, per = 4928, 3264, 77 * 51
    cap = grid_caps.sim_pack(cus)
    frames = cap // per + 1  # MI355X: 134 frames
    assert frames * per > cap and per % 64 != 0 and (per + 1023) // 1024 == 4
    rng = np.random.default_rng(cus + 2)
    probs = calib_ref.edge_probs(rng, frames * per).reshape(frames, per, 21)
    probs[:, 3072:, 0] = np.minimum(probs[:, 3072:, 0], np.float32(500 / 1024.0))
    probs[:, 1024:2048, 1:5] = np.minimum(probs[:, 1024:2048, 1:5], np.float32(600 / 1024.0))
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16)).astype(np.uint8)
    reject_at = cap + 300
    probs.reshape(-1, 21)[reject_at, 7] = np.nan
    s = sim_ref.Set()
    s.add_frames(probs, labels, w, h)
    assert s.info()["sub_batches"] == 4 * frames
    assert not sim_ref.equal(s.evaluate(SIM_CANDS[1:], sim_ref.GATES_AI), s.evaluate(SIM_CANDS[1:], sim_ref.GATES_NONE))  # gates do close
    dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes)
    try:
        dp.upload(probs)
        dl.upload(labels)
        sim.add_frames_device(dp, dl, w, h, frames)  # one launch
    finally:
        dp.free()
        dl.free()
    _sim_checks(sim, s, cap, reject_at, reject_at + 1)


# ---------------------------------------------------------------------------------------------------------- ETH-LSTM sample path ---
def _lstm_samples_np(rec, vec, heads, strides, slot):
    """include/ethcnn.h "ETH-LSTM sample sets": the head's 64 info bytes with byte 0 set to 19, then for k = 0..19 the 465 float32
    [QP byte | 16 label bytes | 448-vector] of record head - k * stride at the slot, the bytes converted to float"""
    m = len(heads)
    out = np.zeros((m, REC_LSTM), np.uint8)
    out[:, :64] = rec[heads, :64]
    out[:, 0] = 19
    body = np.zeros((m, 20, 465), np.float32)
    at = SLOT_BASE + SLOT_BYTES * slot
    for k in range(20):
        ref = heads - k * strides
        body[:, k, :17] = rec[ref, at:at + 17].astype(np.float32)
        body[:, k, 17:] = vec[ref]
    out[:, 64:] = body.reshape(m, -1).view(np.uint8)
    return out


def test_lstm_sample_gather_past_its_cap(ctx, cus):
    nrec, m = 64, grid_caps.lstm_gather(cus) + 3
    assert m > grid_caps.lstm_gather(cus)
    rng = np.random.default_rng(12)
    rec = rng.integers(0, 256, (nrec, REC_INTER), dtype=np.uint8)
    vec = rng.random((nrec, 448), dtype=np.float32)
    strides = rng.integers(1, 4, m).astype(np.int64)
    heads = (19 * strides + rng.integers(0, nrec - 19 * strides)).astype(np.int64)  # the kernel trusts the table
    assert (heads - 19 * strides).min() == 0 and heads.max() == nrec - 1 and set(strides.tolist()) == {1, 2, 3}
    d_rec, d_vec, d_h, d_s, d_out = ctx.alloc(rec.nbytes), ctx.alloc(vec.nbytes), ctx.alloc(m * 8), ctx.alloc(m * 8), ctx.alloc(m * REC_LSTM)
    try:
        d_rec.upload(rec)
        d_vec.upload(vec)
        d_h.upload(heads)
        d_s.upload(strides)
        for slot in (0, 3):
            d_out.upload(np.full(m * REC_LSTM, 0x5A, np.uint8))
            ctx._chk(ctx.lib.ethcnn_bench_lstm_gather(ctx.h, d_rec.ptr, nrec, d_vec.ptr, d_h.ptr, d_s.ptr, m, slot, d_out.ptr))
            ctx.synchronize()
            got = d_out.download(np.uint8, m * REC_LSTM).reshape(m, REC_LSTM)
            assert np.array_equal(got, _lstm_samples_np(rec, vec, heads, strides, slot)), slot
    finally:
        for b in (d_rec, d_vec, d_h, d_s, d_out):
            b.free()


def test_lstm_repack_past_its_cap(ctx, cus):
    """records first .. first + n of a buffer at a slot -> the picture of 32 CTUs a row; the tiles behind the last record are zero"""
    cap = grid_caps.lstm_repack(cus)
    first, n, slot = 3, cap + 45, 1
    total = (n + 31) // 32 * 32
    assert n > cap and n % 32 != 0 and total - n >= 2
    rng = np.random.default_rng(13)
    rec = rng.integers(0, 256, (first + n + 2, REC_INTER), dtype=np.uint8)
    at = SLOT_BASE + SLOT_BYTES * slot + 17
    tiles = np.zeros((total, 64, 64), np.uint8)
    tiles[:n] = rec[first:first + n, at:at + 4096].reshape(n, 64, 64)
    want = tiles.reshape(total // 32, 32, 64, 64).transpose(0, 2, 1, 3).reshape(total // 32 * 64, 2048)
    d_rec, d_pic = ctx.alloc(rec.nbytes), ctx.alloc(total * 4096 + 64)
    try:
        d_rec.upload(rec)
        d_pic.upload(np.full(total * 4096 + 64, 0x5A, np.uint8))
        ctx._chk(ctx.lib.ethcnn_bench_lstm_repack(ctx.h, d_rec.ptr, len(rec), first, n, slot, d_pic.ptr))
        ctx.synchronize()
        got = d_pic.download(np.uint8, total * 4096 + 64)
    finally:
        d_rec.free()
        d_pic.free()
    assert np.all(got[total * 4096:] == 0x5A)
    got = got[:total * 4096].reshape(-1, 2048)
    assert not got[-64:, (n % 32) * 64:].any()  # the tail tiles
    assert np.array_equal(got, want)


def test_copy_past_its_cap(ctx, cus):
    cap = grid_caps.copy16(cus)
    nbytes = cap + 16 * 777
    assert nbytes > cap and nbytes % 16 == 0
    src = np.random.default_rng(14).integers(0, 256, nbytes, dtype=np.uint8)
    d_a, d_b = ctx.alloc(nbytes), ctx.alloc(nbytes + 64)
    try:
        d_a.upload(src)
        d_b.upload(np.full(nbytes + 64, 0x5A, np.uint8))
        ctx._chk(ctx.lib.ethcnn_bench_copy(ctx.h, d_a.ptr, d_b.ptr, nbytes))
        ctx.synchronize()
        got = d_b.download(np.uint8, nbytes + 64)
    finally:
        d_a.free()
        d_b.free()
    assert np.all(got[nbytes:] == 0x5A) and np.array_equal(got[:nbytes], src)
