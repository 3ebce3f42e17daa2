"""-m gpu: every host loop over staged pieces past its first piece.  The host entries of the calibrator, the simulator and the
comparison walk their input in pieces of 2^20 CTUs, the permuted read-back of a sample set and the sample-file writers in pieces of
64 MB; what the loops carry from one piece to the next (the source offsets, the set position of the records and of the sub-batch
maxima, the global CTU index of the comparison, the output offsets) is multiplied by zero in every smaller input.  Every case here
takes its size from tests/host_pieces.py, asserts that it exceeds the piece, and compares with the numpy restatement of the operation
and with the device entry over the same bytes.  Everything is integers or bytes: every comparison is equality."""
import os

import numpy as np
import pytest

import audit_ref as ref
import calib_ref
import decide_ref
import extract_cases
import host_pieces as hp
import sim_ref
from sim_checks import SIM_CANDS, sim_checks
from test_gpu_second_trip import _seeded_files

pytestmark = pytest.mark.gpu
TOL, THR = hp.TOL, sim_ref.thr(*hp.COMPARE_THR)


@pytest.fixture
def cal(pkg, ctx):
    k = pkg.Calibrator(ctx)
    yield k
    k.close()


@pytest.fixture
def sim(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


@pytest.fixture
def sim2(pkg, ctx):
    s = pkg.PartitionSim(ctx)
    yield s
    s.close()


@pytest.fixture(scope="module")
def pc():
    return hp.per_ctu_case()


@pytest.fixture(scope="module")
def pc_set(pc):
    s = sim_ref.Set()
    s.add(pc["probs"], pc["depth"])
    return s


@pytest.fixture(scope="module")
def fc():
    return hp.frame_case()


@pytest.fixture(scope="module")
def fc_set(fc):
    s = sim_ref.Set()
    s.add_frames(fc["probs"], fc["labels"], fc["width"], fc["height"], skip_label_frames=1)
    return s


class Dev(object):
    """host arrays in HBM for the length of a `with`"""

    def __init__(self, ctx, *arrays):
        self.ctx, self.arrays, self.bufs = ctx, arrays, []

    def __enter__(self):
        for a in self.arrays:
            self.bufs.append(self.ctx.alloc(a.nbytes))
            self.bufs[-1].upload(a)
        return self.bufs

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _same_calib(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _same_codes(sim, other, gates="ai"):
    """the decisions of the whole set, candidate by candidate: GPU against GPU"""
    for cand in (SIM_CANDS[:1], SIM_CANDS[1:]):
        assert np.array_equal(sim.decide(cand, gates, 512, want=("codes",))["codes"], other.decide(cand, gates, 512, want=("codes",))["codes"])


# ------------------------------------------------------------------------------------------------------------- per-CTU layout ---
def test_calib_add_across_pieces(ctx, cal, pc):
    n, probs, depth = pc["n"], pc["probs"], pc["depth"]
    assert n > hp.stage_ctus()
    hist, rej = calib_ref.histogram(probs, depth)
    assert int(rej[0]) == 1 and int(hist[0].sum()) + int(rej[0]) == n  # every CTU is a level-0 sample
    cal.add(probs, depth)
    got = cal.get()
    _same_calib(got, (hist, rej, 0))
    cal.reset()
    with Dev(ctx, probs, depth) as (dp, dd):
        cal.add_device(dp, dd, n)  # one call over the same bytes
        _same_calib(cal.get(), got)


def test_sim_add_across_pieces(ctx, sim, sim2, pc, pc_set):
    n, piece = pc["n"], hp.stage_ctus()
    assert n > piece
    sim.add(pc["probs"], pc["depth"])
    sim_checks(sim, pc_set, piece, pc["reject_at"], pc["labelled_at"], rejected=2)
    with Dev(ctx, pc["probs"], pc["depth"]) as (dp, dd):
        sim2.add_device(dp, dd, n)
    assert sim2.info() == sim.info()
    _same_codes(sim, sim2)


@pytest.fixture(scope="module")
def pc_compare():
    a, b, planted = hp.per_ctu_compare()
    return a, b, planted, ref.compare(a, b, TOL, THR), ref.compare(a, b, TOL)


def _same_stats(got, want, flags):
    assert ref.stats_equal(got, want), ref.mismatch(got, want)
    assert np.array_equal(flags, want["flags"])


def test_compare_probs_from_pageable_memory(ctx, pc_compare):
    a, b, planted, want_thr, want = pc_compare
    n, piece = a.shape[0], hp.compare_ctus()
    assert n > piece
    assert want["worst_ctu"] == planted and min(planted) >= piece  # each level's largest difference lies in the second piece
    with Dev(ctx, a, b) as (da, db):
        d_flags = ctx.alloc(n)
        try:
            for thr, w in ((THR, want_thr), (None, want)):
                flags = np.full(n, 0xEE, np.uint8)
                got = ctx.compare_probs(a, b, TOL, thr, want_flags=flags)
                _same_stats(got, w, flags)
                d_flags.upload(np.full(n, 0xEE, np.uint8))
                dev = ctx.compare_probs_device(da, db, n, TOL, thr, d_flags)  # one launch over the same bytes
                _same_stats(dev, w, d_flags.download(np.uint8, n))
                assert ref.stats_equal(got, dev)
        finally:
            d_flags.free()


def test_compare_probs_one_side_and_the_flags_in_place(pkg, pc_compare):
    """a and the flags in ethcnn_host_alloc buffers, b pageable: the pieces read a in place at a + at * 21 and write the flags in place
    at flags + at, while b is staged"""
    a, b, planted, want_thr, _ = pc_compare
    n = a.shape[0]
    assert n > hp.compare_ctus()
    c = pkg.EthCnn(device=0)
    try:
        pa, pf = c.host_buffer(a.nbytes).view(np.float32).reshape(a.shape), c.host_buffer(n)
        pa[:] = a
        pf[:] = 0xEE
        got = c.compare_probs(pa, b, TOL, THR, want_flags=pf)
        got["flags"] = flags = pf.copy()
    finally:
        pa = pf = None  # (views of memory that close() frees: nothing of them may reach a failure report)
        c.close()
    _same_stats(got, want_thr, flags)


def test_bad_depth_in_the_second_piece(pkg, cal, sim, pc):
    """a depth byte of 4 in the last CTU: the first piece was counted and packed when the second one finds it, and the call adds nothing"""
    n, probs, depth = pc["n"], pc["probs"], pc["depth"]
    assert n > hp.stage_ctus()
    bad = depth.copy()
    bad[n - 1, 15] = 4
    cal.add(probs[:300], depth[:300])
    sim.add(probs[:300], depth[:300])
    before = cal.get(), sim.info(), sim.eval(SIM_CANDS, "ai")
    assert int(before[0][0].sum()) > 300 and before[1]["ctus"] == 300
    for add in (cal.add, sim.add):
        with pytest.raises(pkg.EthCnnError) as e:
            add(probs, bad)
        assert e.value.code == pkg.ethcnn.ERR_FORMAT and "1 CTU(s)" in str(e.value) and "above 3" in str(e.value)
    _same_calib(cal.get(), before[0])
    assert sim.info() == before[1] and sim_ref.equal(sim.eval(SIM_CANDS, "ai"), before[2])
    cal.add(probs[300:600], depth[300:600])  # the next valid calls work, and give what the restatements give for the 600 CTUs
    sim.add(probs[300:600], depth[300:600])
    hist, rej = calib_ref.histogram(probs[:600], depth[:600])
    _same_calib(cal.get(), (hist, rej, 0))
    s = sim_ref.Set()
    s.add(probs[:600], depth[:600])
    assert sim.info() == s.info() and sim_ref.equal(sim.eval(SIM_CANDS, "ai"), s.evaluate(SIM_CANDS, sim_ref.GATES_AI))


# --------------------------------------------------------------------------------------------------------------- frame layout ---
def test_calib_add_frames_across_pieces(ctx, cal, fc):
    w, h, frames, probs, labels = fc["width"], fc["height"], fc["frames"], fc["probs"], fc["labels"]
    assert frames > hp.stage_frames(w, h)
    want = calib_ref.histogram_frames(probs, labels, w, h, skip_label_frames=1)
    assert want[1].tolist() == [1, 1, 1] and want[2] == frames * (h // 64)  # the reject of the first piece, the NaN and the 1.5 of the last frame
    cal.add_frames(probs, labels, w, h, skip_label_frames=1)
    got = cal.get()
    _same_calib(got, want)
    cal.reset()
    with Dev(ctx, probs, labels) as (dp, dl):
        cal.add_frames_device(dp, dl, w, h, frames, skip_label_frames=1)
        _same_calib(cal.get(), got)


def test_sim_add_frames_across_pieces(ctx, sim, sim2, fc, fc_set):
    w, h, per, piece, frames, cap = (fc[k] for k in ("width", "height", "per", "piece", "frames", "cap"))
    assert frames > piece == hp.stage_frames(w, h) and cap == piece * per
    s = fc_set
    sim.add_frames(fc["probs"], fc["labels"], w, h, skip_label_frames=1)
    sim_checks(sim, s, cap, fc["reject_at"], fc["labelled_at"], rejected=fc["rejected"])  # around the first CTU of the second piece
    assert sim.info()["sub_batches"] == 4 * frames
    for name, gates in (("ai", sim_ref.GATES_AI), ("ldp", sim_ref.GATES_LDP)):
        want = s.evaluate(SIM_CANDS, gates)
        assert not sim_ref.equal(want, s.evaluate(SIM_CANDS, sim_ref.GATES_NONE))  # gates do close
        assert sim_ref.equal(sim.eval(SIM_CANDS, name), want), name
    for cand in (SIM_CANDS[:1], SIM_CANDS[1:]):  # the two frames of the second piece, whole
        want = decide_ref.decide(s, cand, sim_ref.GATES_AI, 512, cap, (frames - piece) * per)
        got = sim.decide_frames(cand, "ai", w, h, first_frame=piece, nframes=frames - piece)
        assert want["codes"][fc["split_at"] - cap, 21] & decide_ref.REJECTED
        assert np.array_equal(got["codes"], want["codes"]) and np.array_equal(got["reach"], want["reach"])
        assert np.array_equal(got["planes"], decide_ref.planes_of(want["depth"], w, h))
    with Dev(ctx, fc["probs"], fc["labels"]) as (dp, dl):
        sim2.add_frames_device(dp, dl, w, h, frames, skip_label_frames=1)
    assert sim2.info() == sim.info()
    _same_codes(sim, sim2)
    _same_codes(sim, sim2, "ldp")


def test_compare_frames_from_pageable_memory(ctx, fc):
    """4936x3256: partial CTUs in the right column and the bottom row.  The second piece starts at CTU 2362 of frame 263, so what a CTU
    of it counts as checked depends on the kernel deriving the frame position from the global index"""
    a, b, planted = hp.frame_compare()
    n, piece, w, h = a.shape[0], hp.compare_ctus(), hp.COMPARE_W, hp.COMPARE_H
    assert n > piece and piece % fc["per"] != 0
    want = ref.compare(a, b, TOL, THR, w, h)
    assert want["worst_ctu"] == planted and min(planted) >= piece
    shifted = ref.compare(a[piece:], b[piece:], TOL, THR, w, h)  # the second piece as if it began a frame
    here = ref.compare(a[piece:], b[piece:], TOL, THR, w, h, first=piece)
    assert shifted["checked_a"] != here["checked_a"] and shifted["search_diff_ctus"] != here["search_diff_ctus"]
    flags = np.full(n, 0xEE, np.uint8)
    _same_stats(ctx.compare_frames(a, b, w, h, TOL, THR, want_flags=flags), want, flags)


def test_bad_label_in_the_second_piece_of_frames(pkg, cal, sim, fc, pc):
    w, h, frames, probs, labels = fc["width"], fc["height"], fc["frames"], fc["probs"], fc["labels"]
    assert frames > hp.stage_frames(w, h)
    bad = labels.copy()
    bad[-1, 0, 0] = 4  # CTU 0 of the last frame
    cal.add_frames(probs[:1], labels[:2], w, h, skip_label_frames=1)
    sim.add_frames(probs[:1], labels[:2], w, h, skip_label_frames=1)
    before = cal.get(), sim.info(), sim.eval(SIM_CANDS, "ai")
    assert int(before[0][0].sum()) > 3000 and before[1]["sub_batches"] == 4
    for add in (cal.add_frames, sim.add_frames):
        with pytest.raises(pkg.EthCnnError) as e:
            add(probs, bad, w, h, skip_label_frames=1)
        assert e.value.code == pkg.ethcnn.ERR_FORMAT and "1 CTU(s)" in str(e.value) and "above 3" in str(e.value)
    _same_calib(cal.get(), before[0])
    assert sim.info() == before[1] and sim_ref.equal(sim.eval(SIM_CANDS, "ai"), before[2])
    more_p, more_d = pc["probs"][:300], pc["depth"][:300]  # a following good add of 300 CTUs
    cal.add(more_p, more_d)
    sim.add(more_p, more_d)
    hist, rej, skipped = calib_ref.histogram_frames(probs[:1], labels[:2], w, h, skip_label_frames=1)
    hist2, rej2 = calib_ref.histogram(more_p, more_d)
    _same_calib(cal.get(), (hist + hist2, rej + rej2, skipped))
    s = sim_ref.Set()
    s.add_frames(probs[:1], labels[:2], w, h, skip_label_frames=1)
    s.add(more_p, more_d)
    assert sim.info() == s.info() and sim_ref.equal(sim.eval(SIM_CANDS, "ai"), s.evaluate(SIM_CANDS, sim_ref.GATES_AI))


# ---------------------------------------------------------------------------------------------------------------- sample sets ---
@pytest.mark.parametrize("kind", ["ai", "inter"])
def test_permuted_read_and_write_across_pieces(pkg, ctx, kind, tmp_path):
    """a set of more than 64 MB of records read in the order of a seed, whole, as a range that starts in the first piece and ends in
    the second, and into a file"""
    w, h, per = hp.GATHER_W, hp.GATHER_H, hp.GATHER_PER
    rb = hp.REC_AI if kind == "ai" else hp.REC_INTER
    piece, frames = hp.samples_read_records(rb), hp.gather_frames(rb)
    rng = np.random.default_rng(51 + (kind == "ai"))
    if kind == "ai":
        yuvs, labs = _seeded_files(rng, tmp_path, "ai", 1, frames)
        s = pkg.SampleSet(ctx, "ai", [32])
        s.add_sequence(w, h, yuvs[0], labs)
    else:
        yuvs, labs = _seeded_files(rng, tmp_path, "resi", 4, frames + 1)  # (frame 0 is the intra picture: not cut)
        s = pkg.SampleSet(ctx, "inter", [22, 27, 32, 37])
        s.add_sequence(w, h, yuvs, labs)
    out = str(tmp_path / "shuffled.dat")
    try:
        with s:
            count = s.count
            assert count == frames * per > piece and s.record_bytes == rb
            s.build()
            nat = s.read()
            if kind == "ai":
                lab = np.fromfile(labs[0], dtype=np.uint8).reshape(extract_cases.label_shape(w, h, frames))
                assert np.array_equal(nat, extract_cases.np_cut_ai(extract_cases.read_luma(yuvs[0], w, h), [lab], [32]))
            else:
                assert len(np.unique(nat[:, 10:20], axis=0)) == count  # (frame, CTU row, CTU column): every record is another one
            perm = pkg.ethcnn.sample_permutation(3, count)
            assert sorted(perm.tolist()) == list(range(count))
            want = nat[perm]
            assert np.array_equal(s.read(seed=3), want)
            first, n = 5, count - 7
            assert n > piece  # output records [0, piece) are the first launch of this read, [piece, n) its second
            assert np.array_equal(s.read(first, n, seed=3), want[first:first + n])
            s.write(out, seed=3)
            assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(-1, rb), want)
            assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in yuvs + labs + [out])  # no temporary file left
    finally:
        for p in yuvs + labs + [out]:  # (up to 117 MB of sources and 70 MB of records: not kept with the test's directory)
            if os.path.exists(p):
                os.remove(p)


def test_lstm_sample_file_across_pieces(pkg, tmp_path):
    """1824 samples of 37264 bytes: the writer's second piece holds the last 24.  The build itself uploads 76 MB of host records, more
    than one 64 MB slice of that copy"""
    rec = hp.lstm_records()
    assert rec.nbytes > hp.IO_BYTES
    out = str(tmp_path / "lstm.dat")
    c = pkg.EthCnn(device=0)
    try:
        c.load_synthetic(5, 8.0)
        with pkg.LstmSampleSet(c) as ls, pkg.LstmSampleSet(c) as by_slices:
            ls.build_from(rec)
            piece, count = hp.lstm_write_samples(), ls.count
            assert count == 1824 > piece and ls.skipped == 0
            got = ls.read()
            assert (got[:, 0] == 19).all() and len(np.unique(got[:, 64:64 + 4 * 465], axis=0)) > count // 2  # samples differ
            # the samples whose records all lie behind the first upload slice equal a build from those records alone (one slice)
            cut = hp.LSTM_TAIL_FRAME * 6
            assert cut * hp.REC_INTER > hp.IO_BYTES
            heads, tail_heads = pkg.ethcnn.lstm_samples_plan(rec)[0], pkg.ethcnn.lstm_samples_plan(rec[cut:])[0]
            m, mt = count // 4, len(tail_heads)
            assert mt == 48 and np.array_equal(tail_heads + cut, heads[m - mt:])
            tail = by_slices.build_from(rec[cut:]).read()
            assert by_slices.count == 4 * mt
            for slot in range(4):
                assert np.array_equal(got[slot * m + m - mt:(slot + 1) * m], tail[slot * mt:(slot + 1) * mt]), slot
            ls.write(out)
            assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(-1, hp.REC_LSTM), got)
            assert os.listdir(str(tmp_path)) == ["lstm.dat"]
    finally:
        c.close()
        if os.path.exists(out):
            os.remove(out)
