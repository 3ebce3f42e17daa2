"""Sample sets from high-bit-depth and non-4:2:0 video on the GPU (include/ethcnn.h "sample sets", source format): every comparison is
byte for byte.  The deep cut kernel is compared with the numpy restatement of the records over numpy-narrowed planes; the builder, the
drivers and the threshold tool with what the 8-bit 4:2:0 form of the same picture gives, which for the cases of extract_cases.py is
the fixture written by the reference's own scripts (extract16_cases.py: how a deep file narrows back to it)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import extract16_cases as e16
import extract_cases as ec
import grid_caps
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG_DIR = os.path.join(ROOT, "hevc-complexity-reduction_amd")
QPS = [22, 37, 0, 51, 30]
ALIGNMENTS = ((0, 0), (16, 32), (4, 4), (2, 6))  # base offset and pitch padding in bytes: the 16-byte path (twice), the 4-byte and the 2-byte one


@pytest.fixture(scope="module")
def golden():
    return ec.load_golden()


def _deep_planes(rng, F, h, w, depth):
    """two thirds of the samples within the depth, one third anywhere in 16 bits: below 16 bits the clamp to 255 is hit"""
    s = rng.integers(0, 1 << depth, (F, h, w), dtype=np.uint16)
    wild = rng.integers(0, 3, (F, h, w)) == 0
    s[wild] = rng.integers(0, 1 << 16, int(wild.sum()), dtype=np.uint16)
    return s


def _upload16(pkg, ctx, planes, base_off, pitch_bytes):
    """[F, H, W] uint16 -> device bytes: the frames at byte offset base_off, pitch_bytes between rows, 0xEE in every gap"""
    F, H, W = planes.shape
    host = np.full((F, H, pitch_bytes), 0xEE, dtype=np.uint8)
    host[:, :, :2 * W] = np.ascontiguousarray(planes.astype("<u2")).view(np.uint8).reshape(F, H, 2 * W)
    buf = pkg.ethcnn.DeviceBuffer(ctx, base_off + host.nbytes + 64)
    buf.upload(np.concatenate([np.full(base_off, 0xEE, np.uint8), host.reshape(-1), np.full(64, 0xEE, np.uint8)]))
    return buf, buf.ptr + base_off, H * pitch_bytes


# one block with both records in flight; ragged edges dropped; an odd count (the second slot of the last block is off); and, at 10 bits
# only, as many 1920x1080 frames (None) as take the grid-stride loop into a second trip
SHAPES = [(w, h, frames, depth) for (w, h, frames) in ((128, 64, 1), (200, 136, 3), (192, 64, 3)) for depth in (8, 10, 12, 16)]
SHAPES.append((1920, 1080, None, 10))


@pytest.mark.parametrize("w,h,frames,depth", SHAPES)
def test_cut16_device_against_numpy(pkg, ctx, w, h, frames, depth):
    E = pkg.ethcnn
    per = (h // 64) * (w // 64)
    if frames is None:
        cap = grid_caps.cut_ai(grid_caps.cus(ctx))  # (the cut kernels launch at most 8 blocks per CU, two records per block and trip)
        frames = cap // per + 1
        assert frames * per > cap  # MI355X: 9 frames, 4320 records > 4096
    else:
        assert frames * per == {(128, 64): 2, (200, 136): 18, (192, 64): 9}[(w, h)]
    nrec = frames * per
    rng = np.random.default_rng(1000 * depth + w)
    deep = _deep_planes(rng, frames, h, w, depth)
    narrowed = np.minimum(deep >> (depth - 8), 255).astype(np.uint8)
    if depth < 16:
        assert (deep >> (depth - 8) > 255).any()  # the clamp is hit
    labels = [rng.integers(0, 4, (frames, h // 16, w // 16), dtype=np.uint8) for _ in QPS]
    want = ec.np_cut_ai(narrowed, labels, QPS)
    rb = want.shape[1]
    lab_bufs = []
    for lab in labels:
        b = E.DeviceBuffer(ctx, lab.nbytes)
        b.upload(lab)
        lab_bufs.append(b)
    out = E.DeviceBuffer(ctx, (nrec + 2) * rb)
    try:
        for base_off, pad in ALIGNMENTS:
            buf, ptr, fstride = _upload16(pkg, ctx, deep, base_off, 2 * w + pad)
            out.upload(np.full((nrec + 2) * rb, 0x5A, dtype=np.uint8))
            E.cut16_device(ctx, QPS, w, h, frames, ptr, depth, [b.ptr for b in lab_bufs], out.ptr, pitch_bytes=2 * w + pad,
                           frame_stride_bytes=fstride, record_offset=1)
            ctx.synchronize()
            got = out.download(np.uint8, (nrec + 2) * rb).reshape(nrec + 2, rb)
            buf.free()
            assert np.all(got[0] == 0x5A) and np.all(got[-1] == 0x5A), (base_off, pad)  # the guard records are intact
            assert np.array_equal(got[1:-1], want), (base_off, pad)
    finally:
        for b in lab_bufs + [out]:
            b.free()


def test_cut16_device_defaults_and_refusals(pkg, ctx):
    E = pkg.ethcnn
    w, h, F = 128, 64, 1
    rng = np.random.default_rng(5)
    deep = _deep_planes(rng, F, h, w, 10)
    lab = rng.integers(0, 4, (F, h // 16, w // 16), dtype=np.uint8)
    buf, ptr, fstride = _upload16(pkg, ctx, deep, 0, 2 * w)
    lb = E.DeviceBuffer(ctx, lab.nbytes)
    lb.upload(lab)
    out = E.DeviceBuffer(ctx, 2 * 4992)
    E.cut16_device(ctx, [32], w, h, F, ptr, 10, [lb.ptr], out.ptr)  # packed planes: the pitch and stride defaults
    ctx.synchronize()
    want = ec.np_cut_ai(np.minimum(deep >> 2, 255).astype(np.uint8), [lab], [32])
    assert np.array_equal(out.download(np.uint8, 2 * 4992).reshape(2, 4992), want)
    out.upload(np.full(2 * 4992, 0x5A, dtype=np.uint8))
    bad = [dict(bit_depth=7), dict(bit_depth=17), dict(ptr=ptr + 1), dict(pitch_bytes=2 * w + 1), dict(frame_stride_bytes=h * 2 * w + 1),
           dict(pitch_bytes=2 * w - 2), dict(qps=[52]), dict(w=63), dict(record_offset=-1), dict(out=out.ptr + 8)]
    for b in bad:
        with pytest.raises(E.EthCnnError) as e:
            E.cut16_device(ctx, b.get("qps", [32]), b.get("w", w), h, F, b.get("ptr", ptr), b.get("bit_depth", 10), [lb.ptr], b.get("out", out.ptr),
                           pitch_bytes=b.get("pitch_bytes"), frame_stride_bytes=b.get("frame_stride_bytes"), record_offset=b.get("record_offset", 0))
        assert e.value.code == E.ERR_ARG and str(e.value), b
    ctx.synchronize()
    assert np.all(out.download(np.uint8, 2 * 4992) == 0x5A)  # a refused call writes nothing
    for b in (buf, lb, out):
        b.free()


def _build(pkg, ctx, case, seqs):
    s = pkg.SampleSet(ctx, "ai", ec.CASES[case]["qps"])
    for name, w, h, yuvs, labs, depth, chroma in seqs:
        s.add_sequence(w, h, yuvs[0], labs, bit_depth=depth, chroma=chroma)
    return s


@pytest.mark.parametrize("case,form", [("ai4", "d10_420"), ("ai4", "d8_444"), ("ai4", "d12_400"), ("ai4", "mixed"), ("ai1", "d16_420")])
def test_build_read_write_equal_the_fixture(pkg, ctx, golden, case, form, tmp_path):
    want = golden["records_" + case]
    with _build(pkg, ctx, case, e16.make_inputs(case, form, tmp_path / "in", golden)) as s:
        assert s.count == ec.EXPECTED_COUNT[case] and s.count * s.record_bytes == want.size
        s.build()
        nat = s.read()
        assert np.array_equal(nat.reshape(-1), want)
        assert np.array_equal(s.read(3, 5), want.reshape(-1, 4992)[3:8])
        perm = pkg.ethcnn.sample_permutation(3, s.count)
        assert np.array_equal(s.read(seed=3), want.reshape(-1, 4992)[perm])
        plain, shuffled = str(tmp_path / "set.dat"), str(tmp_path / "set.dat_shuffled")
        s.write(plain)
        s.write(shuffled, seed=3)
        assert np.array_equal(np.fromfile(plain, dtype=np.uint8), want)
        assert np.array_equal(np.fromfile(shuffled, dtype=np.uint8), want.reshape(-1, 4992)[perm].reshape(-1))
        with pytest.raises(pkg.EthCnnError) as e:  # the format belongs to sequences added before the build
            s.set_source_format(8, 420)
        assert e.value.code == pkg.ethcnn.ERR_ARG and "built" in str(e.value)


def test_a_built_empty_set_refuses_a_format(pkg, ctx):
    with pkg.SampleSet(ctx, "ai", [32]) as s:
        s.set_source_format(10, 444)
        assert s.build().count == 0
        with pytest.raises(pkg.EthCnnError) as e:
            s.set_source_format(10, 444)
        assert e.value.code == pkg.ethcnn.ERR_ARG and "built" in str(e.value)


@pytest.mark.parametrize("form,columns,options", [("d10_420", 3, ["--input-bit-depth", "10"]), ("mixed", 5, []),
                                                  ("d12_400", 4, ["--input-chroma-format", "400"])])
def test_the_driver_writes_the_fixture_file(pkg, golden, form, columns, options, tmp_path):
    sys.path.insert(0, PKG_DIR)
    import extract_data_AI
    c = ec.CASES["ai4"]
    seqs = e16.make_inputs("ai4", form, tmp_path / "in", golden)
    lst = e16.sequences_file(tmp_path / "seqs.txt", seqs, columns)
    argv = ["--yuv-dir", str(tmp_path / "in"), "--info-dir", str(tmp_path / "in"), "--sequences", lst, "--set", "train", "--seed", "9",
            "--out-dir", str(tmp_path / "out"), "--qps"] + [str(q) for q in c["qps"]]
    assert extract_data_AI.main(argv + options) == 0
    name = "AI_Train_%d.dat" % ec.EXPECTED_COUNT["ai4"]
    assert sorted(os.listdir(str(tmp_path / "out"))) == [name, name + "_shuffled"]
    want = golden["records_ai4"]
    assert np.array_equal(np.fromfile(str(tmp_path / "out" / name), dtype=np.uint8), want)
    perm = pkg.ethcnn.sample_permutation(9, ec.EXPECTED_COUNT["ai4"])
    got = np.fromfile(str(tmp_path / "out" / (name + "_shuffled")), dtype=np.uint8)
    assert np.array_equal(got, want.reshape(-1, 4992)[perm].reshape(-1))


def test_training_from_10_bit_video_equals_training_from_the_8_bit_files(pkg, golden, tmp_path):
    sys.path.insert(0, PKG_DIR)
    import train_CNN_CTU64 as driver
    seqs8 = ec.make_inputs("ai4", str(tmp_path / "in8"), golden["labels_ai4"])
    seqs10 = e16.make_inputs("ai4", "d10_420", tmp_path / "in10", golden)
    lst = tmp_path / "seqs.txt"
    lst.write_text("".join("%s %d %d\n" % s[:3] for s in seqs8))
    common = ["--iters", "200", "--batch", "8", "--seed", "3", "--model-type", "3", "--sequences", str(lst)]
    assert driver.main(common + ["--yuv-dir", str(tmp_path / "in8"), "--info-dir", str(tmp_path / "in8"), "--models", str(tmp_path / "a")]) == 0
    assert driver.main(common + ["--yuv-dir", str(tmp_path / "in10"), "--info-dir", str(tmp_path / "in10"), "--input-bit-depth", "10",
                                 "--models", str(tmp_path / "b")]) == 0
    assert len(seqs10) == len(seqs8)
    for suffix in (".index", ".data-00000-of-00001"):
        a = (tmp_path / "a" / ("model.dat" + suffix)).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "b" / ("model.dat" + suffix)).read_bytes()
    assert (tmp_path / "a" / "loss_accuracy_list.dat").read_bytes() == (tmp_path / "b" / "loss_accuracy_list.dat").read_bytes()


def test_calibration_from_a_10_bit_sequence(pkg, oracle, tmp_path, capsys):
    from test_gpu_calib import _textured_sequence
    from test_gpu_score import _labels_from_texture
    spec = importlib.util.spec_from_file_location("calibrate16", os.path.join(ROOT, "tools", "calibrate_thresholds.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    w, h, frames, qp = 256, 192, 2, 32
    luma = _textured_sequence(32, w, h, frames)
    labels, models = str(tmp_path / "Info_test_256x192_qp32_nf2_CUDepth.dat"), str(tmp_path / "models")
    _labels_from_texture(luma).tofile(labels)
    rng = np.random.default_rng(7)
    yuv8, yuv10 = str(tmp_path / "seq8.yuv"), str(tmp_path / "seq10.yuv")
    e16.reencode(luma, yuv8, 8, 420, rng)
    e16.reencode(luma, yuv10, 10, 420, rng)
    os.mkdir(models)
    pkg.ethcnn.write_ckpt_blob(os.path.join(models, pkg.ethcnn.model_name_for_qp(qp)), oracle.synth_blob(1, 8.0))

    def run(tag, yuv, options):
        out, hist = str(tmp_path / (tag + "_Thr_info.txt")), str(tmp_path / (tag + ".hist"))
        rc = tool.main(["calibrate_thresholds.py", "--out", out, "--order", "ai", "--hist", hist] + options +
                       ["--yuv", yuv, str(w), str(h), str(qp), "--labels", labels, "--model-dir", models])
        cap = capsys.readouterr()
        report = cap.out.replace(out, "OUT")
        return rc, report, cap.err, (open(out).read() if rc == 0 else None), (open(hist, "rb").read() if rc == 0 else None)

    rc8, report8, _, thr8, hist8 = run("a", yuv8, [])
    rc10, report10, _, thr10, hist10 = run("b", yuv10, ["--input-bit-depth", "10"])
    assert rc8 == 0 and rc10 == 0
    assert report8 == report10 and "wrote OUT (ai order)" in report8 and thr8 == thr10 and hist8 == hist10
    # without the option the file reads as four 8-bit frames of another picture (a 10-bit 4:2:0 file always holds a whole number of
    # 8-bit frames): refused, or another histogram
    rc, report, err, thr, hist = run("c", yuv10, [])
    assert rc == 1 or hist != hist8, (rc, err)
