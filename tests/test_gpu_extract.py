"""Sample sets on the GPU (include/ethcnn.h "sample sets"): every comparison is byte for byte.  The fixture holds what the reference's
own Extract_Data scripts write for the cases of extract_cases.py."""
import os
import sys

import numpy as np
import pytest

import extract_cases as ec
import grid_caps
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG_DIR = os.path.join(ROOT, "hevc-complexity-reduction_amd")


@pytest.fixture(scope="module")
def golden():
    return ec.load_golden()


def inputs(case, golden, directory):
    return ec.make_inputs(case, str(directory), golden["labels_" + case] if "labels_" + case in golden.files else None)


def build_set(pkg, ctx, case, seqs, **kw):
    c = ec.CASES[case]
    s = pkg.SampleSet(ctx, c["kind"], c["qps"], order="ra" if c["config"] == "RA" else "encode", **kw)
    for name, w, h, yuvs, labs in seqs:
        s.add_sequence(w, h, yuvs[0] if c["kind"] == "ai" else yuvs, labs)
    return s


@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_build_read_write_equal_the_reference(pkg, ctx, golden, case, tmp_path):
    want = golden["records_" + case]
    with build_set(pkg, ctx, case, inputs(case, golden, tmp_path / "in")) as s:
        assert s.count == ec.EXPECTED_COUNT[case] and s.count * s.record_bytes == want.size
        s.build()
        assert np.array_equal(s.read().reshape(-1), want)
        assert np.array_equal(s.read(3, 5).reshape(-1), want.reshape(-1, s.record_bytes)[3:8].reshape(-1))
        out = tmp_path / "set.dat"
        s.write(str(out))
        assert np.array_equal(np.fromfile(str(out), dtype=np.uint8), want)
        assert sorted(os.listdir(str(tmp_path))) == ["in", "set.dat"]  # no temporary file left


@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_drivers_write_the_reference_files(pkg, golden, case, tmp_path):
    sys.path.insert(0, PKG_DIR)
    import extract_data_AI
    import extract_data_LDP_LDB_RA
    c = ec.CASES[case]
    seqs = inputs(case, golden, tmp_path / "in")
    lst = tmp_path / "seqs.txt"
    lst.write_text("".join("%s %d %d\n" % s[:3] for s in seqs))
    argv = ["--yuv-dir", str(tmp_path / "in"), "--info-dir", str(tmp_path / "in"), "--sequences", str(lst), "--set", "train", "--seed", "9",
            "--out-dir", str(tmp_path / "out"), "--qps"] + [str(q) for q in c["qps"]]
    if c["kind"] == "ai":
        assert extract_data_AI.main(argv) == 0
    else:
        assert extract_data_LDP_LDB_RA.main(argv + ["--config", c["config"]]) == 0
    name = "%s_Train_%d.dat" % (c["config"], ec.EXPECTED_COUNT[case])
    assert sorted(os.listdir(str(tmp_path / "out"))) == [name, name + "_shuffled"]
    want = golden["records_" + case]
    assert np.array_equal(np.fromfile(str(tmp_path / "out" / name), dtype=np.uint8), want)
    rb = 4992 if c["kind"] == "ai" else 16516
    perm = pkg.ethcnn.sample_permutation(9, ec.EXPECTED_COUNT[case])
    got = np.fromfile(str(tmp_path / "out" / (name + "_shuffled")), dtype=np.uint8)
    assert np.array_equal(got, want.reshape(-1, rb)[perm].reshape(-1))


def _upload_planes(pkg, ctx, planes, base_off, pitch):
    """[F, H, W] uint8 -> a device buffer holding the frames at byte offset base_off with `pitch` bytes between rows"""
    F, H, W = planes.shape
    host = np.zeros((F, H, pitch), dtype=np.uint8)
    host[:, :, :W] = planes
    buf = pkg.ethcnn.DeviceBuffer(ctx, base_off + host.nbytes + 64)
    flat = np.concatenate([np.zeros(base_off, np.uint8), host.reshape(-1)])
    buf.upload(flat)
    return buf, buf.ptr + base_off, H * pitch


@pytest.mark.parametrize("w,h", [(4928, 3264), (1920, 1080)])
@pytest.mark.parametrize("kind", ["ai", "inter"])
def test_cut_device_against_numpy(pkg, ctx, kind, w, h):
    E = pkg.ethcnn
    rng = np.random.default_rng(w + (kind == "ai"))
    nplanes, qps = (1, [22, 37, 0, 51, 30]) if kind == "ai" else (4, [37, 22, 32, 27])
    F = 2
    if (w, h) == (4928, 3264):
        # the large picture is the case that takes the cut kernels' grid-stride loops into a second trip: as many frames as pass the
        # cap of the device in hand, and never fewer than two (MI355X: 2 frames = 7854 records > 4096 All-Intra / 2048 inter)
        cap = (grid_caps.cut_ai if kind == "ai" else grid_caps.cut_inter)(grid_caps.cus(ctx))
        F = max(2, cap // ((h // 64) * (w // 64)) + 1)
        assert F * (h // 64) * (w // 64) > cap
    lumas = [rng.integers(0, 256, (F, h, w), dtype=np.uint8) for _ in range(nplanes)]
    labels = [rng.integers(0, 4, (F, h // 16, w // 16), dtype=np.uint8) for _ in qps]
    nrec = F * (h // 64) * (w // 64)
    assert h // 64 == (51 if h == 3264 else 16)  # 1080: floor, the ragged 56 rows are dropped
    if kind == "ai":
        want = ec.np_cut_ai(lumas[0], labels, qps)
    else:
        want = ec.np_cut_inter(lumas, labels, qps, list(range(5, 5 + F)), 300)
    rb = want.shape[1]
    lab_bufs = []
    for lab in labels:
        b = E.DeviceBuffer(ctx, lab.nbytes)
        b.upload(lab)
        lab_bufs.append(b)
    out = E.DeviceBuffer(ctx, (nrec + 2) * rb)
    results = []
    for base_off, pad in ((0, 0), (4, 4), (1, 3), (16, 32)):  # 16-byte aligned, 4-byte aligned, unaligned, aligned with a wider pitch
        ups = [_upload_planes(pkg, ctx, l, base_off, w + pad) for l in lumas]
        out.upload(np.full((nrec + 2) * rb, 0x5A, dtype=np.uint8))
        E.cut_device(ctx, E.SAMPLES_AI if kind == "ai" else E.SAMPLES_INTER, qps, w, h, F, [u[1] for u in ups], [w + pad] * nplanes,
                     [u[2] for u in ups], [b.ptr for b in lab_bufs], out.ptr, record_offset=1, frame_number=5, seq_number=300)
        ctx.synchronize()
        got = out.download(np.uint8, (nrec + 2) * rb).reshape(nrec + 2, rb)
        assert np.all(got[0] == 0x5A) and np.all(got[-1] == 0x5A)  # nothing outside the records asked for
        assert np.array_equal(got[1:-1], want), (base_off, pad)
        results.append(got[1:-1].copy())
        for u in ups:
            u[0].free()
    for b in lab_bufs + [out]:
        b.free()


@pytest.mark.parametrize("case", ["ai4", "ra"])
def test_shuffled_read_and_write(pkg, ctx, golden, case, tmp_path):
    with build_set(pkg, ctx, case, inputs(case, golden, tmp_path / "in")) as s:
        s.build()
        nat = s.read()
        p3, p4 = pkg.ethcnn.sample_permutation(3, s.count), pkg.ethcnn.sample_permutation(4, s.count)
        assert not np.array_equal(p3, p4)
        assert np.array_equal(s.read(seed=3), nat[p3])
        assert np.array_equal(s.read(seed=4), nat[p4])
        assert np.array_equal(s.read(2, 7, seed=3), nat[p3[2:9]])
        a, b, c = (str(tmp_path / n) for n in "abc")
        s.write(a, seed=3)
        s.write(b, seed=3)
        s.write(c, seed=4)
        fa, fb, fc = (np.fromfile(n, dtype=np.uint8) for n in (a, b, c))
        assert np.array_equal(fa, nat[p3].reshape(-1)) and np.array_equal(fa, fb) and not np.array_equal(fa, fc)


@pytest.mark.parametrize("case,net", [("ai4", "ai"), ("ldp", "ldp")])
def test_hand_off_to_a_trainer(pkg, ctx, golden, case, net, tmp_path):
    E = pkg.ethcnn
    seqs = inputs(case, golden, tmp_path / "in")
    records = golden["records_" + case]
    qps = ec.CASES[case]["qps"]

    def run(feed):
        with pkg.Trainer(ctx, batch=8, seed=21, net=net) as tr:
            tr.init_weights(4)
            feed(tr)
            if net == "ai":
                tr.set_qps(qps)
            probs = tr.evaluate(E.SET_TRAIN, qps[1], n=ec.EXPECTED_COUNT[case], want_probs=True)[2]
            vprobs = tr.evaluate(E.SET_VALID, qps[2], n=ec.EXPECTED_COUNT[case], want_probs=True)[2]
            tr.run(1, 20)
            blob, acc = tr.get_blob(with_accum=True)
        return probs, vprobs, blob, acc

    def from_host(tr):
        tr.set_samples(E.SET_TRAIN, records)
        tr.set_samples(E.SET_VALID, records)

    def from_set(take):
        def feed(tr):
            with build_set(pkg, ctx, case, seqs) as s:
                s.build()
                tr.set_samples(E.SET_VALID, s)  # a copy: the set keeps its records
                assert s.count == ec.EXPECTED_COUNT[case]
                tr.set_samples(E.SET_TRAIN, s, take=take)
                assert s.count == (0 if take else ec.EXPECTED_COUNT[case])
            # the set is closed here; the trainer trains on
        return feed

    want = run(from_host)
    for take in (False, True):
        got = run(from_set(take))
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), take
    # kind / net mismatch
    other = "ldp" if net == "ai" else "ai"
    with pkg.Trainer(ctx, batch=8, seed=21, net=other) as tr, build_set(pkg, ctx, case, seqs) as s:
        s.build()
        with pytest.raises(E.EthCnnError) as e:
            tr.set_samples(E.SET_TRAIN, s)
        assert e.value.code == E.ERR_FORMAT
        assert s.count == ec.EXPECTED_COUNT[case]
    with pkg.Trainer(ctx, batch=8, seed=21, net=net) as tr, build_set(pkg, ctx, case, seqs) as s:
        with pytest.raises(E.EthCnnError) as e:  # not built yet
            tr.set_samples(E.SET_TRAIN, s)
        assert e.value.code == E.ERR_ARG


def test_errors_and_the_byte_limit(pkg, ctx, golden, tmp_path):
    E = pkg.ethcnn
    ai = inputs("ai4", golden, tmp_path / "ai")
    ldp = inputs("ldp", golden, tmp_path / "ldp")
    with pkg.SampleSet(ctx, "ai", [22, 27, 32, 37]) as s:
        name, w, h, yuvs, labs = ai[0]
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(60, h, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT
        with open(yuvs[0], "r+b") as f:
            f.truncate(os.path.getsize(yuvs[0]) - 100)
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(yuvs[0]) in str(e.value)
        name, w, h, yuvs, labs = ai[1]
        with open(labs[2], "r+b") as f:
            f.truncate(os.path.getsize(labs[2]) - 1)
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(labs[2]) in str(e.value)
        assert s.count == 0
    with pkg.SampleSet(ctx, "inter", [22, 27, 32, 37]) as s:
        name, w, h, yuvs, labs = ldp[0]
        with open(yuvs[3], "ab") as f:
            f.write(b"\0" * (w * h * 3 // 2))
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs, labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(yuvs[3]) in str(e.value)
    # a set that needs more than its own limit: refused with the byte count, nothing allocated, the context goes on working
    big = tmp_path / "big"
    big.mkdir()
    w, h, frames = 512, 256, 10  # 320 records = 1.6 MB
    rng = np.random.default_rng(1)
    (big / "Big.yuv").write_bytes(ec.synth_yuv(rng, w, h, frames))
    (big / "Info_1_AI_Big_qp32_CUDepth.dat").write_bytes(rng.integers(0, 4, frames * (h // 16) * (w // 16), dtype=np.uint8).tobytes())
    with pkg.SampleSet(ctx, "ai", [32], max_bytes=1 << 20) as s:
        s.add_sequence(w, h, str(big / "Big.yuv"), [str(big / "Info_1_AI_Big_qp32_CUDepth.dat")])
        assert s.count == 320
        with pytest.raises(E.EthCnnError) as e:
            s.build()
        assert e.value.code == E.ERR_NOMEM and str(320 * 4992) in str(e.value)
        with pytest.raises(E.EthCnnError):
            s.read(0, 1)
    ctx.load_synthetic(3, 1.0)
    ctx.set_thresholds(0.5, 0.5)
    luma = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    assert ctx.predict_luma(luma, 128, 64, 1, 32).shape[-1] == 21
    with pkg.SampleSet(ctx, "ai", [32], max_bytes=2 << 20) as s:  # the same set under a limit it fits
        s.add_sequence(w, h, str(big / "Big.yuv"), [str(big / "Info_1_AI_Big_qp32_CUDepth.dat")])
        lab = np.fromfile(str(big / "Info_1_AI_Big_qp32_CUDepth.dat"), dtype=np.uint8).reshape(frames, h // 16, w // 16)
        assert np.array_equal(s.build().read(), ec.np_cut_ai(ec.read_luma(str(big / "Big.yuv"), w, h), [lab], [32]))


@pytest.mark.parametrize("case,script", [("ai4", "train_CNN_CTU64"), ("ldp", "train_resi_CNN_CTU64")])
def test_training_from_video_equals_training_from_the_files(pkg, ctx, golden, case, script, tmp_path):
    sys.path.insert(0, PKG_DIR)
    driver = __import__(script)
    seqs = inputs(case, golden, tmp_path / "in")
    lst = tmp_path / "seqs.txt"
    lst.write_text("".join("%s %d %d\n" % s[:3] for s in seqs))
    sample_file = str(tmp_path / "samples.dat")
    with build_set(pkg, ctx, case, seqs) as s:
        s.build().write(sample_file)
    common = ["--iters", "200", "--batch", "8", "--seed", "3"] + (["--model-type", "3"] if case == "ai4" else [])
    assert driver.main(common + ["--train", sample_file, "--valid", sample_file, "--models", str(tmp_path / "a")]) == 0
    assert driver.main(common + ["--yuv-dir", str(tmp_path / "in"), "--info-dir", str(tmp_path / "in"), "--sequences", str(lst),
                                 "--models", str(tmp_path / "b")]) == 0
    for suffix in (".index", ".data-00000-of-00001"):
        a = (tmp_path / "a" / ("model.dat" + suffix)).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "b" / ("model.dat" + suffix)).read_bytes()
    assert (tmp_path / "a" / "loss_accuracy_list.dat").read_bytes() == (tmp_path / "b" / "loss_accuracy_list.dat").read_bytes()
