"""GPU: the ETH-LSTM sample sets (include/ethcnn.h "ETH-LSTM sample sets") against the host builder they replace,
get_LSTM_input.build_samples(records, gpu_vectors(ctx)), byte for byte: slots, several chunks and both pass shapes of the residual
CNN, mixed geometry with skipped heads, an inter SampleSet as the source, the hand-off to the LSTM trainer, the files, the driver
and the errors.  No tolerance anywhere.  CNN weights: Trainer(net="ldp").init_weights(seed) blobs."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import extract_cases
import grid_caps
import train_data_ldp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "hevc-complexity-reduction_amd")
REC_IN, REC_OUT = 16516, 37264


def ldp_records(width, height, frames, seed, first_frame=0):
    """one sequence's records, frame after frame (tests/train_data_ldp.py's content, the geometry and frame numbers of this case)"""
    per = (width // 64) * (height // 64)
    rec = np.frombuffer(train_data_ldp.make_records(per * frames, seed=seed, width=width, height=height), np.uint8).reshape(-1, REC_IN).copy()
    rec[:, 10:14] = (first_frame + np.arange(per * frames) // per).astype("<u4").view(np.uint8).reshape(-1, 4)
    return rec


@pytest.fixture(scope="module")
def G():
    return importlib.import_module("hevc-complexity-reduction_amd.get_LSTM_input")


@pytest.fixture(scope="module")
def cblob(pkg, ctx):
    t = pkg.Trainer(ctx, batch=8, net="ldp")
    t.init_weights(7)
    blob = t.get_blob()
    t.close()
    return blob


@pytest.fixture(scope="module")
def e(pkg, cblob):
    c = pkg.EthCnn(device=0)
    c.load_blob(cblob)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(G, e):
    """192x128 x 42 frames: 6 CTUs a frame, heads at frames 20, 30, 40 -> 18 per slot; and the host builder's samples"""
    rec = ldp_records(192, 128, 42, seed=5)
    want, skipped = G.build_samples(rec, G.gpu_vectors(e))
    assert want.shape == (72, REC_OUT) and skipped == 0
    return rec, want


def test_equals_the_host_builder_for_every_slot_choice(pkg, e, small):
    rec, want = small
    m = len(want) // 4
    for slots in (None, (0, 1, 2, 3), (0,), (1,), (2,), (3,), (1, 3), (3, 1)):
        with pkg.LstmSampleSet(e, slots=slots) as ls:
            assert ls.build_from(rec) is ls
            got = ls.read()
            assert ls.count == len(ls) == len(got) and ls.skipped == 0
        exp = want if slots is None else np.concatenate([want[s * m:(s + 1) * m] for s in sorted(slots)])
        assert np.array_equal(got, exp), slots
    with pkg.LstmSampleSet(e) as ls:  # a part of the set; bytes and a file path as the source
        ls.build_from(rec.tobytes())
        assert np.array_equal(ls.read(5, 9), want[5:14]) and ls.read(72, 0).shape == (0, REC_OUT)


def test_several_chunks_and_both_pass_shapes(pkg, G, e):
    # 2412 records: one default chunk is above the single-launch limit of 2304 CTUs.  It is also the one build that takes k_resi_repack
    # into a second trip of its grid-stride loop (all records are one chunk of the default 8192), so the frame count follows the cap of
    # the device in hand where that is larger (MI355X: 402 frames, 2412 records > 2048)
    cap = grid_caps.lstm_repack(grid_caps.cus(e))
    rec = ldp_records(192, 128, max(402, cap // 6 + 2), seed=6)
    assert len(rec) >= 2400 and cap < len(rec) <= 8192
    want, skipped = G.build_samples(rec, G.gpu_vectors(e))
    with pkg.LstmSampleSet(e) as a, pkg.LstmSampleSet(e, chunk_ctus=64) as b:
        ga, gb = a.build_from(rec).read(), b.build_from(rec).read()
        assert a.skipped == b.skipped == skipped
    assert np.array_equal(ga, gb)
    assert np.array_equal(ga, want)


def test_mixed_geometry_and_skipped_heads(pkg, G, e):
    both = np.concatenate([ldp_records(192, 128, 42, seed=8), ldp_records(256, 192, 35, seed=9)])
    rec = both[6 * 12:]  # the file starts at frame 12 of the first sequence: its heads at frames 20 and 30 reach before the start
    want, skipped = G.build_samples(rec, G.gpu_vectors(e))
    assert skipped == 12 and len(want) == 4 * (6 + 2 * 12)
    with pkg.LstmSampleSet(e, chunk_ctus=96) as ls:
        got = ls.build_from(rec).read()
        assert ls.skipped == skipped and ls.count == len(want)
    assert np.array_equal(got, want)
    with pkg.LstmSampleSet(e) as ls:  # nothing but skipped heads: an empty, built set
        ls.build_from(both[6 * 15: 6 * 25])
        assert ls.count == 0 and ls.skipped == 6 and ls.read().shape == (0, REC_OUT)


def test_from_an_inter_sample_set(pkg, e, tmp_path):
    rng = np.random.default_rng(21)
    qps = [22, 27, 32, 37]
    with pkg.SampleSet(e, kind="inter", qps=qps) as st:
        for name, w, h, frames in (("a", 128, 64, 32), ("b", 200, 136, 25)):
            yuvs, labs = [], []
            for q in qps:
                yuvs.append(str(tmp_path / ("resi_%s_qp%d.yuv" % (name, q))))
                labs.append(str(tmp_path / ("%s_qp%d_CUDepth.dat" % (name, q))))
                with open(yuvs[-1], "wb") as f:
                    f.write(extract_cases.synth_yuv(rng, w, h, frames))
                with open(labs[-1], "wb") as f:
                    f.write(rng.integers(0, 4, int(np.prod(extract_cases.label_shape(w, h, frames))), dtype=np.uint8).tobytes())
            st.add_sequence(w, h, yuvs, labs)
        st.build()
        before = st.read()
        assert len(before) == 31 * 2 + 24 * 6
        with pkg.LstmSampleSet(e, chunk_ctus=32) as a, pkg.LstmSampleSet(e) as b:
            ga = a.build_from(st).read()
            gb = b.build_from(before).read()
            assert a.count == b.count == 4 * (2 * 2 + 6) and a.skipped == b.skipped == 0
        assert np.array_equal(ga, gb)
        assert np.array_equal(st.read(), before)  # the set was only read
        info = ga[:, :64]
        assert (info[:, 0] == 19).all() and sorted(set(info[:10, 10].tolist())) == [20, 30]


def _trained(pkg, e, feed, qps=None):
    t = pkg.LstmTrainer(e, batch=8, seed=3)
    if qps is not None:
        t.set_qps(qps)
    kept = feed(t)
    assert kept == t.num_samples(0)
    t.init_weights(11)
    t.run(1, 20)  # dropout on
    probs = t.debug_fetch(pkg.ethcnn.LDBG_PROBS)
    blob, acc = t.get_blob(with_accum=True)
    ev = t.evaluate(0, n=kept, want_probs=True)
    t.close()
    return kept, probs, blob, acc, ev


def _same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for x, y in zip(a[4], b[4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_hand_off_to_the_trainer(pkg, e, small):
    rec, want = small
    ref_all = _trained(pkg, e, lambda t: t.set_samples(0, want))
    assert ref_all[0] == 72
    with pkg.LstmSampleSet(e) as ls:
        ls.build_from(rec)
        got = _trained(pkg, e, lambda t: t.set_samples(0, ls, take=True))
        assert ls.count == 0 and len(ls) == 0
        with pytest.raises(pkg.EthCnnError):
            ls.read(0, 1)
    _same(got, ref_all)
    ref_27 = _trained(pkg, e, lambda t: t.set_samples(0, want), qps=[27])
    assert ref_27[0] == 18
    for take in (True, False):  # a four-slot set under a one-QP selection: the kept samples are compacted into a copy
        with pkg.LstmSampleSet(e) as ls:
            ls.build_from(rec)
            got = _trained(pkg, e, lambda t: t.set_samples(0, ls, take=take), qps=[27])
            assert ls.count == (0 if take else 72)
            if not take:
                assert np.array_equal(ls.read(), want)
        _same(got, ref_27)
    with pkg.LstmSampleSet(e) as ls:  # everything kept, no take: a plain copy, the set keeps its samples
        ls.build_from(rec)
        _same(_trained(pkg, e, lambda t: t.set_samples(0, ls)), ref_all)
        assert np.array_equal(ls.read(), want)
        t = pkg.LstmTrainer(e, batch=8)
        t.set_qps([30])
        with pytest.raises(pkg.EthCnnError) as ei:
            t.set_samples(0, ls, take=True)
        assert ei.value.code == pkg.ethcnn.ERR_FORMAT and ls.count == 72
        t.close()


def test_files_and_the_tool(pkg, G, e, cblob, small, tmp_path):
    rec, want = small
    with pkg.LstmSampleSet(e) as ls:
        ls.build_from(rec)
        ls.write(str(tmp_path / "direct.dat"))
        assert np.array_equal(np.fromfile(str(tmp_path / "direct.dat"), np.uint8).reshape(-1, REC_OUT), ls.read())
    assert sorted(os.listdir(str(tmp_path))) == ["direct.dat"]  # no temp file left
    (tmp_path / "ldp.dat").write_bytes(rec.tobytes())
    with pkg.LstmSampleSet(e, slots=[2]) as ls:
        assert np.array_equal(ls.build_from(str(tmp_path / "ldp.dat")).read(), want[36:54])
    cprefix = str(tmp_path / "cnn.dat")
    pkg.ethcnn.write_ckpt_blob(cprefix, cblob)
    r = subprocess.run([sys.executable, os.path.join(PKG_DIR, "get_LSTM_input.py"), "--model", cprefix, "--input", "ldp.dat", "--out", "lstm.dat",
                        "--seed", "4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "252 records -> 72 samples (18 per QP); 0 skipped (a reference before the start of the file)"
    assert np.array_equal(np.fromfile(str(tmp_path / "lstm.dat"), np.uint8).reshape(-1, REC_OUT), want)
    assert np.array_equal(np.fromfile(str(tmp_path / "lstm.dat_shuffled"), np.uint8).reshape(-1, REC_OUT), G.shuffle_groups(want, 4))


def test_driver_trains_from_ldp_files(pkg, G, e, cblob, tmp_path):
    train, valid = ldp_records(192, 128, 42, seed=31), ldp_records(192, 128, 32, seed=32)
    (tmp_path / "ldp_train.dat").write_bytes(train.tobytes())
    (tmp_path / "ldp_valid.dat").write_bytes(valid.tobytes())
    pkg.ethcnn.write_ckpt_blob(str(tmp_path / "cnn.dat"), cblob)
    for name, data in (("train.dat", train), ("valid.dat", valid)):  # get_LSTM_input.py's unshuffled <out>
        G.build_samples(data, G.gpu_vectors(e))[0].tofile(str(tmp_path / name))
    drv = os.path.join(PKG_DIR, "train_LSTM_CTU64.py")
    common = ["--qp", "27", "--iters", "30", "--batch", "8", "--seed", "2"]
    runs = {"hbm": ["--ldp-train", "ldp_train.dat", "--ldp-valid", "ldp_valid.dat", "--cnn-model", "cnn.dat", "--models", "m_hbm"],
            "file": ["--train", "train.dat", "--valid", "valid.dat", "--models", "m_file"]}
    out = {}
    for k, args in runs.items():
        r = subprocess.run([sys.executable, drv] + args + common, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[k] = r.stdout
    assert "QP 27: 18 of 18 training and 12 of 12 validation samples" in out["hbm"]
    assert "QP 27: 18 of 72 training and 12 of 48 validation samples" in out["file"]
    assert not [f for f in os.listdir(str(tmp_path)) if "lstm" in f]  # no 37264-byte file in between
    a = pkg.ethcnn.read_ckpt_lstm_blob(str(tmp_path / "m_hbm" / "model.dat"))
    b = pkg.ethcnn.read_ckpt_lstm_blob(str(tmp_path / "m_file" / "model.dat"))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = pkg.EthCnn(device=0)
    c.load_lstm_checkpoint(str(tmp_path / "m_hbm" / "model.dat"))
    assert np.array_equal(c.get_lstm_blob().view(np.uint32), a.view(np.uint32))
    c.close()
    r = subprocess.run([sys.executable, drv] + runs["hbm"] + ["--qp", "30", "--iters", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "22 27 32 37" in r.stderr
    r = subprocess.run([sys.executable, drv] + runs["hbm"] + ["--train", "train.dat"] + common, cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "cannot be combined" in r.stderr


def test_errors(pkg, e, small):
    E = pkg.ethcnn
    rec, want = small

    def code(fn):
        with pytest.raises(pkg.EthCnnError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    bare = pkg.EthCnn(device=0)
    with pkg.LstmSampleSet(bare) as ls:
        assert code(lambda: ls.build_from(rec))[0] == E.ERR_NOWEIGHTS
    bare.close()
    with pkg.SampleSet(e, kind="ai", qps=[32]) as ai_set, pkg.SampleSet(e, kind="inter") as unbuilt, pkg.LstmSampleSet(e) as ls:
        assert code(lambda: ls.build_from(ai_set))[0] == E.ERR_FORMAT
        assert code(lambda: ls.build_from(unbuilt))[0] == E.ERR_FORMAT
        assert code(lambda: ls.build_from(rec.reshape(-1)[:-1]))[0] == E.ERR_FORMAT
        assert code(lambda: ls.build_from(np.empty(0, np.uint8)))[0] == E.ERR_FORMAT
        assert code(lambda: ls.read())[0] == E.ERR_ARG  # not built
    for slots in ((4,), (-1,), (1, 1), (0, 1, 2, 3, 0)):
        assert code(lambda: pkg.LstmSampleSet(e, slots=slots))[0] == E.ERR_ARG, slots
    for chunk in (48, -32, 31, 1 << 20):
        assert code(lambda: pkg.LstmSampleSet(e, chunk_ctus=chunk))[0] == E.ERR_ARG, chunk
    with pkg.LstmSampleSet(e, max_bytes=1) as ls:
        c, msg = code(lambda: ls.build_from(rec))
        need = int(re.search(r"need (\d+) bytes", msg).group(1))
        assert c == E.ERR_NOMEM and need > 72 * REC_OUT
    with pkg.LstmSampleSet(e, max_bytes=need - 1) as ls:
        c, msg = code(lambda: ls.build_from(rec))
        assert c == E.ERR_NOMEM and str(need) in msg and ls.count == 0
        ls.build_from(rec[:6 * 31])  # with enough room, on the same object
        assert np.array_equal(ls.read(), np.concatenate([want[s * 18: s * 18 + 12] for s in range(4)]))
    with pkg.LstmSampleSet(e, max_bytes=need) as ls:
        assert np.array_equal(ls.build_from(rec).read(), want)
