"""CPU: the checkpoint writer (ethcnn_ckpt_write_blob), the training-sample record parser, and the pins of the
float64 training restatement tests/train_ref.py that the GPU trainer's tests compare against."""
import os

import numpy as np
import pytest

import tf_shim
import tfckpt_writer
import train_data
import train_ref

REF_INDEX = "/root/reference/HM-16.5_Test_AI/bin/model_2000000_qp20~25.dat.index"


def _blob(seed):
    return np.random.default_rng(seed).standard_normal(1288210).astype(np.float32)


def test_write_read_roundtrip(pkg, tmp_path):
    blob = _blob(1)
    prefix = str(tmp_path / "m.dat")
    pkg.ethcnn.write_ckpt_blob(prefix, blob)
    assert sorted(os.listdir(str(tmp_path))) == ["m.dat.data-00000-of-00001", "m.dat.index"]  # no temp files left
    back = pkg.ethcnn.read_ckpt_blob(prefix)
    assert np.array_equal(back.view(np.uint32), blob.view(np.uint32))
    data = open(prefix + ".data-00000-of-00001", "rb").read()
    assert data == blob.astype("<f4").tobytes()
    for name, dtype, shape, shard, off, size, crc in pkg.ethcnn.read_ckpt_index(prefix + ".index"):
        assert dtype == 1 and shard == 0
        assert crc == tfckpt_writer.mask(tfckpt_writer.crc32c(data[off:off + size])), name


def test_written_index_parses_with_the_independent_reader(pkg, tmp_path):
    prefix = str(tmp_path / "m.dat")
    pkg.ethcnn.write_ckpt_blob(prefix, _blob(2))
    ent = tf_shim.read_bundle_index(prefix + ".index")
    table = {n: (tuple(s), o) for n, s, o in train_ref.ethcnn_np.TENSORS}
    assert set(ent) == set(table)
    for name, val in ent.items():
        shape, off = val[0], val[1]
        assert (tuple(shape), off) == table[name], name


@pytest.mark.skipif(not os.path.exists(REF_INDEX), reason="reference checkpoint index absent")
def test_written_index_matches_the_reference_table(pkg, tmp_path):
    prefix = str(tmp_path / "m.dat")
    pkg.ethcnn.write_ckpt_blob(prefix, _blob(3))
    mine = pkg.ethcnn.read_ckpt_index(prefix + ".index")
    ref = pkg.ethcnn.read_ckpt_index(REF_INDEX)
    assert [e[:6] for e in mine] == [e[:6] for e in ref]  # name, dtype, shape, shard, offset, size


def test_writer_rejects_bad_arguments(pkg, tmp_path):
    with pytest.raises(pkg.EthCnnError):
        pkg.ethcnn.write_ckpt_blob(str(tmp_path / "m.dat"), np.zeros(10, np.float32))
    with pytest.raises(pkg.EthCnnError) as ei:
        pkg.ethcnn.write_ckpt_blob(str(tmp_path / "absent_dir" / "m.dat"), _blob(4))
    assert ei.value.code == -2


def test_record_parser():
    recs = np.frombuffer(train_data.make_records(5, seed=3), np.uint8).reshape(5, 4992).copy()
    recs[2, 4160 + 16 * 30: 4160 + 16 * 31] = np.arange(16) % 4  # a distinct row at QP 30
    luma, lab = train_ref.parse_records(recs.tobytes(), [2, 0], [30, 30])
    assert np.array_equal(luma[0], recs[2, :4096])
    assert np.array_equal(lab[0], np.arange(16) % 4)
    assert np.array_equal(lab[1], recs[0, 4160 + 480: 4176 + 480])
    with pytest.raises(ValueError):
        train_ref.parse_records(recs.tobytes()[:-1], [0], 32)


def test_synthetic_labels_are_hevc_depths():
    recs = np.frombuffer(train_data.make_records(50, seed=4), np.uint8).reshape(50, 4992)
    for r in recs:
        d = r[4160:4176].reshape(4, 4)
        assert d.max() <= 3
        assert all(np.array_equal(r[4160 + 16 * q: 4176 + 16 * q], r[4160:4176]) for q in range(52))
        for qy in range(2):  # a 32x32 quadrant is either one depth-1 leaf, or split (every block >= 2), or depth 0 overall
            for qx in range(2):
                blk = d[2 * qy: 2 * qy + 2, 2 * qx: 2 * qx + 2]
                assert (blk == 0).all() or (blk == 1).all() or (blk >= 2).all()
        assert (d == 0).all() or (d > 0).all()


def test_forward_equals_the_pinned_inference_restatement(oracle):
    """train_ref's forward (isdrop = 0) == oracle/ethcnn_np.forward64 (pinned to the reference's executed net_CNN.py)"""
    blob = oracle.synth_blob(5, 4.0)
    recs = train_data.make_records(12, seed=6)
    luma, lab = train_ref.parse_records(recs, np.arange(12), 27)
    got = train_ref.net(__import__("torch").tensor(blob.astype(np.float64)), luma, lab, 27)["probs"].numpy()
    want = oracle.forward64(blob, luma.reshape(-1, 64, 64), 27)["probs"]
    assert np.abs(got - want).max() <= 1e-12


def _loss_numpy(p, lab):
    """numpy transcription of net_CTU64.py:97-111 (labels) and :178-206 (loss_list, accuracy_list), line by line"""
    n = len(lab)
    relu = lambda v: np.maximum(v, 0.0)  # noqa: E731
    y = lab.astype(np.float64).reshape(n, 4, 4)
    ap2 = y.reshape(n, 2, 2, 2, 2).mean(axis=(2, 4))
    ap4 = y.mean(axis=(1, 2)).reshape(n, 1)
    y16 = relu(y - 2).reshape(n, 16)
    y32 = (relu(ap2 - 1) - relu(ap2 - 2)).reshape(n, 4)
    y64 = relu(ap4 - 0) - relu(ap4 - 1)
    v32 = (relu(ap2 - 0) - relu(ap2 - 1)).reshape(n, 4)
    v16 = (relu(y - 1) - relu(y - 2)).reshape(n, 16)
    p64, p32, p16 = p[:, :1], p[:, 1:5], p[:, 5:]
    e = 1e-12
    l64 = (np.sum(-(y64 * np.log(p64 + e))) / (np.count_nonzero(y64) + e) +
           np.sum(-((1 - y64) * np.log((1 - p64) + e))) / (np.count_nonzero(1 - y64) + e)) / 2
    l32 = (np.sum(-(y32 * np.log(p32 + e)) * v32) / (np.count_nonzero(y32 * v32) + e) +
           np.sum(-((1 - y32) * np.log((1 - p32) + e)) * v32) / (np.count_nonzero((1 - y32) * v32) + e)) / 2
    l16 = (np.sum(-(y16 * np.log(p16 + e)) * v16) / (np.count_nonzero(y16 * v16) + e) +
           np.sum(-((1 - y16) * np.log((1 - p16) + e)) * v16) / (np.count_nonzero((1 - y16) * v16) + e)) / 2
    c32 = v32 * (np.round(p32) == np.round(y32))
    c16 = v16 * (np.round(p16) == np.round(y16))
    acc = [np.mean(np.round(p64) == np.round(y64)), np.sum(v32 * c32) / (np.sum(v32) + e), np.sum(v16 * c16) / (np.sum(v16) + e)]
    return np.array([l64, l32, l16]), np.array(acc)


def test_loss_and_accuracy_equal_the_numpy_transcription(oracle):
    blob = oracle.synth_blob(7, 6.0)
    recs = train_data.make_records(40, seed=8)
    luma, lab = train_ref.parse_records(recs, np.arange(40), 32)
    out, grad = train_ref.loss_and_grad(blob, luma, lab, 32)
    l3, a3 = _loss_numpy(out["probs"], lab)
    assert np.abs(out["loss_list"] - l3).max() <= 1e-12
    assert np.abs(out["accuracy_list"] - a3).max() <= 1e-12
    assert abs(out["total_loss"] - l3.sum()) <= 1e-12
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0


def test_gradient_matches_finite_differences(oracle):
    """spot check of the autograd path: central differences on a few parameters of every layer kind"""
    import torch
    blob = oracle.synth_blob(9, 2.0).astype(np.float64)
    recs = train_data.make_records(8, seed=10)
    luma, lab = train_ref.parse_records(recs, np.arange(8), 22)
    _, g = train_ref.loss_and_grad(blob, luma, lab, 22)
    offs = {n: o // 4 for n, _, o in train_ref.ethcnn_np.TENSORS}
    for name in ("Variable_12", "Variable_5", "h_fc1__16__w", "h_fc2__32__b", "y_conv_flat__64__w"):
        k = offs[name] + 3
        h = 1e-6
        bp, bm = blob.copy(), blob.copy()
        bp[k] += h
        bm[k] -= h
        fp = train_ref.net(torch.tensor(bp), luma, lab, 22)["total_loss"].item()
        fm = train_ref.net(torch.tensor(bm), luma, lab, 22)["total_loss"].item()
        assert abs((fp - fm) / (2 * h) - g[k]) <= 1e-5 * max(1.0, abs(g[k])), name


def test_rng_helpers_are_stable():
    """the documented draw() (include/ethcnn.h): fixed known values, so the formula cannot drift silently"""
    assert train_ref.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    idx, qp = train_ref.batch_of(1, 1, 64, 1000, [22, 37])
    assert idx.min() >= 0 and idx.max() < 1000 and set(qp) <= {22, 37}
    m1, m2 = train_ref.dropout_masks(1, 1, 4)
    assert m1.shape == (4, 448) and m2.shape == (4, 336)
