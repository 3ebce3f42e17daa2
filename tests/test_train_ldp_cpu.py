"""CPU: the pins of the float64 Low-Delay-P training restatement tests/train_ref_ldp.py (which the GPU trainer's LDP tests compare
against), its 16516-byte record parser, the synthetic LDP records, and the checkpoint table of the LDP model."""
import os

import numpy as np
import pytest
import torch

import test_train_cpu
import train_data_ldp
import train_ref
import train_ref_ldp

GOLDEN_INDEX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_LDP_2000000_qp22~37.dat.index")


def test_fc1_vectors_equal_the_pinned_resi_restatement(oracle):
    """train_ref_ldp's FC1 outputs == oracle/ethcnn_np.forward64(resi=True)["H1"] (pinned to the reference's LDP .meta graph)"""
    blob = oracle.synth_blob(5, 4.0)
    recs = train_data_ldp.make_records(12, seed=6)
    for qp in (22, 37):
        luma, lab = train_ref_ldp.parse_records(recs, np.arange(12), qp)
        got = train_ref_ldp.net(torch.tensor(blob.astype(np.float64)), luma, lab, qp)["H1"].numpy()
        want = oracle.forward64(blob, luma.reshape(-1, 64, 64), qp, resi=True)["H1"]
        assert np.abs(got - want).max() <= 1e-12


def test_loss_and_accuracy_equal_the_numpy_transcription(oracle):
    blob = oracle.synth_blob(7, 6.0)
    recs = train_data_ldp.make_records(40, seed=8)
    qps = np.resize([22, 27, 32, 37], 40)
    luma, lab = train_ref_ldp.parse_records(recs, np.arange(40), qps)
    out, grad = train_ref_ldp.loss_and_grad(blob, luma, lab, qps)
    l3, a3 = test_train_cpu._loss_numpy(out["probs"], lab)
    assert np.abs(out["loss_list"] - l3).max() <= 1e-12
    assert np.abs(out["accuracy_list"] - a3).max() <= 1e-12
    assert abs(out["total_loss"] - l3.sum()) <= 1e-12
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0


def test_scaling_is_the_ldp_graphs():
    """x = (x - 128) / 255 * 10 and qp / 51 * 0.18: a net whose only path is the QP feature into FC3 of head 64, and a check
    that the residual enters centred (a flat 128 residual gives zero features, so every FC1 output is its bias's leaky-ReLU)"""
    blob = np.zeros(1288210)
    off = {n: o // 4 for n, _, o in train_ref.ethcnn_np.TENSORS}
    blob[off["y_conv_flat__64__w"] + 48] = 1.0  # the qp row of W3 (head 64)
    blob[off["h_fc1__32__b"]: off["h_fc1__32__b"] + 128] = -0.5
    luma = np.full((1, 4096), 128, np.uint8)
    out = train_ref_ldp.net(torch.tensor(blob), luma, np.zeros((1, 16)), 37)
    assert abs(out["probs"][0, 0].item() - 1 / (1 + np.exp(-37 / 51 * 0.18))) <= 1e-15
    assert np.allclose(out["H1"][0, 64:192].numpy(), -0.1)


def test_gradient_matches_finite_differences(oracle):
    blob = oracle.synth_blob(9, 2.0).astype(np.float64)
    recs = train_data_ldp.make_records(8, seed=10)
    qps = [22, 27, 32, 37] * 2
    luma, lab = train_ref_ldp.parse_records(recs, np.arange(8), qps)
    _, g = train_ref_ldp.loss_and_grad(blob, luma, lab, qps)
    offs = {n: o // 4 for n, _, o in train_ref.ethcnn_np.TENSORS}
    for name in ("Variable_12", "Variable_5", "h_fc1__16__w", "h_fc2__32__b", "y_conv_flat__64__w"):
        k = offs[name] + 3
        h = 1e-6
        bp, bm = blob.copy(), blob.copy()
        bp[k] += h
        bm[k] -= h
        fp = train_ref_ldp.net(torch.tensor(bp), luma, lab, qps)["total_loss"].item()
        fm = train_ref_ldp.net(torch.tensor(bm), luma, lab, qps)["total_loss"].item()
        assert abs((fp - fm) / (2 * h) - g[k]) <= 1e-5 * max(1.0, abs(g[k])), name


def _extractor_record(qps, depths, patches, width, height, i_frame, i_line, i_col, i_seq):
    """extract_data_LDP_LDB_RA.py:122-156 (write_data) for one CTU, transcribed"""
    buf = (np.ones((64 + 4 * (1 + 16 + 4096),)) * 255).astype(np.uint8)
    buf[0] = 1
    buf[2], buf[3], buf[4], buf[5] = width % 256, width // 256, height % 256, height // 256
    buf[10], buf[11], buf[12], buf[13] = i_frame % 256, (i_frame >> 8) % 256, (i_frame >> 16) % 256, (i_frame >> 24) % 256
    buf[14], buf[15], buf[16], buf[17], buf[18], buf[19] = i_line % 256, i_line // 256, i_col % 256, i_col // 256, i_seq % 256, i_seq // 256
    for i_qp in range(len(qps)):
        s = 64 + i_qp * (1 + 16 + 4096)
        buf[s] = qps[i_qp]
        buf[s + 17: s + 17 + 4096] = patches[i_qp].reshape(4096)
        buf[s + 1: s + 17] = depths[i_qp].reshape(16)
    return buf


def test_record_parser_matches_the_extractor_layout():
    rng = np.random.default_rng(1)
    qps = [22, 27, 32, 37]
    recs = []
    for i in range(3):
        depths = [rng.integers(0, 4, 16).astype(np.uint8) for _ in qps]
        patches = [rng.integers(0, 256, 4096).astype(np.uint8) for _ in qps]
        recs.append((_extractor_record(qps, depths, patches, 416, 240, i, 1, 2, 3), depths, patches))
    buf = b"".join(r[0].tobytes() for r in recs)
    assert len(buf) == 3 * train_ref_ldp.REC
    assert train_ref_ldp.slot_qps(buf) == qps
    luma, lab = train_ref_ldp.parse_records(buf, [2, 0, 1], [37, 22, 32])
    for k, (i, s) in enumerate(((2, 3), (0, 0), (1, 2))):
        assert np.array_equal(luma[k], recs[i][2][s]) and np.array_equal(lab[k], recs[i][1][s])
    with pytest.raises(ValueError):
        train_ref_ldp.parse_records(buf, [0], 30)  # not a slot
    with pytest.raises(ValueError):
        train_ref_ldp.parse_records(buf[:-1], [0], 22)
    # the synthetic records: the extractor's header, slot QPs in order, labels that differ between slots
    syn = np.frombuffer(train_data_ldp.make_records(30, seed=2), np.uint8).reshape(30, -1)
    want = _extractor_record(qps, [np.zeros(16, np.uint8)] * 4, [np.zeros(4096, np.uint8)] * 4, 416, 240, 0, 0, 0, 2)
    assert np.array_equal(syn[0, :64], want[:64])
    assert train_ref_ldp.slot_qps(syn.tobytes()) == qps
    _, l22 = train_ref_ldp.parse_records(syn.tobytes(), np.arange(30), 22)
    _, l37 = train_ref_ldp.parse_records(syn.tobytes(), np.arange(30), 37)
    assert l37.max() <= 1 and l22.max() == 3 and not np.array_equal(l22, l37)


def test_written_index_matches_the_reference_ldp_table(pkg, tmp_path):
    """ethcnn_ckpt_write_blob's .index == the reference's model_LDP_2000000_qp22~37.dat.index (names, dtypes, shapes, offsets)"""
    prefix = str(tmp_path / "model_LDP_2000000_qp22~37.dat")
    pkg.ethcnn.write_ckpt_blob(prefix, np.random.default_rng(3).standard_normal(1288210).astype(np.float32))
    mine = pkg.ethcnn.read_ckpt_index(prefix + ".index")
    ref = pkg.ethcnn.read_ckpt_index(GOLDEN_INDEX)
    assert len(ref) == 36
    assert [e[:6] for e in mine] == [e[:6] for e in ref]  # name, dtype, shape, shard, offset, size


def test_mixed_eval_slots_follow_the_documented_draw(pkg):
    got = pkg.ethcnn.mixed_eval_slots(77, 300)
    want = [(train_ref.draw(77, 2, 0, i, 0) >> 32) * 4 >> 32 for i in range(300)]
    assert list(got) == want and set(got) == {0, 1, 2, 3}


def test_tune_masks_select_one_heads_six_tensors():
    names = [n for n, _, _ in train_ref.ethcnn_np.TENSORS]
    for tune, tag in train_ref_ldp.TUNE_TAGS.items():
        m = train_ref_ldp.tune_mask(tune)
        on = [n for n, shape, off in train_ref.ethcnn_np.TENSORS if m[off // 4]]
        assert sorted(on) == sorted(n for n in names if tag in n) and len(on) == 6
    blob, acc, g = np.ones(1288210), np.full(1288210, 2.0), np.full(1288210, 3.0)
    nb, na = train_ref_ldp.masked_momentum_update(blob, acc, g, 0.1, 2)
    m = train_ref_ldp.tune_mask(2)
    assert (nb[~m] == 1).all() and (na[~m] == 2).all() and np.allclose(na[m], 4.8) and np.allclose(nb[m], 1 - 0.48)
