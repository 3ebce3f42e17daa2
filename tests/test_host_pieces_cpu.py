"""No GPU: tests/host_pieces.py against the source text it restates, and its fixtures against what tests/test_gpu_host_pieces.py claims
of them, with the numpy references alone: a reject, a labelled CTU and (frame layout) a closing gate on both sides of the piece
boundary, each level's worst difference behind it, and sample sets of more than one read-back piece."""
import os
import re

import numpy as np
import pytest

import audit_ref
import host_pieces as hp
import sim_ref
from sim_checks import SIM_CANDS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hevc-complexity-reduction_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_against_the_source_text():
    assert re.search(r"constexpr int64_t kStageCtus = 1 << 20;", _text("ethcnn_analysis.h")) and hp.STAGE_CTUS == 1 << 20
    for name in ("ethcnn_samples.cpp", "ethcnn_lstm_samples.cpp"):
        assert re.search(r"constexpr size_t kIoBytes = 64u << 20;", _text(name)), name
    assert hp.IO_BYTES == 64 << 20
    train, lstm = _text("ethcnn_train.h"), _text("ethcnn_lstm_train.h")
    assert re.search(r"constexpr int kRec = 4992;", train) and hp.REC_AI == 4992
    assert re.search(r"constexpr int kRecLdp = 16516;", train) and hp.REC_INTER == 16516
    assert re.search(r"constexpr int kRecBytes = 64 \+ 4 \* kSlotFloats \* kSteps;", lstm)
    floats, steps = (int(re.search(r"constexpr int %s = (\d+);" % k, lstm).group(1)) for k in ("kSlotFloats", "kSteps"))
    assert 64 + 4 * floats * steps == hp.REC_LSTM == 37264
    assert re.search(r"constexpr int kRecOut = lstm_train::kRecBytes;", _text("ethcnn_lstm_samples.h"))


def test_pieces_against_the_launchers_text():
    """the expressions the functions restate, where the docstrings say they are"""
    calib, sim, audit = _text("ethcnn_calib.cpp"), _text("ethcnn_sim.cpp"), _text("ethcnn_audit.cpp")
    assert "add_staged(k, probs, depth16, n, kStageCtus, 84, 16, g)" in calib and "add_staged(a, probs, depth16, n, kStageCtus, 84, 16)" in sim
    for text in (calib, sim):
        assert "std::max<int64_t>(1, kStageCtus / per), per * 84, lab" in text
    assert "(a_direct && b_direct && f_direct) ? n : std::min(n, kStageCtus)" in audit
    samples, lstm = _text("ethcnn_samples.cpp"), _text("ethcnn_lstm_samples.cpp")
    assert "std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(kIoBytes / rb)))" in samples and "std::max<int64_t>(1, (int64_t)(kIoBytes / rb))" in samples
    assert "std::max<int64_t>(1, (int64_t)(kIoBytes / kRecOut))" in lstm
    assert hp.stage_ctus() == hp.compare_ctus() == 1 << 20
    assert hp.stage_frames(hp.FRAME_W, hp.FRAME_H) == 263 and hp.stage_frames(65536, 65536) == 1
    assert (hp.samples_read_records(hp.REC_AI), hp.samples_read_records(hp.REC_INTER), hp.lstm_write_samples()) == (13443, 4063, 1800)


def _worst_behind(a, b, planted, piece, width=None, height=None):
    """each level's largest difference is the planted 1.0, and the lowest CTU that has it lies behind the boundary"""
    want = audit_ref.compare(a, b, hp.TOL, None, width, height)
    assert want["max_abs"] == [1.0, 1.0, 1.0] and want["worst_ctu"] == planted and min(planted) >= piece
    first = audit_ref.compare(a[:piece], b[:piece], hp.TOL)
    assert all(0.0 < v < 1.0 for v in first["max_abs"]) and all(0 <= w < piece for w in first["worst_ctu"])
    assert want["rejected_ctus"] > first["rejected_ctus"] > 0  # rejected rows on both sides
    assert all(x > y > 0 for x, y in zip(want["over_tol"], first["over_tol"]))


def test_per_ctu_fixture():
    c = hp.per_ctu_case()
    piece, n = c["piece"], c["n"]
    assert n == (1 << 20) + 589 and n > piece and n % 256 != 0
    s = sim_ref.Set()
    s.add(c["probs"], c["depth"])
    rejected = np.flatnonzero(~s.inside[:, 0])
    assert rejected.tolist() == [c["reject_first"], c["reject_at"]] and c["reject_first"] < piece < c["reject_at"]
    assert s.labelled[c["labelled_at"]] and s.labelled[:piece].any() and s.truth[c["split_at"]].all()
    assert s.bins[c["split_at"], 2] == 0 and s.bins[c["split_at"], 9] == 1024 and np.signbit(c["probs"][c["split_at"], 2])
    assert piece - 500 <= piece < c["reject_at"] < piece + 500  # inside the window of sim_checks
    a, b, planted = hp.per_ctu_compare()
    assert np.array_equal(np.delete(a, planted, axis=0).view(np.uint32), np.delete(c["probs"], planted, axis=0).view(np.uint32))
    _worst_behind(a, b, planted, piece)


def test_frame_fixture():
    c = hp.frame_case()
    per, piece, frames, cap = c["per"], c["piece"], c["frames"], c["cap"]
    assert (per, piece, frames) == (3978, 263, 265) and frames * per > hp.STAGE_CTUS >= cap and frames - piece == 2
    assert (per + 1023) // 1024 == 4 and c["width"] % 64 != 0 and (c["width"] // 16) % 4 != 0 and c["labels"].shape[0] == frames + 1
    s = sim_ref.Set()
    s.add_frames(c["probs"], c["labels"], c["width"], c["height"], skip_label_frames=1)
    assert s.info()["sub_batches"] == 4 * frames and s.info()["rejected_ctus"] == c["rejected"]
    rejected = np.flatnonzero(~(s.inside[:, 0] | s.edge[:, 0]))
    assert rejected.tolist() == [c["reject_first"], c["reject_at"], c["reject_last"], c["split_at"]]
    assert c["reject_first"] < cap < c["reject_at"] < cap + 500 and c["reject_last"] >= (frames - 1) * per
    assert s.labelled[c["labelled_at"]] and s.labelled[:cap].any()
    lab = c["labels"][1:].reshape(frames, -1, c["width"] // 16)
    cy, cx = divmod(c["split_at"] % per, 78)
    assert (lab[-1, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] == 3).all() and cx < c["width"] // 64
    # the gates of the second candidate (AI order: M1 <= 500 closes gate 1, M2 <= 600 gate 2) close in every frame, so in both pieces
    m1, m2 = np.array(s.m1).reshape(frames, 4), np.array(s.m2).reshape(frames, 4)
    g1, g2 = int(SIM_CANDS[1]["down_k"][0]), int(SIM_CANDS[1]["down_k"][1])
    assert (m1[:, 3] <= g1).all() and (m2[:, 1] <= g2).all()
    # and the second piece's frames have a closed gate where the frames 0 and 1 (whose sub-batches a lost offset would hit) have it open
    assert m1[piece, 0] <= g1 < m1[0, 0] and m2[piece + 1, 2] <= g2 < m2[1, 2]
    assert (m1[:piece, :3] > g1).all() and (m2[:piece, [0, 2, 3]] > g2).all()
    assert not sim_ref.equal(s.evaluate(SIM_CANDS[1:], sim_ref.GATES_AI), s.evaluate(SIM_CANDS[1:], sim_ref.GATES_NONE))
    a, b, planted = hp.frame_compare()
    _worst_behind(a, b, planted, hp.compare_ctus(), hp.COMPARE_W, hp.COMPARE_H)
    assert hp.compare_ctus() % per == 2362 and hp.compare_ctus() // per == piece  # the second piece starts inside frame 263


def test_sample_set_sizes(pkg):
    for rb, frames, count in ((hp.REC_INTER, 8, 4216), (hp.REC_AI, 26, 13702)):
        assert hp.gather_frames(rb) == frames and frames * hp.GATHER_PER == count > hp.samples_read_records(rb)
        assert count * rb > hp.IO_BYTES and (frames - 1) * hp.GATHER_PER <= hp.samples_read_records(rb)  # the smallest such set
    rec = hp.lstm_records()
    heads, strides, skipped = pkg.ethcnn.lstm_samples_plan(rec)
    assert len(rec) == 4626 and rec.nbytes > hp.IO_BYTES
    assert 4 * len(heads) == 1824 > hp.lstm_write_samples() and skipped == 0 and 4 * (len(heads) - 6) <= hp.lstm_write_samples()
    cut = hp.LSTM_TAIL_FRAME * 6  # the tail that test_lstm_sample_file_across_pieces builds on its own: wholly behind the first upload slice
    tail_heads, tail_strides, tail_skipped = pkg.ethcnn.lstm_samples_plan(rec[cut:])
    assert cut * hp.REC_INTER > hp.IO_BYTES and len(tail_heads) == 48 and tail_skipped == 12  # (the heads at frames 680 and 690 reach in front of it)
    assert np.array_equal(tail_heads + cut, heads[-48:]) and np.array_equal(tail_strides, strides[-48:])
