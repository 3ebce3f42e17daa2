"""TEST INFRASTRUCTURE: where the pieces of the host entries end.  Several host entries cut their input into pieces and walk them
with an index (`at`, `done`, `j`): the calibrator's and the simulator's host adds, the comparison of two host arrays, the permuted
read-back of a sample set and the two sample-file writers.  Every offset that depends on the index is multiplied by zero until the
input is larger than one piece, and a piece is 2^20 CTUs or 64 MB.  Each function below restates one loop: the LARGEST input that
still is one piece.  A test that means to reach the second piece sizes its input from these and asserts n > piece first (a condition
on the shape, not a measurement); tests/test_gpu_host_pieces.py holds such a test per loop, tests/test_host_pieces_cpu.py pins the
constants against the source text and checks the fixtures below with the references alone.  csrc = the directory
hevc-complexity-reduction_amd/csrc."""
import functools

import numpy as np

import calib_ref

STAGE_CTUS = 1 << 20   # kStageCtus, csrc/ethcnn_analysis.h:15
IO_BYTES = 64 << 20    # kIoBytes, csrc/ethcnn_samples.cpp:13 and csrc/ethcnn_lstm_samples.cpp:11
REC_AI, REC_INTER, REC_LSTM = 4992, 16516, 37264  # kRec / kRecLdp (csrc/ethcnn_train.h:33,35), kRecBytes (csrc/ethcnn_lstm_train.h:52)


def ctus_per_frame(width, height):
    return ((width + 63) // 64) * ((height + 63) // 64)


def stage_ctus():
    """stage_pieces in the per-CTU layout, CTUs: csrc/ethcnn_analysis.cpp:66-80, the offsets `at * pb` and `labels + at * lb` at
    :74-75; called with piece = kStageCtus by ethcnn_calib_add (csrc/ethcnn_calib.cpp:145 through add_staged, :68-78) and by
    ethcnn_sim_add (csrc/ethcnn_sim.cpp:204 through add_staged, :112-119); the simulator's piece callback Add::pack takes `done * per`
    and `done * subs_per_unit` from it (csrc/ethcnn_sim.cpp:76-77)"""
    return STAGE_CTUS


def stage_frames(width, height):
    """the same loop in the frame layout, frames: piece = max(1, kStageCtus / ctus_per_frame), csrc/ethcnn_calib.cpp:176
    (ethcnn_calib_add_frames) and csrc/ethcnn_sim.cpp:233 (ethcnn_sim_add_frames)"""
    return max(1, STAGE_CTUS // ctus_per_frame(width, height))


def compare_ctus():
    """compare_host, CTUs of either layout: csrc/ethcnn_audit.cpp:141-170; piece = min(n, kStageCtus) at :146 unless both arrays and
    the flags lie in ethcnn_host_alloc buffers (then the whole call is one launch); the offsets `a + at * kNOut`, `(long)at` as the
    kernel's `first` and `flags + at` at :158-164"""
    return STAGE_CTUS


def samples_read_records(record_bytes):
    """the permuted ethcnn_samples_read, records: csrc/ethcnn_samples.cpp:443-455, piece = kIoBytes / record_bytes at :443, the
    offsets `first + j` and `out + j * rb` at :451 and :453.  ethcnn_samples_write (csrc/ethcnn_samples.cpp:466-476) walks the set in
    pieces of the same size and reads each through it"""
    return IO_BYTES // record_bytes


def lstm_write_samples():
    """ethcnn_lstm_samples_write, samples: csrc/ethcnn_lstm_samples.cpp:286-296, piece = kIoBytes / 37264 at :286"""
    return IO_BYTES // REC_LSTM


# ------------------------------------------------------------------------------------------------------------------ fixtures ---
# Built once per process (about 90 MB of probabilities each) and never written to afterwards.
TOL = 1e-4
COMPARE_THR = ((600, 700, 800), (400, 300, 200))  # (up_k, down_k) of the comparison's candidate


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def per_ctu_case():
    """n = kStageCtus + 2 * 256 + 77 CTUs in the per-CTU layout -> dict.  The first piece holds a reject of its own (`reject_first`);
    behind the boundary lie a fully split CTU with -0.0 and 1.0 (`split_at`: valid values, bins 0 and 1024), a CTU with NaN, -0.5 and
    1.5 (`reject_at`) and a labelled CTU beside it (`labelled_at`)"""
    piece = stage_ctus()
    n = piece + 2 * 256 + 77
    rng = np.random.default_rng(2520)
    probs, depth = calib_ref.edge_probs(rng, n), calib_ref.random_depths(rng, n)
    c = dict(piece=piece, n=n, reject_first=4321, split_at=piece + 5, reject_at=piece + 300, labelled_at=piece + 301)
    probs[c["reject_first"], 7] = np.nan
    depth[c["split_at"]] = 3
    probs[c["split_at"], 2], probs[c["split_at"], 9] = -0.0, 1.0
    probs[c["reject_at"], 0], probs[c["reject_at"], 3], probs[c["reject_at"], 20] = np.nan, -0.5, 1.5
    _frozen(probs, depth)
    c.update(probs=probs, depth=depth)
    return c


FRAME_W, FRAME_H = 4944, 3264   # 78 x 51 = 3978 CTUs: four sub-batches a frame, a partial CTU column, label rows of 309 bytes
COMPARE_W, COMPARE_H = 4936, 3256  # multiples of 8 with the same CTU grid: a partial right column and a partial bottom row


@functools.lru_cache(maxsize=None)
def frame_case():
    """frames = kStageCtus // 3978 + 2 = 265 frames of 4944x3264 -> dict; a piece is 263 frames, so two frames travel in the second.
    labels holds one frame more, in front (skip_label_frames = 1).  Every frame has its p64 capped at 500 / 1024 in the last sub-batch
    and its p32 at 600 / 1024 in the second, so the gates of the second candidate of sim_checks.SIM_CANDS close in both pieces; the
    two frames of the second piece have one further cap each (p64 of sub-batch 0 in the first, p32 of sub-batch 2 in the second) that
    frames 0 and 1 do not have: maxima that land on another frame's sub-batches change an outcome.  Rejects: one in the first piece,
    one 300 CTUs behind the boundary (a labelled CTU beside it), one in the last frame; the last frame also holds a fully split CTU
    with a NaN at level 1 and a 1.5 at level 2"""
    w, h = FRAME_W, FRAME_H
    per = ctus_per_frame(w, h)
    piece = stage_frames(w, h)
    frames = STAGE_CTUS // per + 2
    cap = piece * per
    rng = np.random.default_rng(2521)
    probs = calib_ref.edge_probs(rng, frames * per).reshape(frames, per, 21)
    p64, p32 = np.float32(500 / 1024.0), np.float32(600 / 1024.0)
    probs[:, 3072:, 0] = np.minimum(probs[:, 3072:, 0], p64)
    probs[:, 1024:2048, 1:5] = np.minimum(probs[:, 1024:2048, 1:5], p32)
    probs[piece, :1024, 0] = np.minimum(probs[piece, :1024, 0], p64)
    probs[piece + 1, 2048:3072, 1:5] = np.minimum(probs[piece + 1, 2048:3072, 1:5], p32)
    labels = rng.integers(0, 4, size=(1 + frames, h // 16, w // 16)).astype(np.uint8)
    c = dict(width=w, height=h, per=per, piece=piece, frames=frames, cap=cap, n=frames * per, reject_first=5 * per + 50,
             reject_at=cap + 300, labelled_at=cap + 301, reject_last=(frames - 1) * per + 100, split_at=(frames - 1) * per + 205)
    flat = probs.reshape(-1, 21)
    flat[c["reject_first"], 0] = np.nan
    flat[c["reject_at"], 7] = np.nan
    flat[c["reject_last"], 7] = np.nan
    cy, cx = divmod(205, (w + 63) // 64)
    labels[-1, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = 3
    flat[c["split_at"], 3], flat[c["split_at"], 6] = np.nan, 1.5
    _frozen(probs, labels)
    c.update(probs=probs, labels=labels, rejected=4)
    return c


def compare_pair(a, piece):
    """b = a with an eighth of its values redrawn, and each level's largest difference behind the piece boundary: a difference of
    1.0 (the largest two probabilities can have) is taken out wherever the redrawing made one, then planted at CTUs piece + 40 / 41 /
    42 on levels 0 / 1 / 2 -> (a', b, [the three CTUs]); a' is a copy of a with the three planted values"""
    a = np.array(a, np.float32).reshape(-1, 21)
    n = a.shape[0]
    rng = np.random.default_rng(2522)
    b = np.where(rng.integers(0, 8, size=a.shape) == 0, calib_ref.edge_probs(rng, n), a).astype(np.float32)
    with np.errstate(invalid="ignore"):
        b = np.where(np.abs(a - b) >= np.float32(1), a, b)
    planted = [piece + 40, piece + 41, piece + 42]
    for ctu, col in zip(planted, (0, 3, 17)):
        assert np.isfinite(a[ctu]).all() and np.isfinite(b[ctu]).all()
        a[ctu, col], b[ctu, col] = 1.0, 0.0
    _frozen(a, b)
    return a, b, planted


@functools.lru_cache(maxsize=None)
def per_ctu_compare():
    c = per_ctu_case()
    return compare_pair(c["probs"], compare_ctus())


@functools.lru_cache(maxsize=None)
def frame_compare():
    """the probabilities of frame_case() as frames of 4936x3256 (the same 3978 CTUs a frame); 2^20 is no multiple of 3978, so the
    second piece starts inside a frame"""
    c = frame_case()
    assert ctus_per_frame(COMPARE_W, COMPARE_H) == c["per"]
    return compare_pair(c["probs"], compare_ctus())


# ---- sample sets: sizes
GATHER_W, GATHER_H = 1984, 1088  # 31 x 17 = 527 whole CTUs a frame (the geometry of test_permuted_read_past_the_gather_cap)
GATHER_PER = (GATHER_W // 64) * (GATHER_H // 64)


def gather_frames(record_bytes):
    """cut frames of 1984x1088 whose records are more than one read-back piece: 8 (inter) and 26 (All-Intra)"""
    return samples_read_records(record_bytes) // GATHER_PER + 1


LSTM_W, LSTM_H, LSTM_FRAMES = 192, 128, 771  # 6 CTUs a frame; heads at frames 20, 30 .. 770 -> 76 * 6 heads, four slots each
LSTM_TAIL_FRAME = 680  # the records from this frame on lie behind the first 64 MB of the file; the heads at frames 700 .. 770 use only them


def lstm_records():
    """Low-Delay-P records of one 192x128 sequence of 771 frames, frame after frame: uint8 [4626, 16516] (76 MB: also more than one
    upload slice of a build from host records).  Random residuals and labels 0..3 under headers as tests/train_data_ldp.py writes them"""
    per = (LSTM_W // 64) * (LSTM_H // 64)
    n = per * LSTM_FRAMES
    rng = np.random.default_rng(2523)
    rec = rng.integers(0, 256, (n, REC_INTER), dtype=np.uint8)
    rec[:, :64] = 255
    rec[:, 0] = 1
    i = np.arange(n)
    for at, v in ((2, np.full(n, LSTM_W)), (4, np.full(n, LSTM_H)), (14, (i % per) // (LSTM_W // 64)), (16, i % (LSTM_W // 64)), (18, np.full(n, 7))):
        rec[:, at], rec[:, at + 1] = v % 256, v // 256
    rec[:, 10:14] = (i // per).astype("<u4").view(np.uint8).reshape(-1, 4)
    for s, qp in enumerate((22, 27, 32, 37)):
        at = 64 + 4113 * s
        rec[:, at] = qp
        rec[:, at + 1:at + 17] &= 3
    return rec
