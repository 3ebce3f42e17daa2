"""TEST INFRASTRUCTURE: seeded synthetic ETH-LSTM training samples in the reference's file format (ETH-LSTM_Training_LDP/
input_data.py:94-108): 37264 bytes = 64 info bytes (byte 0 = 19, i_frame as a little-endian u32 at byte 10) + 20 slots of 465 float32
[qp | 16 depth labels | 448-vector].  The labels are a fixed function of the slot's vector, so a net can learn them."""
import numpy as np

REC, STEPS, SLOT = 37264, 20, 465


def make_samples(n, seed=1, qps=(22, 27, 32, 37)):
    rng = np.random.default_rng(seed)
    vec = (rng.standard_normal((n, STEPS, 448)) * 0.7).astype(np.float32)
    # depth of 16x16 block k from three fixed groups of vector columns: 0..3, every depth and every level occurs
    s64 = vec[:, :, 0:8].sum(2)
    s32 = np.stack([vec[:, :, 64 + 8 * q: 72 + 8 * q].sum(2) for q in range(4)], 2)
    s16 = np.stack([vec[:, :, 192 + 4 * k: 196 + 4 * k].sum(2) for k in range(16)], 2)
    lab = np.zeros((n, STEPS, 16), np.float32)
    for k in range(16):
        q = (k // 8) * 2 + (k % 4) // 2
        d = (s64 > 0).astype(np.float32)
        d = d + d * (s32[:, :, q] > 0)
        d = d + (d == 2) * (s16[:, :, k] > 0)
        lab[:, :, k] = d
    out = np.zeros((n, REC), np.uint8)
    out[:, 0] = 19
    i_frame = rng.integers(19, 600, n).astype("<u4")
    out[:, 10:14] = i_frame.view(np.uint8).reshape(n, 4)
    f = np.zeros((n, STEPS, SLOT), np.float32)
    f[:, :, 0] = rng.choice(np.asarray(qps, np.float32), n)[:, None]
    f[:, :, 1:17] = lab
    f[:, :, 17:] = vec
    out[:, 64:] = f.reshape(n, -1).view(np.uint8)
    return out.tobytes()
