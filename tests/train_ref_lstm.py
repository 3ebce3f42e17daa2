"""TEST INFRASTRUCTURE: a float64 torch-CPU restatement of the reference's ETH-LSTM training graph,
ETH-LSTM_Training_LDP/net_CTU64.py:85-276 (cells and heads :85-140, features and labels :142-216, balanced loss :220-233,
clip + momentum :256-259, accuracy :263-271), its sample parser (input_data.py:88-122) and the trainer's documented RNG streams.
The gradient oracle of the GPU LSTM trainer.  Nothing here is imported by the product.

As shipped: the cells consume slot 19 first (cell_inputs.reverse(), :109) and the predictions are reversed back (:137), but
qp_list / i_frame_in_GOP_one_hot_list are indexed by the unrolled step (:125), so the prediction of slot p sees the features of
slot 19 - p.  Rows of every [20 n, .] output: 20 b + p.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import ethcnn_lstm_np  # noqa: E402
import train_ref  # noqa: E402
from train_ref import draw  # noqa: E402

REC, STEPS, SLOT = 37264, 20, 465
CELLS = (("64", 64, 48, 1, 0), ("32", 128, 96, 4, 64), ("16", 256, 192, 16, 192))  # tag, hidden, fc2, fc3, vector column
FLOATS = ethcnn_lstm_np.LSTM_BLOB_FLOATS
OFFS = {n: (o // 4, int(np.prod(s))) for n, s, o in ethcnn_lstm_np.LSTM_TENSORS}


def views(flat):
    return {n: flat[o // 4: o // 4 + int(np.prod(s))].view(*s) for n, s, o in ethcnn_lstm_np.LSTM_TENSORS}


def parse_samples(buf, idx):
    """-> vectors [n,20,448] float32, labels [n,20,16], qps [n,20], i_frame_in_GOP [n,20] (input_data.py:94-120)"""
    raw = np.frombuffer(buf, dtype=np.uint8)
    if raw.size % REC:
        raise ValueError("sample buffer is not a whole number of %d-byte samples" % REC)
    rec = raw.reshape(-1, REC)[np.asarray(idx)]
    f = np.ascontiguousarray(rec[:, 64:]).view(np.float32).reshape(len(rec), STEPS, SLOT)
    info = rec[:, :64].astype(np.int64)
    i_frame = info[:, 10] + 256 * info[:, 11] + 65536 * info[:, 12] + 16777216 * info[:, 13]
    frames = i_frame[:, None] - np.arange(STEPS)[None, :]      # get_delta_ref_frames with i_frame >= 19
    return f[:, :, 17:].copy(), f[:, :, 1:17].copy(), f[:, :, 0].copy(), np.mod(frames, 4)


def _cell_clip(c):
    """LSTMCell(cell_clip = 5): clip_by_value, no gradient where c was clipped.  A NaN cell becomes -5 and gets no gradient (DESIGN
    section 9: fminf(fmaxf(NaN, -5), 5) = -5; torch.clamp alone would return the NaN)"""
    return torch.where(torch.isnan(c), torch.full_like(c, -5.0), torch.clamp(c, -5.0, 5.0))


def _carry(cpre, c):
    """the cell state the next unrolled step sees: the clipped one"""
    return c


def _forget(fg, c_prev, cpre_prev):
    """f * c_prev (cpre_prev, the state before its clip, is there for a wrong restatement to use)"""
    return fg * c_prev


def net(flat, vec, labels, qps, gop, qp_scale=1.0, mask_h=None, mask_fc2=None):
    """net_CTU64.net with isdrop = (masks given; [20 n, 448] and [20 n, 336], rows 20 b + p).  dict(probs [20 n,21], C, H [20 n,448]
    (c after the clip, h not dropped, computed with slot p as the input), Cpre (c before the clip), X3 [20 n, 53+101+197] (the rows FC3
    multiplies: [fc2 after dropout, qp, one-hot] per cell), G [20 n, 4, 448] (the gate values i, j, f, o), loss_list, accuracy_list,
    total_loss).  _cell_clip, _carry, _forget and train_ref._lrelu are looked up when called: tests/train_edges.py patches them to make
    deliberately wrong restatements."""
    tv = views(flat)
    n, dt = vec.shape[0], flat.dtype   # float64; float32 only to measure what fp32 arithmetic costs (the GPU tests' bounds)
    x = torch.as_tensor(np.asarray(vec, dtype=np.float64)).to(dt)
    qp = (torch.as_tensor(np.asarray(qps, dtype=np.float64)) / 51.0 * qp_scale).to(dt)  # :149 (qp_scale 1: as shipped)
    onehot = F.one_hot(torch.as_tensor(np.asarray(gop, dtype=np.int64)), 4).to(dt)       # :147
    mh = None if mask_h is None else torch.as_tensor(np.asarray(mask_h, dtype=np.float64)).reshape(n, STEPS, 448).to(dt)
    m2 = None if mask_fc2 is None else torch.as_tensor(np.asarray(mask_fc2, dtype=np.float64)).reshape(n, STEPS, 336).to(dt)
    P = [[None] * 3 for _ in range(STEPS)]
    Cs = [[None] * 3 for _ in range(STEPS)]
    Hs = [[None] * 3 for _ in range(STEPS)]
    Ps = [[None] * 3 for _ in range(STEPS)]
    X3 = [[None] * 3 for _ in range(STEPS)]
    Gs = [[None] * 3 for _ in range(STEPS)]
    o2 = 0
    for ci, (tag, hid, n2, n3, col) in enumerate(CELLS):
        pre = "RNN%s/" % tag
        K, bK = tv[pre + "multi_rnn_cell/cell_0/lstm_cell/kernel"], tv[pre + "multi_rnn_cell/cell_0/lstm_cell/bias"]
        W2, b2, W3, b3 = tv[pre + "fc2/full_connect_w"], tv[pre + "fc2/full_connect_b"], tv[pre + "fc3/full_connect_w"], tv[pre + "fc3/full_connect_b"]
        c = torch.zeros(n, hid, dtype=dt)
        h = torch.zeros(n, hid, dtype=dt)
        cpre = torch.zeros(n, hid, dtype=dt)
        for ts in range(STEPS):
            p = STEPS - 1 - ts                                                           # cell_inputs.reverse()
            z = torch.cat([x[:, p, col:col + hid], h], 1) @ K + bK
            i, j, f, o = torch.split(z, hid, dim=1)
            ig, jg, fg, og = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)
            cpre = _forget(fg, c, cpre) + ig * jg
            cc = _cell_clip(cpre)
            h = og * torch.tanh(cc)
            Gs[p][ci] = torch.stack([ig, jg, fg, og], 1).detach()
            c = _carry(cpre, cc)
            efs = torch.cat([qp[:, ts:ts + 1], onehot[:, ts]], 1)                        # :125: indexed by the unrolled step
            out = h if mh is None else h / 0.5 * mh[:, p, col:col + hid]                 # DropoutWrapper on the OUTPUT only
            h2 = train_ref._lrelu(torch.cat([out, efs], 1) @ W2 + b2)                    # leaky_relu, alpha 0.2
            if m2 is not None:
                h2 = h2 / 0.8 * m2[:, p, o2:o2 + n2]
            X3[p][ci] = torch.cat([h2, efs], 1)
            P[p][ci] = torch.sigmoid(X3[p][ci] @ W3 + b3)
            Cs[p][ci], Hs[p][ci], Ps[p][ci] = cc, h, cpre
        o2 += n2
    probs = torch.stack([torch.cat(P[p], 1) for p in range(STEPS)], 1).reshape(n * STEPS, 21)
    C = torch.stack([torch.cat(Cs[p], 1) for p in range(STEPS)], 1).reshape(n * STEPS, 448)
    H = torch.stack([torch.cat(Hs[p], 1) for p in range(STEPS)], 1).reshape(n * STEPS, 448)
    Cpre = torch.stack([torch.cat(Ps[p], 1) for p in range(STEPS)], 1).reshape(n * STEPS, 448)
    lab = np.asarray(labels, dtype=np.float64).reshape(n * STEPS, 16)
    l3 = loss_list(probs, lab.astype(np.float64 if dt == torch.float64 else np.float32))
    x3 = torch.stack([torch.cat(X3[p], 1) for p in range(STEPS)], 1).reshape(n * STEPS, -1)
    gates = torch.stack([torch.cat(Gs[p], 2) for p in range(STEPS)], 1).reshape(n * STEPS, 4, 448)
    return {"probs": probs, "C": C, "H": H, "Cpre": Cpre, "X3": x3, "G": gates, "loss_list": l3,
            "accuracy_list": torch.as_tensor(train_ref.accuracy(probs.detach().numpy(), lab)), "total_loss": l3[2] + l3[1] + l3[0]}


def loss_list(probs, lab):
    """:160-176 labels per row and :220-233 (is_balance = True; counts over all rows at once) -> [loss_64, loss_32, loss_16]"""
    m = lab.shape[0]
    y = torch.as_tensor(lab).reshape(m, 4, 4, 1)
    l64, l32, l16 = train_ref.balanced_loss(train_ref.split_labels(y), probs[:, :1], probs[:, 1:5], probs[:, 5:])
    return torch.stack([l64, l32, l16])


def loss_and_grad(blob, vec, labels, qps, gop, qp_scale=1.0, mask_h=None, mask_fc2=None, dtype=torch.float64):
    """-> (out dict with numpy values, unclipped gradient [FLOATS] in blob layout, its global norm)"""
    flat = torch.tensor(np.asarray(blob, dtype=np.float64), dtype=dtype, requires_grad=True)
    out = net(flat, vec, labels, qps, gop, qp_scale, mask_h, mask_fc2)
    out["total_loss"].backward()
    g = flat.grad.numpy().astype(np.float64)
    return {k: v.detach().numpy() for k, v in out.items()}, g, float(np.sqrt(np.sum(g * g)))


def clip_by_global_norm(g, clip=5.0):
    """tf.clip_by_global_norm: g * clip * min(1 / norm, 1 / clip)"""
    norm = np.sqrt(np.sum(g * g))
    return g * (clip * min(1.0 / norm, 1.0 / clip)) if clip > 0 else g


def lr_at(step, lr_init=0.1, decay_rate=0.3163, decay_steps=25000):
    return lr_init * decay_rate ** (step // decay_steps)


def train_step(blob, accum, grad, lr, clip=5.0, momentum=0.9):
    """clip, then MomentumOptimizer (accum = accum * momentum + g; var -= lr * accum)"""
    return train_ref.momentum_update(blob, accum, clip_by_global_norm(grad, clip), lr, momentum)


# ---- the trainer's documented RNG streams (include/ethcnn.h "ETH-LSTM training")
def batch_of(seed, step, batch, nrec):
    return np.array([(draw(seed, 4, step, b, 0) >> 32) * nrec >> 32 for b in range(batch)], np.int64)


def dropout_masks(seed, step, rows):
    k1, k2 = np.float32(0.5), np.float32(0.8)
    mh = np.array([[1.0 if np.float32((draw(seed, 5, step, r, u) >> 40) * 2.0 ** -24) < k1 else 0.0 for u in range(448)] for r in range(rows)])
    m2 = np.array([[1.0 if np.float32((draw(seed, 5, step, r, 448 + v) >> 40) * 2.0 ** -24) < k2 else 0.0 for v in range(336)] for r in range(rows)])
    return mh, m2


def init_weights(seed, names=None):
    """glorot_uniform of every fc tensor and LSTM kernel (1-D [n]: limit sqrt(3 / n)), zero LSTM biases, from stream 6
    (names: only those tensors, the others stay zero: the pure-Python draw takes seconds per million)"""
    blob = np.zeros(FLOATS, np.float32)
    for t, (name, shape, off) in enumerate(ethcnn_lstm_np.LSTM_TENSORS):
        if names is not None and name not in names:
            continue
        n = int(np.prod(shape))
        limit = np.sqrt(6.0 / (shape[0] + shape[1])) if len(shape) == 2 else (np.sqrt(3.0 / shape[0]) if "full_connect_b" in name else 0.0)
        u = np.array([(draw(seed, 6, t, 0, k) >> 11) for k in range(n)], dtype=np.float64) * 2.0 ** -53
        blob[off // 4: off // 4 + n] = ((2.0 * u - 1.0) * limit).astype(np.float32)
    return blob
