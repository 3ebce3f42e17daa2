"""TEST INFRASTRUCTURE: a float64 torch-CPU restatement of the reference's training graph,
ETH-CNN_Training_AI/net_CTU64.py:94-206, plus its MomentumOptimizer update
(net_CTU64.py:192-196, train_CNN_CTU64.py:36-47).  The gradient oracle of the GPU trainer.

Parameters are views into one float64 leaf in blob layout (the TF-V2 .data payload, keys sorted), so
`grad` comes back in the layout of ethcnn_train_debug_fetch(GRADS).  Nothing here is imported by the product.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import ethcnn_np  # noqa: E402  (TENSORS: the checkpoint table)

REC = 4992                  # input_data.py:16
BRANCH_BASE = {"L": 0, "M": 6, "S": 12}   # conv Variables in creation order L, M, S (net_CTU64.py:122-138)
HEADS = (("64", 64, 48, 1), ("32", 128, 96, 4), ("16", 256, 192, 16))
INV255 = float(np.float32(1.0 / 255.0))   # tf.scalar_mul(1.0 / 255.0, x) with a float32 scalar (:96)
INV51 = float(np.float32(1.0 / 51.0))     # :97


def _var(i):
    return "Variable" if i == 0 else "Variable_%d" % i


def views(flat):
    out = {}
    for name, shape, off in ethcnn_np.TENSORS:
        n = int(np.prod(shape))
        out[name] = flat[off // 4: off // 4 + n].view(*shape)
    return out


def parse_records(buf, idx, qps):
    """records -> (luma [n,4096] uint8, labels [n,16] depths).  Label row of QP q at byte 4160 + 16 q (input_data.py:104)."""
    raw = np.frombuffer(buf, dtype=np.uint8)
    if raw.size % REC:
        raise ValueError("sample buffer is not a whole number of %d-byte records" % REC)
    rec = raw.reshape(-1, REC)[np.asarray(idx)]
    qps = np.broadcast_to(np.asarray(qps), (len(rec),))
    lab = np.stack([r[4160 + 16 * q: 4160 + 16 * (q + 1)] for r, q in zip(rec, qps)]) if len(rec) else np.zeros((0, 16), np.uint8)
    return rec[:, :4096].copy(), lab


def _lrelu(x):
    return F.leaky_relu(x, 0.2)                       # tf.nn.leaky_relu (alpha 0.2), activate() mode 5


def _conv(x, w, b, k):
    """non_overlap_conv (:84-90): NHWC x HWIO, VALID, stride k, + bias, leaky-ReLU"""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=k).permute(0, 2, 3, 1)
    return _lrelu(y + b)


def _avgpool(x, k):
    n, h, w, c = x.shape
    return x.reshape(n, h // k, k, w // k, k, c).mean(dim=(2, 4))


def split_labels(y):
    """labels (:99-111), literally: depths y [n,4,4,1] -> (y64 [n,1], y32 [n,4], y16 [n,16], v32 [n,4], v16 [n,16])"""
    n, relu = y.shape[0], torch.relu
    y16 = relu(y - 2)
    y32 = relu(_avgpool(y, 2) - 1) - relu(_avgpool(y, 2) - 2)
    y64 = relu(_avgpool(y, 4) - 0) - relu(_avgpool(y, 4) - 1)
    v32 = relu(_avgpool(y, 2) - 0) - relu(_avgpool(y, 2) - 1)
    v16 = relu(y - 1) - relu(y - 2)
    return y64.reshape(n, 1), y32.reshape(n, 4), y16.reshape(n, 16), v32.reshape(n, 4), v16.reshape(n, 16)


def _cnz(t):
    return float((t != 0).sum())


def _counts64(y64):
    """count_nonzero of the level-64 positives and negatives (:178-180: no validity mask at this level)"""
    return _cnz(y64), _cnz(1 - y64)


def _denom(count):
    return count + 1e-12


def balanced_loss(labs, p64, p32, p16):
    """loss (:178-190), is_balance = True, counts over the whole batch -> (l64, l32, l16).  Shared by the three restatements
    (All-Intra, Low-Delay-P, ETH-LSTM: the same lines in each net_CTU64.py); split_labels, _counts64 and _denom are looked up when
    called, so tests/train_edges.py can patch one of them to make a deliberately wrong restatement.  One function for three
    references means one error would be in all three at once: its independent guard is the plain-numpy loop of
    tests/test_train_lstm_cpu.py::test_loss_against_plain_numpy (fractional labels included), which shares no code with it."""
    y64, y32, y16, v32, v16 = labs
    eps = 1e-12
    c64p, c64n = _counts64(y64)
    l64 = (torch.sum(-(y64 * torch.log(p64 + eps))) / _denom(c64p) +
           torch.sum(-((1 - y64) * torch.log((1 - p64) + eps))) / _denom(c64n)) / 2
    l32 = (torch.sum(-(y32 * torch.log(p32 + eps)) * v32) / _denom(_cnz(y32 * v32)) +
           torch.sum(-((1 - y32) * torch.log((1 - p32) + eps)) * v32) / _denom(_cnz((1 - y32) * v32))) / 2
    l16 = (torch.sum(-(y16 * torch.log(p16 + eps)) * v16) / _denom(_cnz(y16 * v16)) +
           torch.sum(-((1 - y16) * torch.log((1 - p16) + eps)) * v16) / _denom(_cnz((1 - y16) * v16))) / 2
    return l64, l32, l16


def net(flat, luma, labels, qp, mask1=None, mask2=None, dtype=torch.float64):
    """net_CTU64.net with isdrop = (masks given): returns dict(probs [n,21], H1 [n,448] (leaky-ReLU FC1, before dropout), X3 [n,49+97+193]
    (the rows FC3 multiplies: [h_fc2 after dropout, qp] per head), loss_list,
    accuracy_list, total_loss).  dtype (that of `flat`): float64; float32 only to measure what fp32 arithmetic costs."""
    tv = views(flat)
    n = luma.shape[0]
    x = torch.as_tensor(np.asarray(luma), dtype=dtype).reshape(n, 64, 64, 1) * INV255
    q = torch.as_tensor(np.broadcast_to(np.asarray(qp, dtype=np.float64), (n,)).copy()).to(dtype).reshape(n, 1) * INV51
    y = torch.as_tensor(np.asarray(labels, dtype=np.float64)).to(dtype).reshape(n, 4, 4, 1)
    labs = split_labels(y)
    y64, y32, y16, v32, v16 = labs
    # trunk (:117-156)
    f2, f3 = {}, {}
    for br, pool in (("L", 4), ("M", 2), ("S", 1)):
        xb = _avgpool(x, pool) if pool > 1 else x
        side = 64 // pool
        nb = side // 16
        m = xb.reshape(n, nb, 16, nb, 16).mean(dim=(2, 4), keepdim=True)   # zero_mean_norm_local(., side, 16)
        xb = (xb.reshape(n, nb, 16, nb, 16) - m).reshape(n, side, side, 1)
        bb = BRANCH_BASE[br]
        c1 = _conv(xb, tv[_var(bb)], tv[_var(bb + 1)], 4)
        c2 = _conv(c1, tv[_var(bb + 2)], tv[_var(bb + 3)], 2)
        c3 = _conv(c2, tv[_var(bb + 4)], tv[_var(bb + 5)], 2)
        f2[br], f3[br] = c2.reshape(n, -1), c3.reshape(n, -1)
    feat = torch.cat([f3["S"], f3["M"], f3["L"], f2["S"], f2["M"], f2["L"]], dim=1)
    # heads (:160-176); dropout = x / keep * mask (tf.nn.dropout) after FC1 (keep 0.5) and FC2 (keep 0.8)
    probs, h1s, x3s, o1, o2 = [], [], [], 0, 0
    for tag, n1, n2, n3 in HEADS:
        h1 = _lrelu(feat @ tv["h_fc1__%s__w" % tag] + tv["h_fc1__%s__b" % tag])
        h1s.append(h1)
        if mask1 is not None:
            h1 = h1 / 0.5 * torch.as_tensor(mask1[:, o1:o1 + n1], dtype=dtype)
        h2 = _lrelu(torch.cat([h1, q], 1) @ tv["h_fc2__%s__w" % tag] + tv["h_fc2__%s__b" % tag])
        if mask2 is not None:
            h2 = h2 / 0.8 * torch.as_tensor(mask2[:, o2:o2 + n2], dtype=dtype)
        x3s.append(torch.cat([h2, q], 1))
        z = x3s[-1] @ tv["y_conv_flat__%s__w" % tag] + tv["y_conv_flat__%s__b" % tag]
        probs.append(torch.sigmoid(z))
        o1, o2 = o1 + n1, o2 + n2
    p64, p32, p16 = probs
    eps = 1e-12
    l64, l32, l16 = balanced_loss(labs, p64, p32, p16)   # loss (:178-190)
    total = l16 + l32 + l64
    # accuracy (:198-206)
    with torch.no_grad():
        c32 = v32 * (torch.round(p32) == torch.round(y32)).double()
        c16 = v16 * (torch.round(p16) == torch.round(y16)).double()
        a16 = torch.sum(v16 * c16) / (torch.sum(v16) + eps)
        a32 = torch.sum(v32 * c32) / (torch.sum(v32) + eps)
        a64 = torch.mean((torch.round(p64) == torch.round(y64)).double())
    return {"probs": torch.cat([p64, p32, p16], 1), "H1": torch.cat(h1s, 1), "X3": torch.cat(x3s, 1), "loss_list": torch.stack([l64, l32, l16]),
            "accuracy_list": torch.stack([a64, a32, a16]), "total_loss": total}


def accuracy(probs, labels):
    """accuracy_list (:198-206) of given probabilities [n,21] and label depths [n,16], float64"""
    p = torch.as_tensor(np.asarray(probs, dtype=np.float64))
    n = p.shape[0]
    y = torch.as_tensor(np.asarray(labels, dtype=np.float64)).reshape(n, 4, 4, 1)
    relu, eps = torch.relu, 1e-12
    y16 = relu(y - 2).reshape(n, 16)
    y32 = (relu(_avgpool(y, 2) - 1) - relu(_avgpool(y, 2) - 2)).reshape(n, 4)
    y64 = (relu(_avgpool(y, 4) - 0) - relu(_avgpool(y, 4) - 1)).reshape(n, 1)
    v32 = (relu(_avgpool(y, 2) - 0) - relu(_avgpool(y, 2) - 1)).reshape(n, 4)
    v16 = (relu(y - 1) - relu(y - 2)).reshape(n, 16)
    c32 = v32 * (torch.round(p[:, 1:5]) == torch.round(y32)).double()
    c16 = v16 * (torch.round(p[:, 5:]) == torch.round(y16)).double()
    return np.array([torch.mean((torch.round(p[:, :1]) == torch.round(y64)).double()).item(),
                     (torch.sum(v32 * c32) / (torch.sum(v32) + eps)).item(), (torch.sum(v16 * c16) / (torch.sum(v16) + eps)).item()])


def loss_and_grad(blob, luma, labels, qp, mask1=None, mask2=None, dtype=torch.float64):
    """-> (out dict with numpy values, gradient [BLOB_FLOATS] in blob layout, as float64 numbers)"""
    flat = torch.tensor(np.asarray(blob, dtype=np.float64), dtype=dtype, requires_grad=True)
    out = net(flat, luma, labels, qp, mask1, mask2, dtype)
    out["total_loss"].backward()
    res = {k: v.detach().numpy() for k, v in out.items()}
    return res, flat.grad.numpy().astype(np.float64)


def lr_at(step, lr_init=0.01, decay_rate=0.3163, decay_steps=250000):
    """tf.train.exponential_decay(staircase=True) at global_step = step"""
    return lr_init * decay_rate ** (step // decay_steps)


def momentum_update(blob, accum, grad, lr, momentum=0.9):
    """MomentumOptimizer, use_nesterov=False: accum = accum * momentum + grad; var -= lr * accum"""
    accum = accum * momentum + grad
    return blob - lr * accum, accum


# ---- the trainer's documented counter RNG (include/ethcnn.h), regenerated here
_M = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def draw(seed, stream, step, slot, unit):
    return mix64(mix64(mix64(seed ^ ((stream * 0xD1B54A32D192ED03) & _M)) ^ step) ^ ((slot << 12) | unit))


def batch_of(seed, step, batch, nrec, qps):
    idx = [(draw(seed, 1, step, b, 0) >> 32) * nrec >> 32 for b in range(batch)]
    qp = [qps[(draw(seed, 2, step, b, 0) >> 32) * len(qps) >> 32] for b in range(batch)]
    return np.array(idx, np.int64), np.array(qp, np.int64)


def dropout_masks(seed, step, batch):
    k1, k2 = np.float32(0.5), np.float32(0.8)
    m1 = np.array([[1.0 if np.float32((draw(seed, 3, step, b, u) >> 40) * 2.0 ** -24) < k1 else 0.0 for u in range(448)]
                   for b in range(batch)])
    m2 = np.array([[1.0 if np.float32((draw(seed, 3, step, b, 448 + v) >> 40) * 2.0 ** -24) < k2 else 0.0 for v in range(336)]
                   for b in range(batch)])
    return m1, m2
