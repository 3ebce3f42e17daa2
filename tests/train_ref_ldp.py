"""TEST INFRASTRUCTURE: a float64 torch-CPU restatement of the reference's Low-Delay-P residual training graph,
ETH-CNN_Training_LDP/net_CTU64.py:94-209, and its MomentumOptimizer update restricted to PARTLY_TUNING_MODE's variables.
The gradient oracle of the GPU trainer's LDP variant.  The trunk, heads, labels and loss are those of tests/train_ref.py (whose
helpers it uses); what differs is the input scaling, x = (x - 128) / 255 * 10 and qp = qp / 51 * 0.18 (:102-103), the 16516-byte
record (input_data.py:48-50) and the tuning masks (:200-209).  Nothing here is imported by the product.
"""
import numpy as np
import torch

import train_ref
from train_ref import _avgpool, _conv, _lrelu, _var, views

REC = 16516
SLOT_BASE, SLOT_BYTES = 64, 4113
TUNE_TAGS = {1: "__64__", 2: "__32__", 3: "__16__"}


def parse_records(buf, idx, qps):
    """records -> (residual luma [n,4096] uint8, labels [n,16] depths): the slot of each sample is the one whose QP byte
    (at 64 + 4113 s) equals the sample's QP (input_data.py:119-130 picks a slot; the QP fed to the net is that slot's byte)."""
    raw = np.frombuffer(buf, dtype=np.uint8)
    if raw.size % REC:
        raise ValueError("sample buffer is not a whole number of %d-byte records" % REC)
    rec = raw.reshape(-1, REC)[np.asarray(idx)]
    qps = np.broadcast_to(np.asarray(qps), (len(rec),))
    luma, lab = np.zeros((len(rec), 4096), np.uint8), np.zeros((len(rec), 16), np.uint8)
    for i, (r, q) in enumerate(zip(rec, qps)):
        slots = [s for s in range(4) if r[SLOT_BASE + SLOT_BYTES * s] == q]
        if len(slots) != 1:
            raise ValueError("record %d: QP %d is not exactly one slot's QP" % (i, q))
        o = SLOT_BASE + SLOT_BYTES * slots[0]
        lab[i], luma[i] = r[o + 1: o + 17], r[o + 17: o + 17 + 4096]
    return luma, lab


def slot_qps(buf):
    """the four slot QPs of record 0"""
    r = np.frombuffer(buf, dtype=np.uint8)[:REC]
    return [int(r[SLOT_BASE + SLOT_BYTES * s]) for s in range(4)]


def net(flat, luma, labels, qp, mask1=None, mask2=None, dtype=torch.float64):
    """LDP net_CTU64.net with isdrop = (masks given): dict(probs [n,21], H1 [n,448] (leaky-ReLU FC1, before dropout), X3 (the rows FC3 multiplies, as in train_ref.net), loss_list,
    accuracy_list, total_loss).  dtype (that of `flat`): float64; float32 only to measure what fp32 arithmetic costs."""
    tv = views(flat)
    n = luma.shape[0]
    x = (torch.as_tensor(np.asarray(luma), dtype=dtype).reshape(n, 64, 64, 1) - 128) / 255.0 * 10   # :102
    q = torch.as_tensor(np.broadcast_to(np.asarray(qp, dtype=np.float64), (n,)).copy()).to(dtype).reshape(n, 1) / 51.0 * 0.18  # :103
    y = torch.as_tensor(np.asarray(labels, dtype=np.float64)).to(dtype).reshape(n, 4, 4, 1)
    labs = train_ref.split_labels(y)
    f2, f3 = {}, {}
    for br, pool in (("L", 4), ("M", 2), ("S", 1)):
        xb = _avgpool(x, pool) if pool > 1 else x
        side = 64 // pool
        nb = side // 16
        m = xb.reshape(n, nb, 16, nb, 16).mean(dim=(2, 4), keepdim=True)
        xb = (xb.reshape(n, nb, 16, nb, 16) - m).reshape(n, side, side, 1)
        bb = train_ref.BRANCH_BASE[br]
        c1 = _conv(xb, tv[_var(bb)], tv[_var(bb + 1)], 4)
        c2 = _conv(c1, tv[_var(bb + 2)], tv[_var(bb + 3)], 2)
        c3 = _conv(c2, tv[_var(bb + 4)], tv[_var(bb + 5)], 2)
        f2[br], f3[br] = c2.reshape(n, -1), c3.reshape(n, -1)
    feat = torch.cat([f3["S"], f3["M"], f3["L"], f2["S"], f2["M"], f2["L"]], dim=1)
    probs, h1s, x3s, o1, o2 = [], [], [], 0, 0
    for tag, n1, n2, n3 in train_ref.HEADS:
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
    l64, l32, l16 = train_ref.balanced_loss(labs, p64, p32, p16)
    with torch.no_grad():
        pr = torch.cat([p64, p32, p16], 1)
        acc = torch.as_tensor(train_ref.accuracy(pr.numpy(), labels))
    return {"probs": torch.cat([p64, p32, p16], 1), "H1": torch.cat(h1s, 1), "X3": torch.cat(x3s, 1),
            "loss_list": torch.stack([l64, l32, l16]), "accuracy_list": acc, "total_loss": l16 + l32 + l64}


def loss_and_grad(blob, luma, labels, qp, mask1=None, mask2=None, dtype=torch.float64):
    """-> (out dict with numpy values, gradient [BLOB_FLOATS] in blob layout, as float64 numbers)"""
    flat = torch.tensor(np.asarray(blob, dtype=np.float64), dtype=dtype, requires_grad=True)
    out = net(flat, luma, labels, qp, mask1, mask2, dtype)
    out["total_loss"].backward()
    return {k: v.detach().numpy() for k, v in out.items()}, flat.grad.numpy().astype(np.float64)


def tune_mask(tune):
    """bool [BLOB_FLOATS]: the parameters PARTLY_TUNING_MODE `tune` optimises (net_CTU64.py:200-209)"""
    m = np.zeros(train_ref.ethcnn_np.TENSORS[-1][2] // 4 + int(np.prod(train_ref.ethcnn_np.TENSORS[-1][1])), bool)
    for name, shape, off in train_ref.ethcnn_np.TENSORS:
        if tune == 0 or TUNE_TAGS[tune] in name:
            m[off // 4: off // 4 + int(np.prod(shape))] = True
    return m


def masked_momentum_update(blob, accum, grad, lr, tune, momentum=0.9):
    """MomentumOptimizer.minimize(var_list = the tuned variables): the others, and their (absent) slots, do not move"""
    m = tune_mask(tune)
    nb, na = train_ref.momentum_update(blob, accum, grad, lr, momentum)
    return np.where(m, nb, blob), np.where(m, na, accum)
