"""TEST INFRASTRUCTURE: seeded, learnable synthetic Low-Delay-P training samples in the reference's 16516-byte record format
(ETH-CNN_Training_LDP/input_data.py:48-50; writer Extract_Data/extract_data_LDP_LDB_RA.py:122-156): a 64-byte header as the
extractor lays it out (255 fill, frame count, width, height, frame order, CTU line / column, sequence), then four slots of
[QP byte | 16 depth bytes | 4096 residual bytes] at 64 + 4113 s, QPs 22 / 27 / 32 / 37 in slot order.

Each CTU gets one depth quadtree (tests/train_data.depth_map); slot s caps it at CAPS[s], so the labels DIFFER between slots
(22 and 27 keep depth 3, 32 caps at 2, 37 at 1), and the residual of each slot is 128 + noise whose amplitude grows with that slot's
depth, so the wrong slot's labels or residual fail a test."""
import numpy as np

import train_data

REC = 16516
SLOT_BASE, SLOT_BYTES = 64, 4113
QPS = (22, 27, 32, 37)
CAPS = (3, 3, 2, 1)            # the deepest depth each slot keeps
_AMP = (1.0, 4.0, 12.0, 30.0)  # residual noise amplitude at depth 0..3


def slot_offset(s):
    return SLOT_BASE + SLOT_BYTES * s


def make_records(n, seed, qps=QPS, width=416, height=240):
    rng = np.random.default_rng(seed)
    out = np.full((n, REC), 255, np.uint8)
    ncol = width // 64
    for i in range(n):
        h = out[i]
        h[0] = 1
        h[2], h[3], h[4], h[5] = width % 256, width // 256, height % 256, height // 256
        frame, line, col = i // 24, (i % 24) // ncol, (i % 24) % ncol
        h[10:14] = [(frame >> (8 * k)) & 255 for k in range(4)]
        h[14], h[15], h[16], h[17], h[18], h[19] = line % 256, line // 256, col % 256, col // 256, seed % 256, 0
        d0 = train_data.depth_map(rng)
        for s, q in enumerate(qps):
            d = np.minimum(d0, CAPS[s]).astype(np.uint8)
            amp = np.kron(np.take(_AMP, d), np.ones((16, 16)))
            resi = 128 + rng.normal(0, 1, (64, 64)) * amp
            o = slot_offset(s)
            h[o] = q
            h[o + 1: o + 17] = d.reshape(-1)
            h[o + 17: o + 17 + 4096] = np.clip(np.rint(resi), 0, 255).astype(np.uint8).reshape(-1)
    return out.tobytes()
