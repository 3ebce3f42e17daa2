"""TEST INFRASTRUCTURE: seeded, learnable synthetic training samples in the reference's record format
(input_data.py:16,92-116): 4096 luma bytes, 64 pad bytes, 52 x 16 label bytes (the label row of QP q at 4160 + 16 q).

Each CTU gets a random depth quadtree (so its 16 labels are a consistent HEVC partition); every leaf CU is painted
with a flat level plus noise whose amplitude grows with the leaf's depth, so deeper splits sit on busier content.
The same depths are written at every QP's row."""
import numpy as np

REC = 4992
_AMP = (1.5, 6.0, 18.0, 48.0)  # noise amplitude of a leaf CU at depth 0..3


def depth_map(rng):
    """[4,4] depths of the 16 16x16 blocks of one CTU"""
    d = np.zeros((4, 4), np.uint8)
    if rng.random() < 0.65:
        for qy in range(2):
            for qx in range(2):
                if rng.random() < 0.55:
                    for by in range(2):
                        for bx in range(2):
                            d[2 * qy + by, 2 * qx + bx] = 3 if rng.random() < 0.5 else 2
                else:
                    d[2 * qy: 2 * qy + 2, 2 * qx: 2 * qx + 2] = 1
    return d


def make_records(n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, REC), np.uint8)
    for i in range(n):
        d = depth_map(rng)
        img = np.zeros((64, 64))
        for by in range(4):
            for bx in range(4):
                dep = int(d[by, bx])
                size = 64 >> dep
                # the leaf containing this 16x16 block (depth 3 = four 8x8 leaves inside it)
                for y0 in range(by * 16, by * 16 + 16, min(size, 16)):
                    for x0 in range(bx * 16, bx * 16 + 16, min(size, 16)):
                        s = min(size, 16)
                        img[y0:y0 + s, x0:x0 + s] = rng.uniform(40, 215) + rng.normal(0, _AMP[dep], (s, s))
        # leaves bigger than 16x16 get ONE level: repaint them whole
        if d.max() == 0:
            img[:] = rng.uniform(40, 215) + rng.normal(0, _AMP[0], (64, 64))
        for qy in range(2):
            for qx in range(2):
                if (d[2 * qy: 2 * qy + 2, 2 * qx: 2 * qx + 2] == 1).all():
                    img[32 * qy: 32 * qy + 32, 32 * qx: 32 * qx + 32] = rng.uniform(40, 215) + rng.normal(0, _AMP[1], (32, 32))
        out[i, :4096] = np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(-1)
        out[i, 4160:] = np.tile(d.reshape(-1), 52)
    return out.tobytes()
