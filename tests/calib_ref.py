"""TEST INFRASTRUCTURE: numpy restatement of the threshold calibrator, written from the definitions of include/ethcnn.h "threshold
calibration": the hierarchical histograms (per-CTU and frame layout), the choice of the six thresholds, and the Thr_info.txt line.
Python integers throughout the choice, so nothing can overflow."""
import numpy as np

BINS = 1025
IDX32 = np.array([[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]])


class BadDepth(ValueError):
    """a depth byte above 3: the library's ETHCNN_ERR_FORMAT"""


def bins_of(p):
    """float32 [...] -> (bin int64 [...], valid bool [...]); bin = ceil(p * 1024) in fp32"""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = (p >= np.float32(0)) & (p <= np.float32(1))
        b = np.ceil(np.where(valid, p, np.float32(0)) * np.float32(1024)).astype(np.int64)
    return b, valid


def _count(hist, rejected, level, truth, p):
    b, valid = bins_of(p)
    rejected[level] += int((~valid).sum())
    for t in (0, 1):
        hist[level, t] += np.bincount(b[valid & (truth == t)], minlength=BINS).astype(np.uint64)


def histogram(probs21, depth16):
    """probs [n,21] float32, depth16 [n,16] uint8 -> (hist uint64 [3,2,1025], rejected uint64 [3])"""
    p = np.asarray(probs21, dtype=np.float32).reshape(-1, 21)
    d = np.asarray(depth16).reshape(-1, 16).astype(np.int64)
    assert p.shape[0] == d.shape[0]
    if d.size and d.max() > 3:
        raise BadDepth("depth byte above 3")
    hist, rejected = np.zeros((3, 2, BINS), np.uint64), np.zeros(3, np.uint64)
    t64 = d.sum(axis=1) > 8                                    # [n]
    _count(hist, rejected, 0, t64, p[:, 0])
    d32 = d[:, IDX32]                                          # [n, 4, 4]
    t32 = d32.sum(axis=2) > 6                                  # [n, 4]
    m32 = np.broadcast_to(t64[:, None], t32.shape)
    _count(hist, rejected, 1, t32[m32], p[:, 1:5][m32])
    t16 = d32 == 3                                             # [n, 4, 4]
    m16 = np.broadcast_to((t64[:, None] & t32)[:, :, None], t16.shape)
    _count(hist, rejected, 2, t16[m16], p[:, 5:][:, IDX32][m16])
    return hist, rejected


def gather_frames(probs, labels, width, height, skip_label_frames=0):
    """probs [frames, ceil(h/64) * ceil(w/64), 21], labels [skip + frames, h/16, w/16] -> (probs [m,21], depth16 [m,16],
    skipped_partial): the whole CTUs in raster order"""
    assert width % 16 == 0 and height % 16 == 0
    cw, ch = (width + 63) // 64, (height + 63) // 64
    probs = np.asarray(probs, dtype=np.float32).reshape(-1, ch, cw, 21)
    frames = probs.shape[0]
    labels = np.asarray(labels, dtype=np.uint8).reshape(-1, height // 16, width // 16)[skip_label_frames:skip_label_frames + frames]
    assert labels.shape[0] == frames
    ww, wh = width // 64, height // 64
    lab = labels[:, :wh * 4, :ww * 4].reshape(frames, wh, 4, ww, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 16)
    return probs[:, :wh, :ww].reshape(-1, 21), lab, frames * (cw * ch - ww * wh)


def histogram_frames(probs, labels, width, height, skip_label_frames=0):
    p, d, skipped = gather_frames(probs, labels, width, height, skip_label_frames)
    hist, rejected = histogram(p, d)
    return hist, rejected, skipped


def matrices_at(hist, k):
    """the scorer's 2x2 matrices m[truth][predicted] at threshold k / 1024 on all three levels: predicted split <=> bin > k"""
    return [[[int(hist[l, t, :k + 1].sum()), int(hist[l, t, k + 1:].sum())] for t in (0, 1)] for l in range(3)]


def choose(hist, eps_down_ppm, eps_up_ppm):
    """-> list of three dicts with the fields of ethcnn_calib_level"""
    out = []
    for l in range(3):
        h0, h1 = [int(x) for x in hist[l][0]], [int(x) for x in hist[l][1]]
        n0, n1 = sum(h0), sum(h1)
        below0, below1 = [0], [0]                              # below[k + 1] = samples with bin <= k (Python integers)
        for b in range(BINS):
            below0.append(below0[-1] + h0[b])
            below1.append(below1[-1] + h1[b])
        miss = lambda k: below1[k + 1]
        fsplit = lambda k: n0 - below0[k + 1]
        down = max(k for k in range(-1, BINS) if miss(k) * 10 ** 6 <= int(eps_down_ppm[l]) * n1)
        up = min(k for k in range(0, BINS) if fsplit(k) * 10 ** 6 <= int(eps_up_ppm[l]) * n0)
        crossed = down > up
        if crossed:
            down = up = min(range(up, down + 1), key=lambda k: (miss(k) + fsplit(k), k))
        unc = sum(h0[down + 1:up + 1]) + sum(h1[down + 1:up + 1])
        tot = n0 + n1
        out.append({"n0": n0, "n1": n1, "down_k": down, "up_k": up, "down": down / 1024.0, "up": up / 1024.0, "miss": miss(down),
                    "fsplit": fsplit(up), "uncertain": unc, "uncertain_share": unc / tot if tot else 0.0,
                    "accuracy_512": (sum(h0[:513]) + sum(h1[513:])) / tot if tot else 0.0,
                    "empty_class": int(n0 == 0 or n1 == 0), "crossed": int(crossed)})
    return out


def thr_info_line(levels, order):
    """levels: three dicts with down_k / up_k; order "ai": up1 down1 up2 down2 up3 down3, "ldp": down1 up1 down2 up2 down3 up3"""
    ks = []
    for lv in levels:
        ks += [lv["up_k"], lv["down_k"]] if order == "ai" else [lv["down_k"], lv["up_k"]]
    return " ".join("%.10f" % (k / 1024.0) for k in ks) + "\n"


def edge_probs(rng, n):
    """float32 [n,21] in [0,1] seeded with the values where the bins can go wrong: exact grid values k / 1024, 0, 1 and the fp32
    neighbours of all of them"""
    p = rng.random((n, 21), dtype=np.float32)
    grid = (rng.integers(0, 1025, size=(n, 21)) / 1024.0).astype(np.float32)
    kind = rng.integers(0, 8, size=(n, 21))
    p = np.where(kind == 0, grid, p)
    p = np.where(kind == 1, np.nextafter(grid, np.float32(2)), p)
    p = np.where(kind == 2, np.nextafter(grid, np.float32(-1)), p)
    p = np.where(kind == 3, rng.choice(np.array([0, 1, 0.5, 512.0 / 1024, 511.0 / 1024, 513.0 / 1024], np.float32), size=(n, 21)), p)
    return np.clip(p, np.float32(0), np.float32(1)).astype(np.float32)


def random_depths(rng, n):
    """uint8 [n,16]: a mix of unsplit, partly and deeply split CTUs so that every level has both classes"""
    d = rng.integers(0, 4, size=(n, 16)).astype(np.uint8)
    style = rng.integers(0, 4, size=n)
    d[style == 0] = 0
    d[style == 1] = np.minimum(d[style == 1], 1)
    d[style == 2] = np.maximum(d[style == 2], 2)
    return d
