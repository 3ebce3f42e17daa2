"""TEST INFRASTRUCTURE: numpy restatement of the threshold calibration on reached nodes, written from the text of include/ethcnn.h
"threshold calibration on reached nodes" on the public arrays of sim_ref.Set (bins, inside, edge, truth, labelled, sub, m1, m2; nodes in
the raster order of the 21 probabilities).  The descent and the gates are restated here, one candidate at a time; the choice per level
is calib_ref.choose."""
import numpy as np

import calib_ref
import sim_ref

BINS = calib_ref.BINS
SPANS = ((0, 1), (1, 5), (5, 21))
PARENT32 = np.array([(i % 4) // 2 + 2 * (i // 8) for i in range(16)])  # 16 x 16 block x16 + 4 y16 lies in 32 x 32 block x32 + 2 y32


def read_bins(s, up, down, gates):
    """the bins as the encoder reads them under one candidate: int64 [n, 21], zeroed where a batch gate is closed"""
    bins = s.bins.copy()
    if gates != sim_ref.GATES_NONE and len(s.m1):
        g1, g2 = (down[0], down[1]) if gates == sim_ref.GATES_AI else (up[0], up[1])
        gated = s.sub >= 0                                   # per-CTU layout: no sub-batch, never gated
        m1, m2 = np.asarray(s.m1)[np.maximum(s.sub, 0)], np.asarray(s.m2)[np.maximum(s.sub, 0)]
        open1 = ~gated | (m1 > g1)
        open2 = ~gated | (np.where(open1, m2, 0) > g2)
        bins[~open1, 1:5] = 0
        bins[~open2, 5:] = 0
    return bins


def decided_nodes(s, bins, up, down):
    """rule lines 1 - 4: bool [n, 21], the decided nodes of every CTU under one candidate"""
    n = bins.shape[0]
    out = np.zeros((n, 21), bool)
    visited = np.ones((n, 1), bool)                          # every CTU's 64 x 64 CU is visited
    for l, (a, b) in enumerate(SPANS):
        decided = visited & s.inside[:, a:b]
        at_edge = visited & s.edge[:, a:b]
        split_only = bins[:, a:b] > up[l]
        current_only = ~split_only & (bins[:, a:b] <= down[l])   # HM tests "split only" first
        out[:, a:b] = decided
        recurse = at_edge | (decided & ~current_only)
        if l == 0:
            visited = np.repeat(recurse, 4, axis=1)
        elif l == 1:
            visited = recurse[:, PARENT32]
    return out


def reach_hist(s, cands, gates=sim_ref.GATES_NONE):
    """-> uint64 [ncand, 3, 2, 1025]"""
    cands = np.asarray(cands).reshape(-1)
    assert cands.dtype == sim_ref.THR
    out = np.zeros((cands.size, 3, 2, BINS), np.uint64)
    for c in range(cands.size):
        up, down = [int(x) for x in cands[c]["up_k"]], [int(x) for x in cands[c]["down_k"]]
        assert all(0 <= u <= 1024 for u in up) and all(-1 <= d <= 1024 for d in down)
        bins = read_bins(s, up, down, gates)
        counted = decided_nodes(s, bins, up, down) & s.labelled[:, None]
        for l, (a, b) in enumerate(SPANS):
            for t in (0, 1):
                pick = counted[:, a:b] & (s.truth[:, a:b] == bool(t))
                out[c, l, t] = np.bincount(bins[:, a:b][pick], minlength=BINS).astype(np.uint64)
    return out


def calibrate_reached(s, eps_down, eps_up, gates=sim_ref.GATES_NONE):
    """-> (three dicts with the fields of ethcnn_calib_level, THR record, COUNTS record), or ValueError where the library says
    ETHCNN_ERR_ARG"""
    if not s.labelled.any() or max(list(eps_down) + list(eps_up)) > 10 ** 6:
        raise ValueError("no labelled CTU, or a budget above 10^6 ppm")
    thr = sim_ref.thr(*sim_ref.FULL).reshape(1).copy()
    levels = []
    for l in range(3):
        lv = calib_ref.choose(reach_hist(s, thr, gates)[0], eps_down, eps_up)[l]
        levels.append(lv)
        thr["up_k"][0, l], thr["down_k"][0, l] = lv["up_k"], lv["down_k"]
    return levels, thr[0], s.evaluate(thr, gates)[0]
