"""TEST INFRASTRUCTURE: numpy restatement of the partition decisions, written from the text of include/ethcnn.h "partition decisions" on
top of the simulator's restatement (sim_ref.Set holds the set: bins, geometry, truth flags, sub-batches).  One candidate; nodes and
blocks in the raster order of the 21 probabilities throughout, a Python loop over the 21 nodes."""
import numpy as np

import sim_ref

LEVEL = np.array([0] + [1] * 4 + [2] * 16)
PARENT = np.array([-1] + [0] * 4 + [1 + p for p in sim_ref.PARENT32])  # node -> the node above it
BAD, LABELLED, REJECTED, GATE1_CLOSED, GATE2_CLOSED = 1, 2, 4, 8, 16
COUNTS_FIELD_OF_CODE = {1: "current_only", 2: "split_only", 3: "both", 4: "edge_split"}


def gates_open(s, up, down, gates, sl):
    """-> (open1, open2) bool [n] of the CTUs in slice sl"""
    sub = s.sub[sl]
    gated = sub >= 0
    if gates == sim_ref.GATES_NONE:
        return np.ones(sub.size, bool), np.ones(sub.size, bool)
    g1, g2 = (down[0], down[1]) if gates == sim_ref.GATES_AI else (up[0], up[1])
    m1 = np.where(gated, np.asarray(s.m1 + [0])[sub], 0)
    m2 = np.where(gated, np.asarray(s.m2 + [0])[sub], 0)
    open1 = ~gated | (m1 > g1)
    open2 = ~gated | (np.where(open1, m2, 0) > g2)
    return open1, open2


def decide(s, cand, gates=sim_ref.GATES_NONE, mid_k=512, first=0, n=None):
    """s: sim_ref.Set, cand: one sim_ref.THR record -> dict codes uint8 [n, 24], reach uint8 [n, 16], depth uint8 [n, 16]"""
    cand = np.asarray(cand, sim_ref.THR).reshape(1)[0]
    up, down = [int(x) for x in cand["up_k"]], [int(x) for x in cand["down_k"]]
    assert all(0 <= u <= 1024 for u in up) and all(-1 <= d <= 1024 for d in down) and 0 <= mid_k <= 1024
    n = s.ctus - first if n is None else n
    assert 0 <= first and 0 <= n and first + n <= s.ctus
    sl = slice(first, first + n)
    bins, inside, edge, truth, labelled, n8 = s.bins[sl].copy(), s.inside[sl], s.edge[sl], s.truth[sl], s.labelled[sl], s.n8[sl]
    live = inside[:, 0] | edge[:, 0]                   # a rejected CTU has neither
    open1, open2 = gates_open(s, up, down, gates, sl)
    bins[~open1, 1:5] = 0                              # a closed gate zeroes the level's bins before the rule
    bins[~open2, 5:] = 0
    code = np.zeros((n, 21), np.int64)
    wrong = np.zeros((n, 21), bool)
    for r in range(21):
        visited = np.ones(n, bool) if r == 0 else np.isin(code[:, PARENT[r]], (2, 3, 4))
        d = LEVEL[r]
        at_edge, decided = visited & edge[:, r], visited & inside[:, r]
        split_only = decided & (bins[:, r] > up[d])
        current_only = decided & ~split_only & (bins[:, r] <= down[d])
        both = decided & ~split_only & ~current_only
        code[:, r] = 4 * at_edge + 2 * split_only + 1 * current_only + 3 * both
        wrong[:, r] = labelled & ((split_only & ~truth[:, r]) | (current_only & truth[:, r]))
    goes_below, can_stop = np.isin(code, (2, 3, 4)), np.isin(code, (1, 3))
    codes = np.zeros((n, 24), np.uint8)
    codes[:, :21] = code + 8 * wrong
    codes[:, 21] = (BAD * wrong.any(axis=1) + LABELLED * labelled + REJECTED * ~live + GATE1_CLOSED * (live & ~open1) + GATE2_CLOSED * (live & ~open2))
    codes[:, 22] = (goes_below[:, 5:] * n8).sum(axis=1)
    # reach and the preferred partition, block by block
    prefers_split = np.isin(code, (2, 4)) | ((code == 3) & (bins > mid_k))
    reach, depth = np.zeros((n, 16), np.uint8), np.full((n, 16), 255, np.uint8)
    for b in range(16):
        path = (0, 1 + sim_ref.PARENT32[b], 5 + b)
        above = np.ones(n, bool)                       # every node above the level goes below
        alive = live.copy()                            # the preferred walk has come this far
        for d, r in enumerate(path):
            reach[:, b] |= ((above & can_stop[:, r]).astype(np.uint8) << d).astype(np.uint8)
            here = alive & (code[:, r] != 0)
            stop = here & ~prefers_split[:, r]
            depth[stop, b] = d
            alive = here & prefers_split[:, r]
            above = above & goes_below[:, r]
        reach[:, b] |= (above.astype(np.uint8) << 3).astype(np.uint8)
        depth[alive, b] = 3
    return {"codes": codes, "reach": reach, "depth": depth}


def planes_of(depth, width, height):
    """depth uint8 [frames * nctu, 16] of whole frames -> label planes uint8 [frames, height / 16, width / 16]"""
    assert width % 16 == 0 and height % 16 == 0
    cw, ch = (width + 63) // 64, (height + 63) // 64
    frames = depth.shape[0] // (cw * ch)
    full = depth.reshape(frames, ch, cw, 4, 4).transpose(0, 1, 3, 2, 4).reshape(frames, ch * 4, cw * 4)
    return np.ascontiguousarray(full[:, :height // 16, :width // 16])


def counts_from_codes(codes):
    """the restatement of ethcnn_decide_counts_from_codes -> one sim_ref.COUNTS record"""
    codes = np.asarray(codes, np.uint8).reshape(-1, 24)
    out = np.zeros(1, sim_ref.COUNTS)[0]
    for d, (a, b) in enumerate(((0, 1), (1, 5), (5, 21))):
        c = codes[:, a:b]
        for value, field in COUNTS_FIELD_OF_CODE.items():
            out[field][d] = int(((c & 7) == value).sum())
        out["checked"][d] = int(np.isin(c & 7, (1, 3)).sum())
        out["wrong_split"][d], out["wrong_stop"][d] = int((c == (2 | 8)).sum()), int((c == (1 | 8)).sum())
    out["checked"][3] = int(codes[:, 22].astype(np.int64).sum())
    out["bad_ctus"] = int((codes[:, 21] & BAD).astype(bool).sum())
    return out


def label_leaf_lacks(reach, depth16):
    """bool [n]: some block's reach lacks the bit of its label depth"""
    return ((reach.astype(np.int64) >> depth16.astype(np.int64)) & 1 == 0).any(axis=1)


def split_only_below_label(codes, depth16):
    """bool [n]: a SPLIT ONLY node below the label's leaf on some block's path (the wrong_split that leaves the label reachable)"""
    code = codes[:, :21] & 7
    out = np.zeros(codes.shape[0], bool)
    for b in range(16):
        path = (0, 1 + sim_ref.PARENT32[b], 5 + b)
        for d, r in enumerate(path):
            out |= (code[:, r] == 2) & (depth16[:, b].astype(np.int64) < d)
    return out


def random_quadtrees(rng, n):
    """uint8 [n, 16]: consistent partitions -- a 64 x 64 leaf is 0 everywhere, a 32 x 32 leaf 1 on its four blocks, else 2 or 3 per block"""
    d = rng.integers(2, 4, size=(n, 16)).astype(np.uint8)
    for j in range(4):
        stop32 = rng.integers(0, 3, size=n) == 0
        for b in range(16):
            if sim_ref.PARENT32[b] == j:
                d[stop32, b] = 1
    d[rng.integers(0, 4, size=n) == 0] = 0
    return d


# ------------------------------------------------------------------------------------------------------------- shared cases ---
GATE_CAND = ((600, 700, 800), (500, 600, 200))  # closes gates of gate_case() under both gated orders


def candidates(rng, k):
    """k candidates: the one that fills every counter, the full search, up = down, crossed; the rest random, a third of them crossed"""
    up, down = rng.integers(0, 1025, size=(k, 3)), rng.integers(-1, 1025, size=(k, 3))
    keep = rng.integers(0, 3, size=k) > 0
    lo, hi = np.minimum(up, down), np.maximum(up, down)
    up, down = np.maximum(np.where(keep[:, None], hi, up), 0), np.where(keep[:, None], lo, down)
    up[:4] = [(600, 700, 800), (1024, 1024, 1024), (512, 512, 512), (300, 400, 500)]
    down[:4] = [(400, 300, 200), (-1, -1, -1), (512, 512, 512), (700, 800, 900)]
    return sim_ref.thr(up, down)


def gate_case(rng):
    """2112 x 2048 x 2 frames: 1056 CTUs a frame = sub-batches of 1024 and 32.  The small sub-batch of frame 0 has its p64 capped at
    500 / 1024 (M1 <= 500: under GATE_CAND its level-1 gate closes, and with it the level-2 gate), that of frame 1 its p32 capped at
    600 / 1024 (M2 <= 600: only its level-2 gate closes) -> (probs [2, 1056, 21], labels [2, 128, 132])"""
    import calib_ref
    probs = calib_ref.edge_probs(rng, 2 * 1056).reshape(2, 1056, 21)
    probs[0, 1024:, 0] = np.minimum(probs[0, 1024:, 0], np.float32(500 / 1024.0))
    probs[1, 1024:, 0] = np.float32(1)
    probs[1, 1024:, 1:5] = np.minimum(probs[1, 1024:, 1:5], np.float32(600 / 1024.0))
    labels = rng.integers(0, 4, size=(2, 128, 132)).astype(np.uint8)
    return probs, labels
