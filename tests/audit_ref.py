"""TEST INFRASTRUCTURE: numpy restatement of the comparison of two predictions, written from the text of include/ethcnn.h "comparing two
predictions" and "partition-search simulation" (rule lines 1-4).  Nodes stay in the raster order of the 21 probabilities; the descent is
a Python loop over the 21 nodes, as in decide_ref.  Returns plain Python values under the names of ethcnn_compare_stats, plus "flags"."""
import numpy as np

import calib_ref
import sim_ref

LEVEL = np.array([0] + [1] * 4 + [2] * 16)
PARENT = np.array([-1] + [0] * 4 + [1 + p for p in sim_ref.PARENT32])  # node -> the node above it
SPANS = ((0, 1), (1, 5), (5, 21))
SUMS = ("ctus", "rejected_ctus", "over_tol", "bits_diff", "class_diff", "search_diff_ctus", "checked_a", "checked_b")
FIELDS = SUMS + ("worst_ctu", "max_abs", "with_thr")
REJECTED, OVER_TOL, CLASS, SEARCH = 1, 2, 4, 8


def geometry(n, width=None, height=None, first=0):
    """-> inside bool [n, 21], edge bool [n, 21], n8 int64 [n, 16] of CTUs first .. first + n; per-CTU layout: every node is inside"""
    if width is None:
        return np.ones((n, 21), bool), np.zeros((n, 21), bool), np.full((n, 16), 4, np.int64)
    assert width % 8 == 0 and height % 8 == 0
    cw, ch = (width + 63) // 64, (height + 63) // 64
    per = cw * ch
    inside, edge, n8 = np.zeros((per, 21), bool), np.zeros((per, 21), bool), np.zeros((per, 16), np.int64)
    for cy in range(ch):
        for cx in range(cw):
            levels, n8[cy * cw + cx] = sim_ref._geometry(min(64, width - 64 * cx), min(64, height - 64 * cy))
            inside[cy * cw + cx] = np.concatenate([lv[0] for lv in levels])
            edge[cy * cw + cx] = np.concatenate([lv[1] for lv in levels])
    at = (first + np.arange(n)) % per
    return inside[at], edge[at], n8[at]


def outcomes(bins, up, down):
    """rule line 4 for every value -> 2 SPLIT ONLY, 1 CURRENT ONLY, 3 BOTH; int64 [n, 21]"""
    up, down = np.asarray(up)[LEVEL], np.asarray(down)[LEVEL]
    split_only = bins > up
    current_only = ~split_only & (bins <= down)
    return np.where(split_only, 2, np.where(current_only, 1, 3))


def descend(outcome, inside, edge):
    """-> code int64 [n, 21]: 0 not visited, 1 / 2 / 3 the outcome of a visited decided node, 4 a visited frame-edge node"""
    code = np.zeros(outcome.shape, np.int64)
    for r in range(21):
        visited = np.ones(outcome.shape[0], bool) if r == 0 else np.isin(code[:, PARENT[r]], (2, 3, 4))
        code[:, r] = np.where(visited & inside[:, r], outcome[:, r], np.where(visited & edge[:, r], 4, 0))
    return code


def checked_of(code, n8):
    out = [int(np.isin(code[:, a:b], (1, 3)).sum()) for a, b in SPANS]
    return out + [int((np.isin(code[:, 5:], (2, 3, 4)) * n8).sum())]


def compare(a, b, tol, thr=None, width=None, height=None, first=0):
    a, b = np.asarray(a, np.float32).reshape(-1, 21), np.asarray(b, np.float32).reshape(-1, 21)
    assert a.shape == b.shape
    n = a.shape[0]
    bins_a, valid_a = calib_ref.bins_of(a)
    bins_b, valid_b = calib_ref.bins_of(b)
    ok = valid_a.all(axis=1) & valid_b.all(axis=1)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)                                  # one fp32 subtraction
        over = (d > np.float32(tol)) & ok[:, None]
    bits = (a.view(np.uint32) != b.view(np.uint32)) & ok[:, None]
    out = {"ctus": n, "rejected_ctus": int((~ok).sum()), "over_tol": [], "bits_diff": [], "max_abs": [], "worst_ctu": [],
           "class_diff": [0, 0, 0], "search_diff_ctus": 0, "checked_a": [0, 0, 0, 0], "checked_b": [0, 0, 0, 0], "with_thr": int(thr is not None)}
    idx = np.flatnonzero(ok)
    for lo, hi in SPANS:
        out["over_tol"].append(int(over[:, lo:hi].sum()))
        out["bits_diff"].append(int(bits[:, lo:hi].sum()))
        if idx.size:
            row = d[idx, lo:hi].max(axis=1)
            out["max_abs"].append(float(row.max()))
            out["worst_ctu"].append(int(idx[np.flatnonzero(row == row.max())[0]]) + first)
        else:
            out["max_abs"].append(0.0)
            out["worst_ctu"].append(-1)
    flags = np.where(ok, OVER_TOL * over.any(axis=1), REJECTED).astype(np.uint8)
    if thr is not None:
        thr = np.asarray(thr, sim_ref.THR).reshape(1)[0]
        up, down = [int(x) for x in thr["up_k"]], [int(x) for x in thr["down_k"]]
        assert all(0 <= u <= 1024 for u in up) and all(-1 <= v <= 1024 for v in down)
        inside, edge, n8 = geometry(n, width, height, first)
        oa, ob = outcomes(bins_a, up, down), outcomes(bins_b, up, down)
        cls = (oa != ob) & ok[:, None]
        ca, cb = descend(oa, inside & ok[:, None], edge & ok[:, None]), descend(ob, inside & ok[:, None], edge & ok[:, None])
        search = (ca != cb).any(axis=1)
        out["class_diff"] = [int(cls[:, lo:hi].sum()) for lo, hi in SPANS]
        out["search_diff_ctus"] = int(search.sum())
        out["checked_a"], out["checked_b"] = checked_of(ca, n8), checked_of(cb, n8)
        flags |= (CLASS * cls.any(axis=1) + SEARCH * search).astype(np.uint8)
    out["flags"] = flags
    return out


def combine(x, y):
    """the stats of a set from those of its two parts, x first: sums add, a maximum combines by (value, lowest index); y's indices are
    those of its own call and move by x's ctus"""
    out = {"with_thr": x["with_thr"]}
    for f in SUMS:
        out[f] = [p + q for p, q in zip(x[f], y[f])] if isinstance(x[f], list) else x[f] + y[f]
    out["max_abs"], out["worst_ctu"] = [], []
    for l in range(3):
        wy = y["worst_ctu"][l] + x["ctus"] if y["worst_ctu"][l] >= 0 else -1
        cands = [(v, w) for v, w in ((x["max_abs"][l], x["worst_ctu"][l]), (y["max_abs"][l], wy)) if w >= 0]
        v, w = min(cands, key=lambda c: (-c[0], c[1])) if cands else (0.0, -1)
        out["max_abs"].append(v)
        out["worst_ctu"].append(w)
    return out


def stats_equal(got, want):
    """every field of the struct, exactly; max_abs by its bits"""
    for f in FIELDS:
        g, w = got[f], want[f]
        if f == "max_abs":
            g, w = np.asarray(g, np.float32).view(np.uint32).tolist(), np.asarray(w, np.float32).view(np.uint32).tolist()
        if g != w:
            return False
    return True


def mismatch(got, want):
    return {f: (got[f], want[f]) for f in FIELDS if got[f] != want[f]}


# ------------------------------------------------------------------------------------------------------------- shared cases ---
def perturbed(rng, a, ulp_share=0.01, big_share=0.001, big=1e-3):
    """b = a with ulp_share of its CTUs moved by one ulp in one value and big_share of them by `big` in one value, kept inside [0, 1]"""
    b = np.array(a, np.float32).reshape(-1, 21)
    n = b.shape[0]
    for share, move in ((ulp_share, None), (big_share, np.float32(big))):
        rows = rng.choice(n, size=max(1, int(round(n * share))), replace=False)
        cols = rng.integers(0, 21, size=rows.size)
        v = b[rows, cols]
        up = v < np.float32(0.5)
        if move is None:
            b[rows, cols] = np.where(up, np.nextafter(v, np.float32(2)), np.nextafter(v, np.float32(-1)))
        else:
            b[rows, cols] = np.where(up, v + move, v - move)
    assert ((b >= 0) & (b <= 1)).all()
    return b.reshape(np.shape(a))


def crafted_cases():
    """the edge cases of the definition -> list of dicts: name, a, b, tol, thr (or None), width, height (or None), expect (the fields
    worked out by hand)"""
    f32 = np.float32
    thr_mid = sim_ref.thr((512, 512, 512), (100, 100, 100))
    out = []
    # a probability exactly on k / 1024 and one ulp above it: bin 512 is not > 512, bin 513 is
    a = np.full((3, 21), f32(0.5), f32)
    b = a.copy()
    b[1, 0] = np.nextafter(f32(0.5), f32(1))
    out.append(dict(name="on the grid and one ulp above", a=a, b=b, tol=1e-4, thr=thr_mid, width=None, height=None,
                    expect={"bits_diff": [1, 0, 0], "over_tol": [0, 0, 0], "class_diff": [1, 0, 0], "search_diff_ctus": 1, "max_abs": [2.0 ** -24, 0.0, 0.0],
                            "worst_ctu": [1, 0, 0], "rejected_ctus": 0, "checked_a": [3, 12, 48, 192], "checked_b": [2, 12, 48, 192]}))
    # down_k > up_k: the order of the tests decides.  bin 200: not > 300, <= 700: CURRENT ONLY; bin 301: SPLIT ONLY, and so is 1000 below it
    a = np.full((1, 21), f32(1000 / 1024.0), f32)
    b = a.copy()
    a[0, 0], b[0, 0] = f32(200 / 1024.0), f32(301 / 1024.0)
    out.append(dict(name="down_k above up_k", a=a, b=b, tol=0.05, thr=sim_ref.thr((300, 300, 300), (700, 700, 700)), width=None, height=None,
                    expect={"class_diff": [1, 0, 0], "search_diff_ctus": 1, "checked_a": [1, 0, 0, 0], "checked_b": [0, 0, 0, 64], "over_tol": [1, 0, 0],
                            "max_abs": [float(f32(301 / 1024.0) - f32(200 / 1024.0)), 0.0, 0.0]}))
    # -0.0 against 0.0: the bit patterns differ, nothing else does
    a = np.zeros((2, 21), f32)
    b = a.copy()
    b[1, 7] = f32(-0.0)
    out.append(dict(name="minus zero", a=a, b=b, tol=0.0, thr=thr_mid, width=None, height=None,
                    expect={"bits_diff": [0, 0, 1], "over_tol": [0, 0, 0], "class_diff": [0, 0, 0], "search_diff_ctus": 0, "max_abs": [0.0, 0.0, 0.0],
                            "worst_ctu": [0, 0, 0], "rejected_ctus": 0}))
    # a subnormal difference of two normal numbers, and of a subnormal against zero
    a = np.full((2, 21), f32(0.25), f32)
    b = a.copy()
    a[0, 2], b[0, 2] = f32(1.5 * 2.0 ** -126), f32(2.0 ** -126)
    a[1, 9], b[1, 9] = f32(0.0), f32(2.0 ** -149)
    out.append(dict(name="subnormal differences", a=a, b=b, tol=0.0, thr=None, width=None, height=None,
                    expect={"over_tol": [0, 1, 1], "bits_diff": [0, 1, 1], "max_abs": [0.0, 2.0 ** -127, 2.0 ** -149], "worst_ctu": [0, 0, 1],
                            "class_diff": [0, 0, 0], "search_diff_ctus": 0, "checked_a": [0, 0, 0, 0], "with_thr": 0}))
    # a rejection on one side only: the CTU's other differences count nowhere
    a = np.full((3, 21), f32(0.75), f32)
    b = a.copy()
    b[1, :] = f32(0.1)
    b[1, 4] = f32(np.nan)
    b[2, 20] = f32(0.75 + 0.125)
    out.append(dict(name="rejected on one side", a=a, b=b, tol=1e-4, thr=thr_mid, width=None, height=None,
                    expect={"rejected_ctus": 1, "over_tol": [0, 0, 1], "bits_diff": [0, 0, 1], "max_abs": [0.0, 0.0, 0.125], "worst_ctu": [0, 0, 2],
                            "class_diff": [0, 0, 0], "search_diff_ctus": 0, "ctus": 3}))
    # a maximum attained at two CTUs: the lowest index
    a = np.full((9, 21), f32(0.5), f32)
    b = a.copy()
    b[7, 3] = b[3, 2] = f32(0.75)
    b[5, 1] = f32(0.625)
    out.append(dict(name="a maximum at two CTUs", a=a, b=b, tol=0.2, thr=None, width=None, height=None,
                    expect={"max_abs": [0.0, 0.25, 0.0], "worst_ctu": [0, 3, 0], "over_tol": [0, 2, 0], "bits_diff": [0, 3, 0]}))
    # 200 x 136: partial CTUs on both edges (4 x 3 CTUs, the last column 8 wide, the last row 8 high), two frames
    rng = np.random.default_rng(2026)
    a = calib_ref.edge_probs(rng, 24)
    b = perturbed(rng, a, ulp_share=0.2, big_share=0.3, big=0.3)
    rows = rng.choice(24, size=12, replace=False)          # half the CTUs get three fresh values, so that searches differ
    for k in range(3):
        b[rows, rng.integers(0, 21, size=12)] = rng.random(12, dtype=np.float32)
    out.append(dict(name="200 x 136", a=a, b=b, tol=1e-4, thr=sim_ref.thr((600, 700, 800), (400, 300, 200)), width=200, height=136, expect={}))
    for c in out:
        c["a"].setflags(write=False)
        c["b"].setflags(write=False)
    return out
