"""TEST INFRASTRUCTURE: restatement of the expected wrong decisions, written from the text of include/ethcnn.h "partition-search
simulation: expected wrong decisions" on top of the simulator's restatement (sim_ref.Set holds bins and geometry): the tables (identity,
the monotone fit with fractions.Fraction), the counter (the descent of sim_ref._eval_chunk under gates none, vectorised over candidates;
from_codes gives the same numbers from decide_ref's per-node codes) and the ladder walk of ladder_ref.build with risk in place of bad.
Python integers throughout, so nothing can overflow."""
from fractions import Fraction

import numpy as np

import decide_ref
import ladder_ref as lref
import sim_ref

ONE = 1 << 20
BINS = 1025
MAGIC = "ethcnn-reliability 1"
SPANS = ((0, 1), (1, 5), (5, 21))
NO_CAP = 2 ** 64 - 1


def identity():
    return np.tile(np.arange(BINS, dtype=np.uint32) * 1024, (3, 1))


def from_hist(hist):
    """hist [3, 2, 1025] (level, truth, bin) -> uint32 [3, 1025], non-decreasing in the bin: pool-adjacent-violators as the header words it"""
    hist = np.asarray(hist).reshape(3, 2, BINS)
    out = np.zeros((3, BINS), np.uint32)
    for l in range(3):
        s = [int(x) for x in hist[l, 1]]
        t = [a + int(b) for a, b in zip(s, hist[l, 0])]
        stack = []
        for b in range(BINS):
            stack.append([s[b], t[b], b, b])
            while len(stack) >= 2:
                top, below = stack[-1], stack[-2]
                if not (top[1] == 0 or below[1] == 0 or Fraction(below[0], below[1]) > Fraction(top[0], top[1])):
                    break
                stack[-2:] = [[below[0] + top[0], below[1] + top[1], below[2], top[3]]]
        if sum(t) == 0:
            out[l] = identity()[l]
            continue
        for S, T, first, last in stack:
            value = Fraction(S, T) * ONE
            out[l, first:last + 1] = value.numerator // value.denominator
    return out


def table_text(rel):
    rel = np.asarray(rel).reshape(3, BINS)
    return MAGIC + "\n" + "".join(" ".join(str(int(x)) for x in row) + "\n" for row in rel)


def evaluate(s, cands, rel=None, chunk=None):
    """s: sim_ref.Set, cands: sim_ref.THR records -> (exp_wrong_split, exp_wrong_stop): lists of [3] Python integers per candidate, in
    units of 1 / ONE.  Gates none; every CTU that is not rejected counts, labelled or not"""
    cands = np.asarray(cands).reshape(-1)
    assert cands.dtype == sim_ref.THR
    rel = (identity() if rel is None else np.asarray(rel)).astype(np.int64).reshape(3, BINS)
    assert rel.min() >= 0 and rel.max() <= ONE
    up, down = cands["up_k"].astype(np.int64), cands["down_k"].astype(np.int64)
    assert ((up >= 0) & (up <= 1024) & (down >= -1) & (down <= 1024)).all()
    n = max(1, s.bins.shape[0])
    chunk = chunk or max(1, (1 << 22) // (16 * n))
    split, stop = [], []
    for at in range(0, cands.size, chunk):
        u, dn = up[at:at + chunk], down[at:at + chunk]
        k = u.shape[0]
        visited = np.ones((k, s.bins.shape[0], 1), bool)           # every CTU's 64 x 64 CU is visited
        sp, st = np.zeros((k, 3), np.int64), np.zeros((k, 3), np.int64)   # (a level's sum is at most n * 16 * 2^20)
        for d, (a, b) in enumerate(SPANS):
            bins, inside, edge = s.bins[None, :, a:b], s.inside[None, :, a:b], s.edge[None, :, a:b]
            decided = visited & inside                                # rule 4
            split_only = decided & (bins > u[:, None, None, d])
            current_only = decided & ~split_only & (bins <= dn[:, None, None, d])
            r = rel[d][s.bins[:, a:b]][None]                          # the table value of every node
            sp[:, d] = (split_only * (ONE - r)).sum(axis=(1, 2))
            st[:, d] = (current_only * r).sum(axis=(1, 2))
            recurse = (visited & edge) | (decided & ~current_only)    # rule 3, SPLIT ONLY and BOTH
            visited = np.repeat(recurse, 4, axis=2) if d == 0 else recurse[:, :, sim_ref.PARENT32] if d == 1 else None
        split += [[int(x) for x in row] for row in sp]
        stop += [[int(x) for x in row] for row in st]
    return split, stop


def risk_of(split, stop):
    return sum(split) + sum(stop)


def from_codes(s, codes, rel=None, first=0):
    """a second route to the same numbers: the per-node codes of the partition decisions (decide_ref.decide, PartitionSim.decide, gates
    none) of ONE candidate on CTUs first .. of s -> (exp_wrong_split [3], exp_wrong_stop [3])"""
    rel = (identity() if rel is None else np.asarray(rel)).astype(np.int64).reshape(3, BINS)
    code = np.asarray(codes)[:, :21].astype(np.int64) & 7
    bins = s.bins[first:first + code.shape[0]]
    split, stop = [], []
    for d, (a, b) in enumerate(SPANS):
        r = rel[d][bins[:, a:b]]
        split.append(int(((code[:, a:b] == 2) * (ONE - r)).sum()))
        stop.append(int(((code[:, a:b] == 1) * r).sum()))
    return split, stop


def build(s, rel=None, weights=None, grid=8, max_rungs=lref.MAX_RUNGS, max_risk_ppm=NO_CAP, stats=None):
    """the walk of ladder_ref.build with risk in place of bad -> list of rungs, each a dict: up_k, down_k, coord, value, checked,
    exp_wrong_split, exp_wrong_stop, risk, cost.  stats as in ladder_ref.build"""
    lref.check(weights, grid, max_rungs, 0)
    if not 0 <= max_risk_ppm < 2 ** 64:
        raise ValueError("max_risk_ppm")
    w = [int(x) for x in (lref.WEIGHTS if weights is None else weights)]
    counted = s.ctus - s.rejected
    if counted == 0:
        raise ValueError("no counted CTU")
    if s.ctus * (w[0] + 4 * w[1] + 16 * w[2] + 64 * w[3]) >= 2 ** 64:
        raise ValueError("the cost bound does not fit in 64 bits")

    def counts(cands):  # [(up, down)] -> [(checked, split, stop, risk, cost)]
        thr = sim_ref.thr([u for u, _ in cands], [d for _, d in cands])
        got = s.evaluate(thr, sim_ref.GATES_NONE)
        split, stop = evaluate(s, thr, rel)
        out = []
        for g, a, b in zip(got, split, stop):
            chk = [int(x) for x in g["checked"]]
            out.append((chk, a, b, risk_of(a, b), sum(x * y for x, y in zip(w, chk))))
        return out

    def rung(up, down, c, v, got):
        return {"up_k": list(up), "down_k": list(down), "coord": c, "value": v, "checked": got[0], "exp_wrong_split": got[1], "exp_wrong_stop": got[2],
                "risk": got[3], "cost": got[4]}

    up, down = list(sim_ref.FULL[0]), list(sim_ref.FULL[1])
    at = counts([(up, down)])[0]
    rungs = [rung(up, down, -1, 0, at)]
    while len(rungs) < max_rungs:
        R, C = at[3], at[4]
        moves = []
        for c in range(6):
            vs = lref._values(c, up, down, grid)
            for i in range(0, len(vs), lref.CHUNK):
                part = vs[i:i + lref.CHUNK]
                got = counts([lref._with(up, down, c, v) for v in part])
                hit = next((j for j, g in enumerate(got) if g[4] < C), None)
                if hit is not None:
                    g = got[hit]
                    if g[3] * 10 ** 6 > max_risk_ppm * counted * ONE:   # above the cap: no move, nothing further is looked at
                        if stats is not None:
                            stats["capped"] = stats.get("capped", 0) + 1
                    else:
                        moves.append((Fraction(g[3] - R, C - g[4]), -(C - g[4]), c, part[hit], g))
                    break
        if not moves:
            break
        if stats is not None and sum(1 for m in moves if m[0] == min(x[0] for x in moves)) > 1:
            stats["ties"] = stats.get("ties", 0) + 1
        _, _, c, v, at = min(moves, key=lambda m: m[:3])
        up, down = lref._with(up, down, c, v)
        rungs.append(rung(up, down, c, v, at))
    return rungs
