"""TEST INFRASTRUCTURE: restatement of the ladder search, written from the text of include/ethcnn.h "search budget: building a ladder" on
top of the simulator's restatement (sim_ref.Set.evaluate gives every count): the greedy walk, the thinning and the ladder file, all in
Python integers, so nothing can overflow.  A step evaluates only the grid's candidates, walked outwards in small chunks."""
from fractions import Fraction

import numpy as np

import sim_ref

WEIGHTS = (64, 16, 4, 1)
MAX_RUNGS = 4096
CHUNK = 16


def check(weights, grid, max_rungs, max_bad_ppm):
    """ValueError where the library says ETHCNN_ERR_ARG"""
    if weights is not None and (len(weights) != 4 or any(not 0 <= int(w) < 2 ** 32 for w in weights)):
        raise ValueError("weights")
    if not (1 <= grid <= 1024 and grid & (grid - 1) == 0):
        raise ValueError("grid")
    if not 1 <= max_rungs <= MAX_RUNGS:
        raise ValueError("max_rungs")
    if not 0 <= max_bad_ppm <= 10 ** 6:
        raise ValueError("max_bad_ppm")


def _values(c, up, down, grid):
    """the candidate values of coordinate c, nearest to its current value first"""
    d = c >> 1
    if c & 1:
        vs = [v for v in range(0, 1025, grid) if max(down[d], 0) <= v < up[d]]
        return vs[::-1]
    return [v for v in range(0, 1025, grid) if down[d] < v <= up[d]]


def _with(up, down, c, v):
    up, down = list(up), list(down)
    (up if c & 1 else down)[c >> 1] = v
    return up, down


def build(s, weights=None, grid=8, max_rungs=MAX_RUNGS, max_bad_ppm=10 ** 6, stats=None):
    """s: sim_ref.Set -> list of rungs, each a dict: up_k, down_k (lists), coord, value, checked (4 integers), bad_ctus, cost.
    stats (a dict, optional) counts under "ties" the steps at which two moves shared the smallest ratio, and under "capped" the moves
    that the cap on bad CTUs took away"""
    check(weights, grid, max_rungs, max_bad_ppm)
    w = [int(x) for x in (WEIGHTS if weights is None else weights)]
    labelled = int(s.labelled.sum())
    if labelled == 0:
        raise ValueError("no labelled CTU")
    if s.ctus * (w[0] + 4 * w[1] + 16 * w[2] + 64 * w[3]) >= 2 ** 64:
        raise ValueError("the cost bound does not fit in 64 bits")

    def counts(cands):  # [(up, down)] -> [(checked, bad, cost)]
        got = s.evaluate(sim_ref.thr([u for u, _ in cands], [d for _, d in cands]), sim_ref.GATES_NONE)
        out = []
        for g in got:
            chk = [int(x) for x in g["checked"]]
            out.append((chk, int(g["bad_ctus"]), sum(a * b for a, b in zip(w, chk))))
        return out

    up, down = list(sim_ref.FULL[0]), list(sim_ref.FULL[1])
    chk, B, C = counts([(up, down)])[0]
    rungs = [{"up_k": list(up), "down_k": list(down), "coord": -1, "value": 0, "checked": chk, "bad_ctus": B, "cost": C}]
    while len(rungs) < max_rungs:
        moves = []
        for c in range(6):
            vs = _values(c, up, down, grid)
            for at in range(0, len(vs), CHUNK):
                part = vs[at:at + CHUNK]
                got = counts([_with(up, down, c, v) for v in part])
                hit = next((i for i, g in enumerate(got) if g[2] < C), None)
                if hit is not None:
                    chk_v, bad_v, cost_v = got[hit]
                    if bad_v * 10 ** 6 > max_bad_ppm * labelled:   # above the cap: no move, nothing further is looked at
                        if stats is not None:
                            stats["capped"] = stats.get("capped", 0) + 1
                    else:
                        moves.append((Fraction(bad_v - B, C - cost_v), -(C - cost_v), c, part[hit], chk_v, bad_v, cost_v))
                    break
        if not moves:
            break
        if stats is not None and sum(1 for m in moves if m[0] == min(x[0] for x in moves)) > 1:
            stats["ties"] = stats.get("ties", 0) + 1
        _, _, c, v, chk, B, C = min(moves, key=lambda m: m[:3])
        up, down = _with(up, down, c, v)
        rungs.append({"up_k": list(up), "down_k": list(down), "coord": c, "value": v, "checked": chk, "bad_ctus": B, "cost": C})
    return rungs


def thin(cost, K):
    """-> list of indices; ValueError where the library says ETHCNN_ERR_ARG"""
    cost = [int(x) for x in cost]
    n = len(cost)
    if n < 1 or K < 1 or any(b >= a for a, b in zip(cost, cost[1:])):
        raise ValueError("n, K, or costs that do not fall strictly")
    if n <= K:
        return list(range(n))
    if K == 1:
        return [0]
    out = []
    for j in range(K):
        target = cost[0] - j * (cost[0] - cost[n - 1]) // (K - 1)
        i = next(i for i in range(n) if cost[i] <= target)
        if i not in out:
            out.append(i)
    return sorted(out)


def ladder_lines(up, down, order):
    """the text of a ladder file: six values k / 1024 with ten decimals per rung, in the token order of `order`"""
    lines = []
    for u, d in zip(up, down):
        pairs = zip(u, d) if order == "ai" else zip(d, u)
        lines.append(" ".join("%.10f" % (int(x) / 1024.0) for p in pairs for x in p))
    return "\n".join(lines) + "\n"
