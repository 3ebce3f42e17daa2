"""TEST INFRASTRUCTURE: numpy restatement of the search budget, written from the text of include/ethcnn.h "search budget" on top of the
simulator's and the decisions' restatements (sim_ref.Set holds the set; decide_ref.decide gives the codes): the checks per frame and
rung, the choice with Python integers (nothing can overflow), and the baked rows."""
import numpy as np

import decide_ref as dref
import sim_ref

FRAME, CARRY = 0, 1
WEIGHTS = (64, 16, 4, 1)
COMPANION = ((768, 768, 768), (256, 256, 256))
VALUE_OF_CODE = np.array([0.0, 0.0, 1.0, 0.5, 1.0], np.float32)  # not visited, current only, split only, both, frame edge


def default_ladder():
    j = np.arange(513)
    return sim_ref.thr(np.repeat((1024 - j)[:, None], 3, axis=1), np.repeat((j - 1)[:, None], 3, axis=1))


def _window(s, a, b):
    """the CTUs a .. b of set s as a set of their own (the gates are never used: sub-batches stay behind)"""
    w = sim_ref.Set()
    w.bins, w.inside, w.edge, w.n8 = s.bins[a:b], s.inside[a:b], s.edge[a:b], s.n8[a:b]
    w.truth, w.labelled = s.truth[a:b], s.labelled[a:b]
    w.sub = np.full(b - a, -1, np.int64)
    w.ctus = b - a
    return w


def cost(s, ladder, first, per, nframes):
    """-> uint32 [nframes, K + 1, 4]: checked[0..3] of every rung over each frame's CTUs, column K the full search"""
    ladder = np.asarray(ladder, sim_ref.THR).reshape(-1)
    cands = np.concatenate([ladder, sim_ref.thr(*sim_ref.FULL).reshape(1)])
    out = np.zeros((nframes, cands.size, 4), np.uint32)
    for f in range(nframes):
        out[f] = _window(s, first + f * per, first + (f + 1) * per).evaluate(cands, sim_ref.GATES_NONE)["checked"]
    return out


def choose(checked, weights, budget_ppm, mode):
    """-> (rung [F], over [F], cost [F], full [F]) as lists of Python integers; ValueError where the library says ETHCNN_ERR_ARG"""
    checked = np.asarray(checked)
    k = checked.shape[1] - 1
    if not 0 <= budget_ppm <= 10 ** 6 or mode not in (FRAME, CARRY) or not 1 <= k <= 4096 or any(not 0 <= int(w) < 2 ** 32 for w in weights):
        raise ValueError("budget, mode, ladder size or weights out of range")
    rung, over, cost_out, full_out = [], [], [], []
    carry = 0
    for row in checked:
        costs = [sum(int(w) * int(x) for w, x in zip(weights, c)) for c in row]
        if max(costs) >= 2 ** 64:
            raise ValueError("a cost does not fit in 64 bits")
        full = costs[k]
        allow = budget_ppm * full + carry
        fits = [i for i in range(k) if costs[i] * 10 ** 6 <= allow]
        at = fits[0] if fits else min(range(k), key=lambda i: (costs[i], i))
        carry = allow - costs[at] * 10 ** 6 if fits and mode == CARRY else 0
        rung.append(at)
        over.append(0 if fits else 1)
        cost_out.append(costs[at])
        full_out.append(full)
    return rung, over, cost_out, full_out


def bake(s, ladder, rung, first, per, nframes):
    """-> float32 [nframes * per, 21]: the codes of each frame under its rung as the values the encoder reads"""
    ladder = np.asarray(ladder, sim_ref.THR).reshape(-1)
    out = np.zeros((nframes * per, 21), np.float32)
    for f in range(nframes):
        codes = dref.decide(s, ladder[rung[f]], sim_ref.GATES_NONE, first=first + f * per, n=per)["codes"]
        rows = VALUE_OF_CODE[codes[:, :21] & 7]
        rows[(codes[:, 21] & dref.REJECTED) != 0] = 0.5  # a rejected CTU gets the full search
        out[f * per:(f + 1) * per] = rows
    return out
