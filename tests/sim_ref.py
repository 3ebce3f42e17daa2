"""TEST INFRASTRUCTURE: numpy restatement of the partition-search simulator, written from the text of include/ethcnn.h "partition-search
simulation" and from HM's rule (HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:419-463): the set (per-CTU and frame layout, gates'
sub-batches, truth flags), the evaluation vectorised over candidates, the sweep and the coordinate-descent search.  Nodes stay in the
raster order of the 21 probabilities; the search uses Python integers, so nothing can overflow."""
import numpy as np

import calib_ref

GATES_NONE, GATES_AI, GATES_LDP = 0, 1, 2
THR = np.dtype([("up_k", "<i4", (3,)), ("down_k", "<i4", (3,))])
COUNTS = np.dtype([("checked", "<u8", (4,)), ("split_only", "<u8", (3,)), ("current_only", "<u8", (3,)), ("both", "<u8", (3,)),
                   ("edge_split", "<u8", (3,)), ("wrong_split", "<u8", (3,)), ("wrong_stop", "<u8", (3,)), ("bad_ctus", "<u8")])
FIELDS = COUNTS.names
FULL = ((1024, 1024, 1024), (-1, -1, -1))
COORDS = ("down0", "up0", "down1", "up1", "down2", "up2")
PARENT32 = np.array([(i % 4) // 2 + 2 * (i // 8) for i in range(16)])  # the 32 x 32 block of 16 x 16 block x16 + 4 y16


def thr(up_k, down_k):
    up_k, down_k = np.asarray(up_k, np.int32), np.asarray(down_k, np.int32)
    out = np.zeros(up_k.shape[:-1], THR)
    out["up_k"], out["down_k"] = up_k, down_k
    return out


def _geometry(rw, rh):
    """the part rw x rh of a CTU that lies inside the picture -> per node of a level (inside, edge), and the 8 x 8 CUs inside the
    picture per 16 x 16 block"""
    out = []
    for s, nb in ((64, 1), (32, 2), (16, 4)):
        ox, oy = np.tile(np.arange(nb) * s, nb), np.repeat(np.arange(nb) * s, nb)
        inside = (ox + s <= rw) & (oy + s <= rh)
        visitable = (ox < rw) & (oy < rh)              # rule 1: a CU that starts outside the picture is not visited
        out.append((inside, visitable & ~inside))
    ox, oy = np.tile(np.arange(4) * 16, 4), np.repeat(np.arange(4) * 16, 4)
    n8 = sum(((ox + dx < rw) & (oy + dy < rh)).astype(np.int64) for dx in (0, 8) for dy in (0, 8))
    return out, n8


class Set(object):
    """the simulator's set: everything per CTU, candidate-independent"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.bins = np.zeros((0, 21), np.int64)
        self.inside, self.edge = np.zeros((0, 21), bool), np.zeros((0, 21), bool)
        self.n8 = np.zeros((0, 16), np.int64)
        self.truth, self.labelled = np.zeros((0, 21), bool), np.zeros(0, bool)
        self.sub = np.zeros(0, np.int64)               # -1: no sub-batch
        self.m1, self.m2 = [], []                      # per sub-batch
        self.ctus = self.rejected = 0

    def info(self):
        keep = self.inside[:, 0] | self.edge[:, 0]
        return {"ctus": self.ctus, "whole_ctus": int(self.inside[keep].all(axis=1).sum()), "labelled_ctus": int(self.labelled.sum()),
                "rejected_ctus": self.rejected, "sub_batches": len(self.m1)}

    def _append(self, probs, inside, edge, n8, depth, sub):
        """depth: int64 [n, 16] with -1 rows for CTUs without labels, or None"""
        bins, valid = calib_ref.bins_of(probs)
        ok = valid.all(axis=1)
        n = probs.shape[0]
        truth, labelled = np.zeros((n, 21), bool), np.zeros(n, bool)
        if depth is not None:
            has = depth[:, 0] >= 0
            if depth.max(initial=0) > 3:
                raise calib_ref.BadDepth("depth byte above 3")
            d = np.where(has[:, None], depth, 0)
            truth[:, 0] = d.sum(axis=1) > 8
            truth[:, 1:5] = d[:, calib_ref.IDX32].sum(axis=2) > 6
            truth[:, 5:] = d == 3
            labelled = has & ok
            truth &= labelled[:, None]
        new = np.unique(sub[sub >= 0])                 # new sub-batches, in order
        if new.size:
            assert np.array_equal(new, len(self.m1) + np.arange(new.size))
            sel = (sub >= 0) & ok
            m1, m2 = np.zeros(new.size, np.int64), np.zeros(new.size, np.int64)
            np.maximum.at(m1, sub[sel] - new[0], bins[sel, 0])
            np.maximum.at(m2, sub[sel] - new[0], bins[sel, 1:5].max(axis=1))
            self.m1 += [int(x) for x in m1]
            self.m2 += [int(x) for x in m2]
        inside, edge = inside & ok[:, None], edge & ok[:, None]  # a rejected CTU counts nowhere
        self.bins = np.concatenate([self.bins, bins])
        self.inside, self.edge = np.concatenate([self.inside, inside]), np.concatenate([self.edge, edge])
        self.n8 = np.concatenate([self.n8, n8])
        self.truth, self.labelled = np.concatenate([self.truth, truth]), np.concatenate([self.labelled, labelled])
        self.sub = np.concatenate([self.sub, sub])
        self.ctus += n
        self.rejected += int((~ok).sum())

    def add(self, probs, depth16=None):
        probs = np.asarray(probs, np.float32).reshape(-1, 21)
        n = probs.shape[0]
        depth = None if depth16 is None else np.asarray(depth16).reshape(n, 16).astype(np.int64)
        self._append(probs, np.ones((n, 21), bool), np.zeros((n, 21), bool), np.full((n, 16), 4, np.int64), depth, np.full(n, -1, np.int64))

    def add_frames(self, probs, labels, width, height, skip_label_frames=0):
        assert width % 8 == 0 and height % 8 == 0 and (labels is None or (width % 16 == 0 and height % 16 == 0))
        cw, ch = (width + 63) // 64, (height + 63) // 64
        probs = np.asarray(probs, np.float32).reshape(-1, ch * cw, 21)
        frames, per = probs.shape[0], ch * cw
        inside, edge, n8 = np.zeros((per, 21), bool), np.zeros((per, 21), bool), np.zeros((per, 16), np.int64)
        for cy in range(ch):
            for cx in range(cw):
                levels, n8[cy * cw + cx] = _geometry(min(64, width - 64 * cx), min(64, height - 64 * cy))
                inside[cy * cw + cx] = np.concatenate([lv[0] for lv in levels])
                edge[cy * cw + cx] = np.concatenate([lv[1] for lv in levels])
        depth = None
        if labels is not None:
            lab = np.asarray(labels, np.uint8).reshape(-1, height // 16, width // 16)[skip_label_frames:skip_label_frames + frames].astype(np.int64)
            assert lab.shape[0] == frames
            depth = np.full((frames, ch, cw, 16), -1, np.int64)
            ww, wh = width // 64, height // 64
            depth[:, :wh, :ww] = lab[:, :wh * 4, :ww * 4].reshape(frames, wh, 4, ww, 4).transpose(0, 1, 3, 2, 4).reshape(frames, wh, ww, 16)
            depth = depth.reshape(-1, 16)
        spf = (per + 1023) // 1024
        sub = len(self.m1) + (np.arange(frames)[:, None] * spf + np.arange(per)[None, :] // 1024).reshape(-1)
        self._append(probs.reshape(-1, 21), np.tile(inside, (frames, 1)), np.tile(edge, (frames, 1)), np.tile(n8, (frames, 1)), depth, sub)

    # ------------------------------------------------------------------------------------------------------------ evaluation ---
    def _eval_chunk(self, up, down, gates):
        """up, down int64 [k, 3] -> COUNTS records [k]"""
        k, n = up.shape[0], self.bins.shape[0]
        out = np.zeros(k, COUNTS)
        gated = self.sub >= 0
        if gates == GATES_NONE or not gated.any():
            open1 = open2 = np.ones((k, n), bool)
        else:
            g1, g2 = (down[:, 0], down[:, 1]) if gates == GATES_AI else (up[:, 0], up[:, 1])
            m1 = np.where(gated, np.asarray(self.m1 + [0])[self.sub], 0)
            m2 = np.where(gated, np.asarray(self.m2 + [0])[self.sub], 0)
            open1 = ~gated[None, :] | (m1[None, :] > g1[:, None])
            open2 = ~gated[None, :] | (np.where(open1, m2[None, :], 0) > g2[:, None])
        bins = [self.bins[None, :, 0:1], np.where(open1[:, :, None], self.bins[None, :, 1:5], 0), np.where(open2[:, :, None], self.bins[None, :, 5:], 0)]
        spans = ((0, 1), (1, 5), (5, 21))
        visited = np.ones((k, n, 1), bool)             # every CTU's 64 x 64 CU is visited
        bad = np.zeros((k, n), bool)
        for d, (a, b) in enumerate(spans):
            inside, edge, truth = self.inside[None, :, a:b], self.edge[None, :, a:b], self.truth[None, :, a:b]
            at_edge = visited & edge                                             # rule 3
            decided = visited & inside                                           # rule 4
            split_only = decided & (bins[d] > up[:, None, None, d])
            current_only = decided & ~split_only & (bins[d] <= down[:, None, None, d])
            both = decided & ~split_only & ~current_only
            recurse = at_edge | split_only | both
            labelled = self.labelled[None, :, None]
            wrong_split, wrong_stop = split_only & labelled & ~truth, current_only & labelled & truth
            bad |= (wrong_split | wrong_stop).any(axis=2)
            for name, what in (("split_only", split_only), ("current_only", current_only), ("both", both), ("edge_split", at_edge),
                               ("wrong_split", wrong_split), ("wrong_stop", wrong_stop)):
                out[name][:, d] = what.sum(axis=(1, 2))
            out["checked"][:, d] = (current_only | both).sum(axis=(1, 2))
            if d == 0:
                visited = np.repeat(recurse, 4, axis=2)
            elif d == 1:
                visited = recurse[:, :, PARENT32]
            else:                                      # rules 1 and 2: the 8 x 8 CUs inside the picture are checked
                out["checked"][:, 3] = (recurse * self.n8[None]).sum(axis=(1, 2))
        out["bad_ctus"] = bad.sum(axis=1)
        return out

    def evaluate(self, cands, gates=GATES_NONE, chunk=None):
        cands = np.asarray(cands).reshape(-1)
        assert cands.dtype == THR
        up, down = cands["up_k"].astype(np.int64), cands["down_k"].astype(np.int64)
        assert ((up >= 0) & (up <= 1024) & (down >= -1) & (down <= 1024)).all()
        n = max(1, self.bins.shape[0])
        chunk = chunk or max(1, (1 << 22) // (16 * n))
        parts = [self._eval_chunk(up[i:i + chunk], down[i:i + chunk], gates) for i in range(0, cands.size, chunk)]
        return np.concatenate(parts) if parts else np.zeros(0, COUNTS)

    def sweep_candidates(self, base, coord):
        lo = 0 if coord & 1 else -1
        values = np.arange(lo, 1025, dtype=np.int32)
        cands = np.repeat(np.asarray(base, THR).reshape(1), values.size)
        cands["up_k" if coord & 1 else "down_k"][:, coord >> 1] = values
        return values, cands

    def sweep(self, base, coord, gates=GATES_NONE):
        values, cands = self.sweep_candidates(base, coord)
        return values, self.evaluate(cands, gates)

    def search(self, start, gates, weights, max_bad_ppm, max_rounds=16):
        """-> (THR record, COUNTS record, rounds), or ValueError where the library says ETHCNN_ERR_ARG"""
        labelled = int(self.labelled.sum())
        if labelled == 0 or max_bad_ppm > 10 ** 6 or max_rounds < 0:
            raise ValueError("no labelled CTU, or a budget above 10^6 ppm, or negative rounds")
        cost = lambda c: sum(int(w) * int(x) for w, x in zip(weights, c["checked"]))
        feasible = lambda c: int(c["bad_ctus"]) * 10 ** 6 <= int(max_bad_ppm) * labelled
        cur = np.asarray(start, THR).reshape(1).copy()
        at = self.evaluate(cur, gates)[0]
        if not feasible(at):
            raise ValueError("infeasible start")
        rounds, changed = 0, True
        while changed and rounds < max_rounds:
            changed = False
            for coord in range(6):
                values, counts = self.sweep(cur[0], coord, gates)
                best = min((i for i in range(values.size) if feasible(counts[i])), key=lambda i: (cost(counts[i]), i))
                field = cur["up_k" if coord & 1 else "down_k"]
                if field[0, coord >> 1] != values[best]:
                    field[0, coord >> 1] = values[best]
                    changed = True
                at = counts[best]
            rounds += 1
        return cur[0], at, rounds


def equal(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


def fills_every_field(counts, edges=3, labels=True):
    """against vacuous passes: every word of the counters is non-zero for at least one candidate.  edges: the levels that can cross
    the frame edge in the set -- 0 without partial CTUs, 2 when the picture's sizes are multiples of 16 (no 16 x 16 CU crosses), else
    3; labels False: a set without labels has no wrong_* / bad_ctus by construction"""
    skip = () if labels else ("wrong_split", "wrong_stop", "bad_ctus")
    filled = {f: (counts[f].reshape(counts.shape[0], -1) != 0).any(axis=0) for f in FIELDS if f not in skip}
    filled["edge_split"] = filled["edge_split"][:int(edges)]
    return all(v.all() for v in filled.values())
