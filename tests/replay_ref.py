"""numpy restatement of include/ethcnn.h "sample-set replay": header fields, runs and their validation, the source table and the
reconstructed planes.  Plain loops over small inputs; shared by tests/test_replay_cpu.py and tests/test_gpu_replay.py."""
import numpy as np

REC = 16516
SLOT_BASE, SLOT_BYTES = 64, 4113
RULES = ("geometry", "outside", "QP differs", "QPs not distinct", "duplicate", "missing")


class ReplayFormat(Exception):
    def __init__(self, record, rule):
        Exception.__init__(self, "record %d breaks rule '%s'" % (record, rule))
        self.record, self.rule = record, rule


def _le(rec, at, nbytes):
    return sum(rec[:, at + k].astype(np.int64) << (8 * k) for k in range(nbytes))


def fields(rec):
    rec = np.asarray(rec, np.uint8).reshape(-1, REC)
    return dict(w=_le(rec, 2, 2), h=_le(rec, 4, 2), f=_le(rec, 10, 4), line=_le(rec, 14, 2), col=_le(rec, 16, 2), seq=_le(rec, 18, 2),
                qps=np.stack([rec[:, SLOT_BASE + SLOT_BYTES * s].astype(np.int64) for s in range(4)], axis=1))


def plan(rec):
    """-> the runs in order, each a dict(seq, w, h, rows, cols, f0, frames, nctu, qps, src [frames, nctu]); ReplayFormat(record, rule)
    for the first broken rule (in the order of RULES, over the whole input) and the lowest record that shows it"""
    h = fields(rec)
    n = len(h["w"])
    C, R = h["w"] // 64, h["h"] // 64
    for i in range(n):
        if h["w"][i] < 64 or h["h"][i] < 64 or h["f"][i] >= 2 ** 31:
            raise ReplayFormat(i, "geometry")
    for i in range(n):
        if h["line"][i] >= R[i] or h["col"][i] >= C[i]:
            raise ReplayFormat(i, "outside")
    members = {}  # key -> record indices, ascending; dicts keep the order of first appearance
    for i in range(n):
        members.setdefault((int(h["seq"][i]), int(h["w"][i]), int(h["h"][i])), []).append(i)
    keys = sorted(members, key=lambda k: k[0])  # stable: by seq, then by first appearance
    for i in range(n):
        first = members[(int(h["seq"][i]), int(h["w"][i]), int(h["h"][i]))][0]
        if tuple(h["qps"][i]) != tuple(h["qps"][first]):
            raise ReplayFormat(i, "QP differs")
    for first in sorted(m[0] for m in members.values()):
        if len(set(int(q) for q in h["qps"][first])) != 4:
            raise ReplayFormat(first, "QPs not distinct")
    dup = []
    for m in members.values():
        seen = set()
        for i in m:
            place = (int(h["f"][i]), int(h["line"][i]), int(h["col"][i]))
            if place in seen:
                dup.append(i)
            seen.add(place)
    if dup:
        raise ReplayFormat(min(dup), "duplicate")
    runs, missing = [], []
    for key in keys:
        m = members[key]
        rows, cols = key[2] // 64, key[1] // 64
        f0, f1 = int(h["f"][m].min()), int(h["f"][m].max())
        at = {(int(h["f"][i]), int(h["line"][i]), int(h["col"][i])): i for i in m}
        gone = None
        for f in range(f0, f1 + 1):
            for place in ((f, l, c) for l in range(rows) for c in range(cols)):
                if gone is None and place not in at:
                    gone = place
        if gone is not None:
            missing.append(min(i for i in m if h["f"][i] >= gone[0]))
            continue
        src = np.array([at[(f, l, c)] for f in range(f0, f1 + 1) for l in range(rows) for c in range(cols)], np.int64)
        runs.append(dict(seq=key[0], w=key[1], h=key[2], rows=rows, cols=cols, f0=f0, frames=f1 - f0 + 1, nctu=rows * cols,
                         qps=[int(q) for q in h["qps"][m[0]]], src=src.reshape(f1 - f0 + 1, rows * cols)))
    if missing:
        raise ReplayFormat(min(missing), "missing")
    return runs


def planes(rec, run, slot):
    """-> (residual uint8 [frames, 64 rows, 64 cols], labels uint8 [frames, 4 rows, 4 cols]) of a run of plan() at a QP slot"""
    rec = np.asarray(rec, np.uint8).reshape(-1, REC)
    F, R, C = run["frames"], run["rows"], run["cols"]
    at = SLOT_BASE + SLOT_BYTES * slot
    picked = rec[run["src"].reshape(-1)]
    resi = picked[:, at + 17: at + 17 + 4096].reshape(F, R, C, 64, 64).transpose(0, 1, 3, 2, 4).reshape(F, 64 * R, 64 * C)
    labels = picked[:, at + 1: at + 17].reshape(F, R, C, 4, 4).transpose(0, 1, 3, 2, 4).reshape(F, 4 * R, 4 * C)
    return np.ascontiguousarray(resi), np.ascontiguousarray(labels)
