"""Rate of the ladder search on one MI355X -> profiles/ladder_rate.json.

  set       synthetic labelled frames resident in HBM: labels uniform in 0..3, probabilities a noisy teacher of them on the grid
            k / 128.  "c4": 4928x3264 x 425 frames = 1,668,975 CTUs; "hd": 1920x1088 x 50 frames = 25,500 CTUs (1080 lines are not a
            multiple of 16, and label files exist for multiples of 16 only: HM's padded height).
  build     PartitionSim.build_ladder (ethcnn_ladder_build: one k_ladder_step launch per step) for the first 64 rungs at grid 8 and
            again at grid 1: wall time of the whole call, best of three, and that time per step.
  sweep     the route the library offered before: per rung six PartitionSim.sweep calls (every value of a coordinate, all counters
            back to the host) and the choice of include/ethcnn.h "search budget: building a ladder" made on the host from them; in the
            same job, best of three.  The two paths are compared for equality.

    python scripts/ladder_rate.py [--out profiles/ladder_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WEIGHTS = (64, 16, 4, 1)
RUNGS = 64


def make_set(w, h, frames, seed):
    """-> (probs float32 [frames, per, 21], labels uint8 [frames, h / 16, w / 16]); every CTU is whole"""
    assert w % 64 == 0 and h % 64 == 0
    rng = np.random.default_rng(seed)
    cw, ch = w // 64, h // 64
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16), dtype=np.uint8)
    d = labels.reshape(frames, ch, 4, cw, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 4, 4).astype(np.int32)   # [CTU][y16][x16]
    truth = np.zeros((d.shape[0], 21), bool)
    truth[:, 0] = d.sum(axis=(1, 2)) > 8
    truth[:, 1:5] = (d.reshape(-1, 2, 2, 2, 2).sum(axis=(2, 4)) > 6).reshape(-1, 4)
    truth[:, 5:] = (d == 3).reshape(-1, 16)
    p = np.where(truth, np.float32(0.72), np.float32(0.28)) + rng.normal(0.0, 0.22, size=truth.shape).astype(np.float32)
    probs = (np.clip(np.rint(p * 128), 0, 128) / 128.0).astype(np.float32)
    return probs.reshape(frames, cw * ch, 21), labels


def best_of(fn, n=3):
    best, out = None, None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def sweep_route(sim, grid, max_rungs, labelled):
    """the same walk from six sweeps per rung and a host-side choice -> list of (up_k, down_k)"""
    w = np.array(WEIGHTS, dtype=np.uint64)
    up, down = [1024] * 3, [-1] * 3
    full = sim.eval(np.array([[up, down]]), "none")[0]
    C, B = int((full["checked"] * w).sum()), int(full["bad_ctus"])
    path = [(list(up), list(down))]
    while len(path) < max_rungs:
        moves = []
        for c in range(6):
            d = c >> 1
            values, counts = sim.sweep(np.array([[up, down]]), c)
            cost = (counts["checked"] * w[None, :]).sum(axis=1)
            lo = int(values[0])
            if c & 1:
                vs = [v for v in range(0, 1025, grid) if max(down[d], 0) <= v < up[d]][::-1]
            else:
                vs = [v for v in range(0, 1025, grid) if down[d] < v <= up[d]]
            hit = next((v for v in vs if int(cost[v - lo]) < C), None)
            if hit is not None and int(counts["bad_ctus"][hit - lo]) * 10 ** 6 <= 10 ** 6 * labelled:
                cv, bv = int(cost[hit - lo]), int(counts["bad_ctus"][hit - lo])
                moves.append((Fraction(bv - B, C - cv), -(C - cv), c, hit, cv, bv))
        if not moves:
            break
        _, _, c, v, C, B = min(moves)
        (up if c & 1 else down)[c >> 1] = v
        path.append((list(up), list(down)))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ladder_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sets: a check of the script, not a measurement")
    args = ap.parse_args()
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    sets = {"hd": (1920, 1088, 50), "c4": (4928, 3264, 425)} if not args.quick else {"hd": (640, 384, 4), "c4": (1280, 704, 6)}
    result = {"device": None, "weights": list(WEIGHTS), "rungs_asked": RUNGS, "quick": bool(args.quick), "sets": {}}
    with pkg.EthCnn(device=0) as ctx:
        result["device"] = ctx.device_name
        for name, (w, h, frames) in sets.items():
            probs, labels = make_set(w, h, frames, 7)
            with pkg.PartitionSim(ctx) as sim:
                sim.add_frames(probs, labels, w, h)
                del probs
                info = sim.info()
                entry = {"width": w, "height": h, "frames": frames, "ctus": info["ctus"], "labelled_ctus": info["labelled_ctus"], "grids": {}}
                for grid in (8, 1):
                    sim.build_ladder(grid=grid, max_rungs=4)   # warm-up
                    t_build, lad = best_of(lambda: sim.build_ladder(grid=grid, max_rungs=RUNGS))
                    steps = max(len(lad["cost"]) - 1, 1)
                    t_sweep, path = best_of(lambda: sweep_route(sim, grid, RUNGS, info["labelled_ctus"]))
                    same = [(u, d) for u, d in path] == [(t["up_k"].tolist(), t["down_k"].tolist()) for t in lad["thr"]]
                    entry["grids"][str(grid)] = {
                        "rungs": len(lad["cost"]), "last_cost_share": int(lad["cost"][-1]) / int(lad["cost"][0]), "last_bad_ctus": int(lad["bad_ctus"][-1]),
                        "build_seconds": t_build, "build_seconds_per_step": t_build / steps,
                        "sweep_route_seconds": t_sweep, "sweep_route_seconds_per_step": t_sweep / steps,
                        "sweep_route_over_build": t_sweep / t_build, "paths_equal": bool(same)}
                    print(name, "grid", grid, json.dumps(entry["grids"][str(grid)]), flush=True)
                result["sets"][name] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0 if all(g["paths_equal"] for s in result["sets"].values() for g in s["grids"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
