"""Rate of the histogram of reached nodes on one MI355X -> profiles/reach_rate.json.

  set        the C4 geometry of scripts/risk_rate.py, resident in HBM: 4928x3264 x 425 frames = 1,668,975 CTUs, labels uniform in 0..3, every
             CTU whole and labelled.  Twice: probabilities uniform in [0, 1) (the adds spread over 1024 bins), and saturated, every value 0
             or 1 (all adds of a level and truth meet in two LDS words: the worst contention k_reach_hist can see).
  reach      PartitionSim.reach_hist (k_reach_hist) for 1 candidate (the full search: all 21 nodes of every CTU are added) and for 16 (the
             full search and 15 rungs that prune more and more): 50 calls in one window after a warm-up, best of three windows; a call
             is synchronous and includes its scratch allocation and the copy of the histograms to the host.
  calib      Calibrator.add_frames_device over the same probabilities and labels in HBM: the existing LDS-histogram kernel (k_calib_count),
             which reads 84 + 16 bytes a CTU where k_reach_hist reads a 64-byte record per candidate.  Timed the same way.
  decide     the route that exists without the kernel: PartitionSim.decide codes to the host and a numpy histogram of the decided nodes.
             Best of three, uniform set only.
  calibrate  PartitionSim.calibrate_reached as a whole (three histograms, three choices, one evaluation): 10 calls a window, best of three.
  The ratios saturated / uniform are the finding about LDS contention.

    python scripts/reach_rate.py [--out profiles/reach_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = 50


def window(fn, calls=CALLS, n=3):
    """seconds per call: `calls` synchronous calls in one window, the best of n windows"""
    best = None
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        dt = (time.perf_counter() - t0) / calls
        best = dt if best is None else min(best, dt)
    return best


def numpy_route(sim, thr, bins, truth):
    codes = sim.decide(thr, "none", want=("codes",))["codes"]
    decided = np.isin(codes[:, :21] & 7, (1, 2, 3)) & ((codes[:, 21:22] & 2) != 0)
    hist = np.zeros((3, 2, 1025), np.uint64)
    for l, (a, b) in enumerate(((0, 1), (1, 5), (5, 21))):
        for t in (0, 1):
            hist[l, t] = np.bincount(bins[:, a:b][decided[:, a:b] & (truth[:, a:b] == bool(t))], minlength=1025)
    return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_rate.json"))
    ap.add_argument("--quick", action="store_true", help="a small set: a check of the script, not a measurement")
    args = ap.parse_args()
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    w, h, frames = (4928, 3264, 425) if not args.quick else (1280, 704, 6)
    cw, ch = w // 64, h // 64
    rng = np.random.default_rng(7)
    labels = rng.integers(0, 4, size=(frames, h // 16, w // 16), dtype=np.uint8)
    uniform = rng.random((frames, cw * ch, 21), dtype=np.float32)
    sets = {"uniform": uniform, "saturated": np.rint(uniform).astype(np.float32)}
    rungs = np.arange(16)
    cands = e.sim_thr(np.repeat((1024 - 32 * rungs)[:, None], 3, axis=1), np.repeat((32 * rungs - 1)[:, None], 3, axis=1))   # rung 0: the full search
    result = {"device": None, "quick": bool(args.quick), "width": w, "height": h, "frames": frames, "calls_per_window": CALLS, "sets": {}}
    with pkg.EthCnn(device=0) as ctx:
        result["device"] = ctx.device_name
        d_labels = ctx.alloc(labels.nbytes)
        d_labels.upload(labels)
        for name, probs in sets.items():
            entry = {}
            with pkg.PartitionSim(ctx) as sim, pkg.Calibrator(ctx) as cal:
                sim.add_frames(probs, labels, w, h)
                info = sim.info()
                result.update(ctus=info["ctus"], labelled_ctus=info["labelled_ctus"])
                one = sim.reach_hist(cands[:1])   # warm-up
                sim.reach_hist(cands)
                entry["reach_hist_1_seconds"] = window(lambda: sim.reach_hist(cands[:1]))
                entry["reach_hist_16_seconds"] = window(lambda: sim.reach_hist(cands))
                entry["reach_hist_1_ctus_per_second"] = info["ctus"] / entry["reach_hist_1_seconds"]
                entry["reach_hist_16_ctu_candidates_per_second"] = 16 * info["ctus"] / entry["reach_hist_16_seconds"]
                entry["nodes_added_full_search"] = int(one.sum())
                d_probs = ctx.alloc(probs.nbytes)
                d_probs.upload(probs)
                cal.add_frames_device(d_probs, d_labels, w, h, frames)   # warm-up
                entry["calib_add_frames_device_seconds"] = window(lambda: cal.add_frames_device(d_probs, d_labels, w, h, frames))
                entry["reach_hist_1_over_calib_add"] = entry["reach_hist_1_seconds"] / entry["calib_add_frames_device_seconds"]
                d_probs.free()
                sim.calibrate_reached(50000, 50000)   # warm-up
                entry["calibrate_reached_seconds"] = window(lambda: sim.calibrate_reached(50000, 50000), calls=10)
                if name == "uniform":
                    d = labels.reshape(frames, ch, 4, cw, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 16).astype(np.int64)
                    truth = np.zeros((d.shape[0], 21), bool)
                    idx32 = np.array([[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]])
                    truth[:, 0], truth[:, 1:5], truth[:, 5:] = d.sum(axis=1) > 8, d[:, idx32].sum(axis=2) > 6, d == 3
                    bins = np.ceil(probs.reshape(-1, 21) * np.float32(1024)).astype(np.int64)
                    mid = cands[8]
                    entry["decide_and_numpy_seconds"] = window(lambda: numpy_route(sim, mid, bins, truth), calls=1)
                    entry["decide_and_numpy_equals_reach_hist"] = bool(np.array_equal(numpy_route(sim, mid, bins, truth), sim.reach_hist(mid)[0]))
                    entry["decide_and_numpy_over_reach_hist_1"] = entry["decide_and_numpy_seconds"] / window(lambda: sim.reach_hist(mid), calls=10)
            result["sets"][name] = entry
            print(name, json.dumps(entry), flush=True)
        d_labels.free()
    u, s = result["sets"]["uniform"], result["sets"]["saturated"]
    result["saturated_over_uniform"] = {k: s[k] / u[k] for k in ("reach_hist_1_seconds", "reach_hist_16_seconds", "calib_add_frames_device_seconds",
                                                                   "calibrate_reached_seconds")}
    print("saturated / uniform", json.dumps(result["saturated_over_uniform"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
