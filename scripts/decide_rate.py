"""Rate of the partition decisions on one MI355X -> profiles/decide_rate.json (method: scripts/replay_rate.py).  A record, not a gate.

  copy     the float4 grid-stride copy (ethcnn_bench_copy), re-measured here: a 1 GiB buffer (beyond the 256 MB last-level cache)
           and a 64 MiB one (inside it)
  kernel   ethcnn_decide_frames_device over the C4 job's geometry of scripts/calib_rate.py -- 4928x3264 (77 x 51 whole CTUs a frame),
           425 frames = 1,668,975 CTUs, with labels -- with the set resident in HBM: after a warm-up, LAUNCHES calls in one window that
           ends in a synchronisation (every call is synchronous itself: launch, wait), best of three windows.  Once with codes, reach
           and planes (64 B read, 56 B written per CTU), once with the planes alone (64 B read, 16 B written).  bytes = records read
           plus output bytes written; the fraction of the copy rate of the working set's size class.
  check    the codes of the last launch, summed by ethcnn_decide_counts_from_codes, against ethcnn_sim_eval of the same candidate

    python scripts/decide_rate.py [--out profiles/decide_rate.json] [--quick]
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
W, H, FRAMES = 4928, 3264, 425
LLC = 256 << 20


def window(ctx, launch, launches):
    for _ in range(5):
        launch()
    ctx.synchronize()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(launches):
            launch()
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / launches
        best = dt if best is None else min(best, dt)
    return best


def copy_rate(pkg, ctx, nbytes, launches):
    E = pkg.ethcnn
    a, b = E.DeviceBuffer(ctx, nbytes), E.DeviceBuffer(ctx, nbytes)
    a.upload(np.zeros(nbytes, np.uint8))
    dt = window(ctx, lambda: ctx._chk(ctx.lib.ethcnn_bench_copy(ctx.h, a.ptr, b.ptr, nbytes)), launches)
    a.free()
    b.free()
    return dict(bytes=nbytes, working_set_bytes=2 * nbytes, fits_last_level_cache=2 * nbytes <= LLC, launches_per_window=launches,
                seconds_per_launch=dt, bytes_read_plus_written_per_s=2 * nbytes / dt)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decide_rate.json"))
    ap.add_argument("--quick", action="store_true", help="25 frames, 5 launches (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    E = pkg.ethcnn
    frames, launches = (25, 5) if a.quick else (FRAMES, 50)
    nctu = (W // 64) * (H // 64)
    n = frames * nctu
    rng = np.random.default_rng(1)
    probs = rng.random((frames, nctu, 21), dtype=np.float32)
    labels = rng.integers(0, 4, size=(frames, H // 16, W // 16), dtype=np.uint8)
    cand = E.sim_thr((600, 700, 800), (400, 300, 200))
    res = {"width": W, "height": H, "frames": frames, "ctus": n, "candidate": {"up_k": [600, 700, 800], "down_k": [400, 300, 200], "gates": "ai", "mid_k": 512}}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        copies = [copy_rate(pkg, ctx, (64 << 20) if a.quick else (1 << 30), launches), copy_rate(pkg, ctx, 64 << 20, launches)]
        res["float4_copy"] = copies
        with pkg.PartitionSim(ctx) as sim:
            sim.add_frames(probs, labels, W, H)
            d_codes, d_reach, d_planes = ctx.alloc(n * 24), ctx.alloc(n * 16), ctx.alloc(labels.nbytes)
            res["kernel"] = []
            for name, outs, written in (("codes + reach + planes", (d_codes, d_reach, d_planes), 56), ("planes alone", (None, None, d_planes), 16)):
                dt = window(ctx, lambda: sim.decide_frames_device(cand, "ai", 512, 0, W, H, frames, *outs), launches)
                moved, ws = n * (64 + written), n * (64 + written)
                ref = copies[0 if ws > LLC else 1]
                res["kernel"].append(dict(kernel="k_decide", outputs=name, ctus_per_launch=n, launches_per_window=launches, windows=3, seconds_per_launch=dt,
                                          ctus_per_s=n / dt, bytes_read_plus_written_per_s=moved / dt, working_set_bytes=ws, fits_last_level_cache=ws <= LLC,
                                          copy_rate_compared=ref["bytes_read_plus_written_per_s"],
                                          fraction_of_copy_rate=moved / dt / ref["bytes_read_plus_written_per_s"],
                                          window="synchronous calls (launch + wait each) in one window, best of three"))
            sim.decide_frames_device(cand, "ai", 512, 0, W, H, frames, d_codes, None, None)
            counts = E.sim_counts_from_codes(d_codes.download(np.uint8, n * 24), ctx.lib)
            same = bool(counts == sim.eval(cand, "ai")[0])
            for b in (d_codes, d_reach, d_planes):
                b.free()
    res["identical_counts"] = same
    res["not_measured"] = ["the host form (it adds a pageable download)", "the per-CTU form with its depth output", "label planes whose rows take the byte-wise stores (width / 16 not a multiple of 4)", "other GPUs of the pool"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the codes' counters and ethcnn_sim_eval disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
