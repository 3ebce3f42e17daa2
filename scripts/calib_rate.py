"""Rate of the calibration histogram on one MI355X -> profiles/calib_rate.json.  A record, not a gate.

  gpu    Calibrator.add_frames_device over the C4 job's geometry -- 4928x3264 (77 x 51 whole CTUs a frame), 425 frames = 1,668,975 CTUs --
         with probabilities (140 MB) and labels (27 MB) resident in HBM: after a warm-up call, one call per synchronised window (the
         call is synchronous: count launch, commit launch, the flag word back to the host), best of three
  numpy  the restatement of the tests (tests/calib_ref.py: histogram_frames) over the same arrays on the same box, once; the two
         histograms are compared for equality

    python scripts/calib_rate.py [--out profiles/calib_rate.json] [--quick]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, FRAMES = 4928, 3264, 425


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib_rate.json"))
    ap.add_argument("--quick", action="store_true", help="25 frames (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    import calib_ref
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    frames = 25 if a.quick else FRAMES
    nctu = (W // 64) * (H // 64)
    rng = np.random.default_rng(1)
    probs = rng.random((frames, nctu, 21), dtype=np.float32)
    labels = rng.integers(0, 4, size=(frames, H // 16, W // 16), dtype=np.uint8)
    res = {"width": W, "height": H, "frames": frames, "ctus": frames * nctu, "bytes_read": int(probs.nbytes + labels.nbytes)}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes)
        dp.upload(probs)
        dl.upload(labels)
        with pkg.Calibrator(ctx) as cal:
            cal.add_frames_device(dp, dl, W, H, frames)  # warm-up: code object, first launch
            ctx.synchronize()
            times = []
            for _ in range(3):
                cal.reset()
                ctx.synchronize()
                t0 = time.perf_counter()
                cal.add_frames_device(dp, dl, W, H, frames)
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
            hist, rejected, skipped = cal.get()
        dp.free()
        dl.free()
    best = min(times)
    res["gpu"] = dict(seconds=best, all_seconds=times, ctus_per_s=frames * nctu / best, bytes_per_s=res["bytes_read"] / best,
                      window="one synchronous add_frames_device call between two synchronisations, best of three")
    t0 = time.perf_counter()
    want_hist, want_rej, want_skipped = calib_ref.histogram_frames(probs, labels, W, H)
    dt = time.perf_counter() - t0
    res["numpy"] = dict(seconds=dt, ctus_per_s=frames * nctu / dt, runs=1)
    same = bool(np.array_equal(hist, want_hist) and np.array_equal(rejected, want_rej) and skipped == want_skipped)
    res["identical_counts"] = same
    res["not_measured"] = ["the host entries (they add a pageable upload)", "label planes that take the byte-wise gather (width / 16 not a multiple of 4)",
                           "other GPUs of the pool"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the GPU histogram and the numpy restatement disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
