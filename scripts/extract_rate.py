"""Rates of the sample-set path on one MI355X -> profiles/extract_rate.json.

  kernels   each cut kernel alone on HBM-resident frames (4928x3264 and 1920x1080): after a warm-up, LAUNCHES launches in one
            synchronised window (no single-shot timing); records/s and bytes read + written per second, beside the 6.29 TB/s the
            kernel guide measured for a float4 copy on this part
  build     SampleSet.build from files in the page cache (one pass to warm the cache, then timed passes): records/s
  hand-off  Trainer.set_samples(set, take=True) of a set of at least 1 GB

    python scripts/extract_rate.py [--out profiles/extract_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12  # bytes/s read + written, measured float4 copy


def kernel_rate(pkg, ctx, kind, w, h, launches, frames):
    E = pkg.ethcnn
    rng = np.random.default_rng(1)
    nplanes, qps = (1, [22, 27, 32, 37]) if kind == "ai" else (4, [22, 27, 32, 37])
    rb = E.SAMPLE_BYTES[E.SAMPLES_AI if kind == "ai" else E.SAMPLES_INTER]
    nrec = frames * (h // 64) * (w // 64)
    planes, labels = [], []
    for _ in range(nplanes):
        b = E.DeviceBuffer(ctx, frames * w * h)
        b.upload(rng.integers(0, 256, frames * w * h, dtype=np.uint8))
        planes.append(b)
    for _ in qps:
        b = E.DeviceBuffer(ctx, frames * (h // 16) * (w // 16))
        b.upload(rng.integers(0, 4, frames * (h // 16) * (w // 16), dtype=np.uint8))
        labels.append(b)
    out = E.DeviceBuffer(ctx, nrec * rb)

    def launch():
        E.cut_device(ctx, E.SAMPLES_AI if kind == "ai" else E.SAMPLES_INTER, qps, w, h, frames, [p.ptr for p in planes], [w] * nplanes,
                     [w * h] * nplanes, [l.ptr for l in labels], out.ptr)

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
    for b in planes + labels + [out]:
        b.free()
    moved = nrec * (nplanes * 4096 + 16 * len(qps) + rb)
    return dict(kind=kind, width=w, height=h, frames_per_launch=frames, records_per_launch=nrec, launches_per_window=launches, windows=3,
                seconds_per_launch=best, records_per_s=nrec / best, bytes_read_plus_written_per_s=moved / best,
                fraction_of_copy_rate=moved / best / COPY_RATE)


def make_files(d, w, h, frames, qps, inter):
    rng = np.random.default_rng(2)
    frame = np.concatenate([rng.integers(0, 256, w * h, dtype=np.uint8), np.zeros(w * h // 2, np.uint8)]).tobytes()
    yuvs, labs = [], []
    for i in range(4 if inter else 1):
        yuvs.append(os.path.join(d, "p%d.yuv" % i))
        with open(yuvs[-1], "wb") as f:
            for _ in range(frames):
                f.write(frame)
    for q in qps:
        labs.append(os.path.join(d, "l%d.dat" % q))
        with open(labs[-1], "wb") as f:
            f.write(rng.integers(0, 4, frames * (h // 16) * (w // 16), dtype=np.uint8).tobytes())
    return yuvs, labs


def build_rate(pkg, ctx, kind, w, h, frames, passes):
    qps = [22, 27, 32, 37]
    with tempfile.TemporaryDirectory() as d:
        yuvs, labs = make_files(d, w, h, frames, qps, kind == "inter")
        times, count = [], 0
        for i in range(passes + 1):  # pass 0 warms the page cache and the staging path
            with pkg.SampleSet(ctx, kind, qps) as s:
                s.add_sequence(w, h, yuvs if kind == "inter" else yuvs[0], labs)
                t0 = time.perf_counter()
                s.build()
                if i:
                    times.append(time.perf_counter() - t0)
                count = s.count
    best = min(times)
    return dict(kind=kind, width=w, height=h, frames=frames, records=count, timed_passes=passes, seconds=best, records_per_s=count / best,
                host_threads=ctx.host_threads, note="files in the page cache; wall time of ethcnn_samples_build including its allocations")


def handoff(pkg, ctx, w, h, frames):
    qps = [22, 27, 32, 37]
    out = []
    for kind, net in (("ai", "ai"), ("inter", "ldp")):
        with tempfile.TemporaryDirectory() as d:
            yuvs, labs = make_files(d, w, h, frames if kind == "ai" else frames // 3 + 2, qps, kind == "inter")
            with pkg.SampleSet(ctx, kind, qps) as s, pkg.Trainer(ctx, batch=8, net=net) as tr:
                s.add_sequence(w, h, yuvs if kind == "inter" else yuvs[0], labs)
                s.build()
                nbytes = s.count * s.record_bytes
                t0 = time.perf_counter()
                tr.set_samples(pkg.ethcnn.SET_TRAIN, s, take=True)
                dt = time.perf_counter() - t0
                out.append(dict(net=net, records=nbytes // s.record_bytes, bytes=nbytes, take_seconds=dt))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    res = dict(copy_rate_bytes_per_s=COPY_RATE, kernels=[], build=[], handoff=[])
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        for kind in ("ai", "inter"):
            for (w, h) in ((4928, 3264), (1920, 1080)):
                frames = 2 if a.quick else (4 if w > 2000 else 16)
                res["kernels"].append(kernel_rate(pkg, ctx, kind, w, h, 5 if a.quick else 50, frames))
        res["build"].append(build_rate(pkg, ctx, "ai", 1920, 1080, 8 if a.quick else 200, 1 if a.quick else 3))
        res["build"].append(build_rate(pkg, ctx, "inter", 1920, 1080, 4 if a.quick else 50, 1 if a.quick else 3))
        res["handoff"] = handoff(pkg, ctx, 1920, 1080, 8 if a.quick else 440)
    res["not_measured"] = ["build from files that are not in the page cache", "sets near the size of HBM",
                           "the reference's own scripts (they do not exist on the GPU machine)", "more than one GPU"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
