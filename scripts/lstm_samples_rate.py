"""Rates of the ETH-LSTM sample-set path on one MI355X -> profiles/lstm_samples_rate.json.

  copy      the float4 grid-stride copy (ethcnn_bench_copy), re-measured here: a 1 GiB buffer (beyond the 256 MB last-level cache)
            and a 64 MiB one (inside it)
  kernels   k_resi_repack and k_lstm_sample_gather alone over all records of a synthetic file of 42 frames (20160 records: a launch
            touches less than the last-level cache holds) and of 136 frames (65280 records: more than it holds): after a warm-up,
            LAUNCHES launches in one synchronised window, best of three windows; bytes the algorithm reads + writes per second and
            the fraction of the copy rate of the same working-set class
  build     wall time of the whole build of ONE file: 1920x1080 geometry (30 x 16 = 480 CTUs a frame), frames 1..42 = 20160
            records (333 MB), heads at frames 20, 30, 40 -> 1440 x 4 slots = 5760 samples (215 MB): LstmSampleSet.build_from(host
            records), LstmSampleSet.build_from(resident inter SampleSet), and the host path it replaces,
            get_LSTM_input.build_samples(records, gpu_vectors(ctx)), in the same process; the three results are compared byte for byte
  hand-off  LstmTrainer.set_samples(set, take=True)

    python scripts/lstm_samples_rate.py [--out profiles/lstm_samples_rate.json] [--quick]
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
W, H = 1920, 1080
PER = (W // 64) * (H // 64)
REC_IN, REC_OUT = 16516, 37264
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


def make_set(pkg, ctx, d, frames):
    """an inter SampleSet of `frames` - 1 frames of 1920x1080 (the initial frame is skipped): random residuals, labels in 0..3"""
    rng = np.random.default_rng(2)
    qps = [22, 27, 32, 37]
    yuvs, labs = [], []
    for i, q in enumerate(qps):
        yuvs.append(os.path.join(d, "resi%d.yuv" % i))
        with open(yuvs[-1], "wb") as f:
            for _ in range(frames):
                f.write(rng.integers(0, 256, W * H, dtype=np.uint8).tobytes())
                f.write(bytes(W * H // 2))
        labs.append(os.path.join(d, "l%d.dat" % q))
        with open(labs[-1], "wb") as f:
            f.write(rng.integers(0, 4, frames * (H // 16) * (W // 16), dtype=np.uint8).tobytes())
    st = pkg.SampleSet(ctx, "inter", qps)
    st.add_sequence(W, H, yuvs, labs)
    return st.build()


def synthetic_records(frames):
    """`frames` frames of 1920x1080 records from frame 0 on: random bytes under real headers (the kernels read nothing else)"""
    n = frames * PER
    rec = np.random.default_rng(4).integers(0, 256, (n, REC_IN), dtype=np.uint8)
    rec[:, 2:4] = np.array([W], "<u2").view(np.uint8)
    rec[:, 4:6] = np.array([H], "<u2").view(np.uint8)
    rec[:, 10:14] = (np.arange(n) // PER).astype("<u4").view(np.uint8).reshape(-1, 4)
    return rec


def kernel_rates(pkg, ctx, frames, copies, launches):
    """both kernels over ALL records of a synthetic file of `frames` frames; working set = the bytes a launch touches"""
    E = pkg.ethcnn
    rec = synthetic_records(frames)
    n = len(rec)
    d_rec = E.DeviceBuffer(ctx, rec.size)
    d_rec.upload(rec.reshape(-1))
    heads, strides, _ = E.lstm_samples_plan(rec)
    del rec
    out = []

    def entry(kernel, dt, moved, ws, **extra):
        ref = copies[0 if ws > LLC else 1]
        out.append(dict(kernel=kernel, launches_per_window=launches, windows=3, seconds_per_launch=dt, bytes_read_plus_written_per_s=moved / dt,
                        working_set_bytes=ws, fits_last_level_cache=ws <= LLC, copy_rate_compared=ref["bytes_read_plus_written_per_s"],
                        fraction_of_copy_rate=moved / dt / ref["bytes_read_plus_written_per_s"], **extra))

    chunk = n // 32 * 32
    pic = E.DeviceBuffer(ctx, chunk * 4096)
    dt = window(ctx, lambda: ctx._chk(ctx.lib.ethcnn_bench_lstm_repack(ctx.h, d_rec.ptr, n, 0, chunk, 1, pic.ptr)), launches)
    pic.free()
    # a residual is 4096 bytes that start on no cache line: 4096 + 128 bytes of lines read, 4096 written
    entry("k_resi_repack", dt, 2 * chunk * 4096, chunk * (4096 + 128) + chunk * 4096, records_per_launch=chunk)
    m = len(heads)
    vec, d_h, d_s, smp = E.DeviceBuffer(ctx, n * 1792), E.DeviceBuffer(ctx, m * 8), E.DeviceBuffer(ctx, m * 8), E.DeviceBuffer(ctx, m * REC_OUT)
    vec.upload(np.random.default_rng(3).random(n * 448, dtype=np.float32).view(np.uint8))
    d_h.upload(heads.view(np.uint8))
    d_s.upload(strides.view(np.uint8))
    dt = window(ctx, lambda: ctx._chk(ctx.lib.ethcnn_bench_lstm_gather(ctx.h, d_rec.ptr, n, vec.ptr, d_h.ptr, d_s.ptr, m, 1, smp.ptr)),
                launches)
    # per sample: 64 info bytes, 20 x (17 bytes + 1792 of vector) read, 37264 written; touched: every vector row a head reaches
    # (at most all of them), a 128-byte line per [QP | labels] group, the samples
    entry("k_lstm_sample_gather", dt, m * (64 + 20 * (17 + 1792) + REC_OUT), min(n, 20 * m) * 1792 + 20 * m * 128 + m * REC_OUT,
          samples_per_launch=m, records=n)
    for b in (d_rec, vec, d_h, d_s, smp):
        b.free()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_samples_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    G = importlib.import_module("hevc-complexity-reduction_amd.get_LSTM_input")
    frames = 23 if a.quick else 43
    launches = 5 if a.quick else 50
    res = {}
    with pkg.EthCnn(device=0) as ctx, tempfile.TemporaryDirectory() as d:
        res["device"] = ctx.device_name
        t = pkg.Trainer(ctx, batch=8, net="ldp")
        t.init_weights(1)
        ctx.load_blob(t.get_blob())
        t.close()
        copies = [copy_rate(pkg, ctx, (64 << 20) if a.quick else (1 << 30), launches), copy_rate(pkg, ctx, 64 << 20, launches)]
        res["float4_copy"] = copies
        st = make_set(pkg, ctx, d, frames)
        rec = st.read()
        res["file"] = dict(width=W, height=H, ctus_per_frame=PER, frames="1..%d" % (frames - 1), records=len(rec), bytes=int(rec.size))
        res["kernels"] = sum((kernel_rates(pkg, ctx, f, copies, launches) for f in ((22, 42) if a.quick else (42, 136))), [])
        build = {}
        results = {}
        for name, src in (("from_host_records", rec), ("from_resident_set", st)):
            times = []
            for i in range(4):  # pass 0 warms the allocator, the workspace and the code objects
                with pkg.LstmSampleSet(ctx) as ls:
                    t0 = time.perf_counter()
                    ls.build_from(src)
                    dt = time.perf_counter() - t0
                    if i:
                        times.append(dt)
                    if i == 3:
                        results[name] = ls.read()
            build[name] = dict(seconds=min(times), all_seconds=times)
        times = []
        for i in range(2):
            t0 = time.perf_counter()
            want, _ = G.build_samples(rec, G.gpu_vectors(ctx))
            times.append(time.perf_counter() - t0)
        build["host_build_samples"] = dict(seconds=min(times), all_seconds=times)
        same = all(np.array_equal(v, want) for v in results.values())
        build["samples"] = len(want)
        build["identical_bytes"] = bool(same)
        for name in ("from_host_records", "from_resident_set"):
            build[name]["speedup_over_host_path"] = build["host_build_samples"]["seconds"] / build[name]["seconds"]
        res["build"] = build
        del results
        with pkg.LstmSampleSet(ctx) as ls, pkg.LstmTrainer(ctx, batch=8) as tr:
            ls.build_from(st)
            nbytes = ls.count * REC_OUT
            t0 = time.perf_counter()
            kept = tr.set_samples(0, ls, take=True)
            res["handoff"] = dict(samples=kept, bytes=nbytes, take_seconds=time.perf_counter() - t0,
                                  note="adopts the buffer; the time is the validation pass over every sample")
        st.close()
    res["not_measured"] = ["sets near the size of HBM", "input files outside the page cache (the host-record build reads a numpy array)",
                           "more than one GPU", "the reference's own script (it does not exist on the GPU machine)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the builders disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
