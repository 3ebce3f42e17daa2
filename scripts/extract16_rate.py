"""Rates of the deep sample-set path on one MI355X -> profiles/extract16_rate.json (method: scripts/extract_rate.py and
scripts/narrow_rate.py: a warm-up, LAUNCHES launches in one synchronised window, three windows, all rows in one job on one box).

  kernels   on 16 x 1920x1080 and 4 x 4928x3264 frames of 10-bit luma resident in HBM, per workload:
              fused     k_cut_ai16 alone (cut16_device): 2 source bytes read and 1.22 record bytes written per sample
              pair      narrow_luma_device followed by cut_device on the same frames, the two launches that give the same records
                        without the fused kernel: 2 read + 1 written, then 1 read + 1.22 written
              copy      the float4 grid-stride copy (ethcnn_bench_copy) over the fused kernel's byte count
            every window is recorded, so the spread between the windows of a row can be set against the difference between rows; the
            records of both routes are compared with each other and, for the first frame, with numpy
  build     SampleSet.build of the same 200 x 1920x1080 frames as an 8-bit and as a 10-bit 4:2:0 file (twice the bytes, narrowed by the
            kernel), alternating, files in the page cache: wall seconds of every pass

    python scripts/extract16_rate.py [--out profiles/extract16_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BD = 10
QPS = [22, 27, 32, 37]
LLC = 256 << 20


def windows(ctx, launch, launches):
    """seconds per launch of three synchronised windows of `launches` launches, after a warm-up"""
    for _ in range(5):
        launch()
    ctx.synchronize()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(launches):
            launch()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) / launches)
    return out


def row(name, secs, moved):
    return dict(row=name, seconds_per_launch_windows=secs, seconds_per_launch=min(secs), window_spread_seconds=max(secs) - min(secs),
                bytes_read_plus_written=moved, bytes_read_plus_written_per_s=moved / min(secs))


def kernel_rows(pkg, ctx, w, h, frames, launches):
    import extract_cases as ec
    E = pkg.ethcnn
    rng = np.random.default_rng(w)
    one = rng.integers(0, 1 << BD, size=(min(frames, 4), h, w), dtype=np.uint16)
    one[:, ::7, ::5] = 65535
    nrec, lplane = frames * (h // 64) * (w // 64), (h // 16) * (w // 16)
    d_src, d_narrow = E.DeviceBuffer(ctx, frames * h * w * 2), E.DeviceBuffer(ctx, frames * h * w)
    for f in range(frames):  # (frame f of the set = frame f % 4 of the random ones)
        ctx._chk(ctx.lib.ethcnn_memcpy_h2d(ctx.h, d_src.ptr + f * h * w * 2, one[f % len(one)].ctypes.data, h * w * 2))
    lab = rng.integers(0, 4, (len(QPS), frames, lplane), dtype=np.uint8)
    labels = []
    for q in range(len(QPS)):
        b = E.DeviceBuffer(ctx, frames * lplane)
        b.upload(lab[q])
        labels.append(b)
    out_fused, out_pair = E.DeviceBuffer(ctx, nrec * 4992), E.DeviceBuffer(ctx, nrec * 4992)
    lptr = [b.ptr for b in labels]

    def fused():
        E.cut16_device(ctx, QPS, w, h, frames, d_src.ptr, BD, lptr, out_fused.ptr)

    def pair():
        ctx.narrow_luma_device(d_src, w, h, frames, BD, d_narrow)
        E.cut_device(ctx, E.SAMPLES_AI, QPS, w, h, frames, [d_narrow.ptr], [w], [w * h], lptr, out_pair.ptr)

    assert w % 16 == 0  # (the narrowed planes are packed: pitch roundup16(width) = width)
    covered = nrec * 4096  # samples inside whole CTUs
    moved_fused = nrec * (8192 + 16 * len(QPS) + 4992)
    moved_pair = frames * h * w * 3 + nrec * (4096 + 16 * len(QPS) + 4992)
    rows = [row("k_cut_ai16", windows(ctx, fused, launches), moved_fused),
            row("k_narrow_luma + k_cut_ai", windows(ctx, pair, launches), moved_pair)]
    a, b = out_fused.download(np.uint8, nrec * 4992), out_pair.download(np.uint8, nrec * 4992)
    per = (h // 64) * (w // 64)
    want = ec.np_cut_ai(np.minimum(one[:1] >> (BD - 8), 255).astype(np.uint8), [l[:1].reshape(1, h // 16, w // 16) for l in lab], QPS)
    same = bool(np.array_equal(a, b)) and bool(np.array_equal(a[:per * 4992], want.reshape(-1)))
    for buf in [d_src, d_narrow, out_fused, out_pair] + labels:
        buf.free()
    nbytes = moved_fused // 2 // 16 * 16
    ca, cb = E.DeviceBuffer(ctx, nbytes), E.DeviceBuffer(ctx, nbytes)
    ca.upload(np.zeros(nbytes, np.uint8))
    rows.append(row("float4 copy over the fused kernel's byte count", windows(ctx, lambda: ctx._chk(ctx.lib.ethcnn_bench_copy(ctx.h, ca.ptr, cb.ptr, nbytes)), launches),
                    2 * nbytes))
    ca.free()
    cb.free()
    fused_s, pair_s = rows[0]["seconds_per_launch"], rows[1]["seconds_per_launch"]
    return dict(width=w, height=h, frames=frames, bit_depth=BD, records=nrec, samples_in_whole_ctus=covered, launches_per_window=launches, windows=3,
                fused_working_set_bytes=moved_fused, fits_last_level_cache=moved_fused <= LLC, rows=rows,
                fused_over_pair_seconds=fused_s / pair_s, pair_minus_fused_seconds=pair_s - fused_s,
                largest_window_spread_seconds=max(rows[0]["window_spread_seconds"], rows[1]["window_spread_seconds"]),
                fused_fraction_of_copy_rate=rows[0]["bytes_read_plus_written_per_s"] / rows[2]["bytes_read_plus_written_per_s"],
                records_identical_and_equal_numpy=same), same


def build_times(pkg, ctx, w, h, frames, rounds):
    lplane = (h // 16) * (w // 16)
    need = frames * w * h * 3 // 2 * 3 + (64 << 20)
    d = None
    for base in ("/dev/shm", tempfile.gettempdir()):
        try:
            sv = os.statvfs(base)
            if sv.f_bavail * sv.f_frsize > need:
                d = tempfile.mkdtemp(prefix="ethcnn_extract16_", dir=base)
                break
        except OSError:
            pass
    if d is None:
        return dict(note="no file system with %.1f GB free: build not measured" % (need / 1e9)), True
    try:
        rng = np.random.default_rng(9)
        deep = rng.integers(0, 1 << BD, size=(8, h, w), dtype=np.uint16)
        y8, y10 = os.path.join(d, "seq8.yuv"), os.path.join(d, "seq10.yuv")
        c8, c10 = np.full(w * h // 2, 128, np.uint8).tobytes(), np.full(w * h // 2, 512, "<u2").tobytes()
        with open(y8, "wb") as f8, open(y10, "wb") as f10:
            for k in range(frames):
                f10.write(deep[k % 8].astype("<u2").tobytes())
                f10.write(c10)
                f8.write((deep[k % 8] >> (BD - 8)).astype(np.uint8).tobytes())
                f8.write(c8)
        labs = []
        for q in QPS:
            labs.append(os.path.join(d, "l%d.dat" % q))
            with open(labs[-1], "wb") as f:
                f.write(rng.integers(0, 4, frames * lplane, dtype=np.uint8).tobytes())
        runs, first, count = {8: [], 10: []}, {}, 0
        for i in range(rounds + 1):  # round 0 warms the page cache and the staging path
            for bd, src in ((8, y8), (10, y10)):
                with pkg.SampleSet(ctx, "ai", QPS) as s:
                    s.add_sequence(w, h, src, labs, bit_depth=bd)
                    t0 = time.perf_counter()
                    s.build()
                    dt = time.perf_counter() - t0
                    if i:
                        runs[bd].append(dt)
                    else:
                        first[bd] = s.read(0, min(s.count, 600))
                    count = s.count
        same = bool(np.array_equal(first[8], first[10]))
        res = dict(width=w, height=h, frames=frames, records=count, timed_passes_each=rounds, directory=os.path.dirname(d), fill_threads=ctx.host_threads,
                   first_records_identical=same, note="files in the page cache; wall time of ethcnn_samples_build including its allocations; passes alternate")
        for bd in (8, 10):
            best = min(runs[bd])
            luma = frames * w * h * (2 if bd > 8 else 1)
            res["%d_bit_4_2_0" % bd] = dict(seconds=best, all_seconds=runs[bd], records_per_s=count / best, luma_bytes_read_and_uploaded=luma,
                                            luma_bytes_per_s=luma / best)
        res["seconds_10_over_8"] = min(runs[10]) / min(runs[8])
        return res, same
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract16_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    res, ok = dict(kernels=[]), True
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        for (w, h, frames) in ((1920, 1080, 16), (4928, 3264, 4)):
            r, same = kernel_rows(pkg, ctx, w, h, 2 if a.quick else frames, 5 if a.quick else 50)
            res["kernels"].append(r)
            ok = ok and same
        res["build"], same = build_times(pkg, ctx, 1920, 1080, 8 if a.quick else 200, 1 if a.quick else 3)
        ok = ok and same
    res["not_measured"] = ["build from files that are not in the page cache", "bit depths other than 10 (the kernel's work does not depend on the shift)",
                           "source planes that are not 16-byte aligned", "more than one GPU"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
