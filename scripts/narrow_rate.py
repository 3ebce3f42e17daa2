"""Rates of the high-bit-depth source path on one MI355X -> profiles/narrow_rate.json (method: scripts/replay_rate.py).

  kernel    k_narrow_luma alone (ethcnn_narrow_luma_device) on 3840x2160 x 50 frames of 10-bit samples (829 MB read + 415 MB written:
            beyond the 256 MB last-level cache) and on 1920x1080 x 8 (33 + 17 MB: inside it): after a warm-up, LAUNCHES launches in one
            synchronised window, best of three windows; bytes = source bytes read plus destination bytes written; beside it the float4
            grid-stride copy (ethcnn_bench_copy) over the same byte count, re-measured here, and the fraction of it.  The output of
            the last launch is compared with numpy.
  file      the same frames as an 8-bit 4:2:0 file and as a 10-bit 4:2:0 file (twice the bytes), both through predict_yuv_file,
            alternating, ROUNDS times each; CTU/s of the best and of every run; cu_depth.dat of both compared byte for byte.

    python scripts/narrow_rate.py [--out profiles/narrow_rate.json] [--quick]
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
LLC = 256 << 20
BD = 10


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
    nbytes = nbytes // 16 * 16
    a, b = E.DeviceBuffer(ctx, nbytes), E.DeviceBuffer(ctx, nbytes)
    a.upload(np.zeros(nbytes, np.uint8))
    dt = window(ctx, lambda: ctx._chk(ctx.lib.ethcnn_bench_copy(ctx.h, a.ptr, b.ptr, nbytes)), launches)
    a.free()
    b.free()
    return dict(bytes=nbytes, working_set_bytes=2 * nbytes, fits_last_level_cache=2 * nbytes <= LLC, launches_per_window=launches,
                seconds_per_launch=dt, bytes_read_plus_written_per_s=2 * nbytes / dt)


def kernel_rate(pkg, ctx, w, h, frames, launches):
    E = pkg.ethcnn
    rng = np.random.default_rng(w)
    one = rng.integers(0, 1 << BD, size=(min(frames, 4), h, w), dtype=np.uint16)
    one[:, ::7, ::5] = 65535
    rw = (w + 15) // 16 * 16
    d_src, d_dst = E.DeviceBuffer(ctx, frames * h * w * 2), E.DeviceBuffer(ctx, frames * h * rw)
    for f in range(frames):  # (frame f of the set = frame f % 4 of the random ones)
        ctx._chk(ctx.lib.ethcnn_memcpy_h2d(ctx.h, d_src.ptr + f * h * w * 2, one[f % len(one)].ctypes.data, h * w * 2))
    moved = frames * h * (2 * w + rw)
    dt = window(ctx, lambda: ctx.narrow_luma_device(d_src, w, h, frames, BD, d_dst), launches)
    last = np.empty(h * rw, np.uint8)
    ctx._chk(ctx.lib.ethcnn_memcpy_d2h(ctx.h, last.ctypes.data, d_dst.ptr + (frames - 1) * h * rw, last.nbytes))
    want = np.zeros((h, rw), np.uint8)
    want[:, :w] = np.minimum(one[(frames - 1) % len(one)] >> (BD - 8), 255)
    same = bool(np.array_equal(last.reshape(h, rw), want))
    d_src.free()
    d_dst.free()
    copy = copy_rate(pkg, ctx, moved // 2, launches)
    return dict(kernel="k_narrow_luma", width=w, height=h, frames=frames, bit_depth=BD, launches_per_window=launches, windows=3,
                seconds_per_launch=dt, bytes_read=frames * h * w * 2, bytes_written=frames * h * rw, bytes_read_plus_written_per_s=moved / dt,
                working_set_bytes=moved, fits_last_level_cache=moved <= LLC, float4_copy_same_bytes=copy,
                fraction_of_copy_rate=moved / dt / copy["bytes_read_plus_written_per_s"], last_frame_equals_numpy=same), same


def file_scope(pkg, ctx, w, h, frames, rounds):
    nctu = pkg.ethcnn.ctus_per_frame(w, h)
    need = frames * w * h * 3 // 2 * 3 + 2 * frames * nctu * 84 + (64 << 20)
    d = None
    for base in ("/dev/shm", tempfile.gettempdir()):
        try:
            sv = os.statvfs(base)
            if sv.f_bavail * sv.f_frsize > need:
                d = tempfile.mkdtemp(prefix="ethcnn_narrow_", dir=base)
                break
        except OSError:
            pass
    if d is None:
        return dict(note="no file system with %.1f GB free: file scope not measured" % (need / 1e9)), True
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
        o8, o10 = os.path.join(d, "a.dat"), os.path.join(d, "b.dat")
        runs = {8: [], 10: []}
        for i in range(rounds + 1):  # round 0 warms the staging ring, the workspace and the page cache
            for bd, src, out in ((8, y8, o8), (10, y10, o10)):
                ctx.set_source_format(bd, 420)
                t0 = time.perf_counter()
                n = ctx.predict_yuv_file(src, w, h, 32, out)
                dt = time.perf_counter() - t0
                assert n == frames
                if i:
                    runs[bd].append(dt)
        ctx.set_source_format(8, 420)
        same = open(o8, "rb").read() == open(o10, "rb").read()
        res = dict(width=w, height=h, frames=frames, ctus=frames * nctu, directory=os.path.dirname(d), fill_threads=ctx.host_threads,
                   identical_cu_depth=bool(same))
        for bd, src in ((8, y8), (10, y10)):
            best = min(runs[bd])
            res["%d_bit_4_2_0" % bd] = dict(file_bytes=os.path.getsize(src), luma_bytes_read=frames * w * h * (2 if bd > 8 else 1),
                                            seconds=best, all_seconds=runs[bd], ctus_per_s=frames * nctu / best,
                                            luma_file_bytes_per_s=frames * w * h * (2 if bd > 8 else 1) / best,
                                            pcie_luma_bytes_per_s=frames * w * h / best)
        return res, same
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrow_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    launches = 3 if a.quick else 50
    res, ok = {}, True
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        ctx.load_synthetic(1, 8.0)
        ctx.set_thresholds(0.5, 0.5)
        res["kernel"] = []
        for (w, h, frames) in (((200, 136, 3), (768, 512, 2)) if a.quick else ((3840, 2160, 50), (1920, 1080, 8))):
            r, same = kernel_rate(pkg, ctx, w, h, frames, launches)
            res["kernel"].append(r)
            ok = ok and same
        res["file"], same = file_scope(pkg, ctx, *((416, 240, 24, 2) if a.quick else (1920, 1080, 480, 5)))
        ok = ok and same
    res["not_measured"] = ["files outside the page cache", "depths other than 10 bits (the shift amount is an operand, not a code path)", "more than one GPU"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the narrowed output differs from numpy, or the two files' cu_depth.dat differ")
    return 0


if __name__ == "__main__":
    sys.exit(main())
