"""Rates of the sample-set replay on one MI355X -> profiles/replay_rate.json (method: scripts/lstm_samples_rate.py).

  copy      the float4 grid-stride copy (ethcnn_bench_copy), re-measured here: a 1 GiB buffer (beyond the 256 MB last-level cache)
            and a 64 MiB one (inside it)
  kernel    k_uncut_inter alone (ethcnn_replay_uncut_device) over all records of a synthetic 1920x1080 file of 42 frames (20160
            records: a launch touches less than the last-level cache holds) and of 136 frames (65280 records: more than it holds),
            with the source table in file order and permuted: after a warm-up, LAUNCHES launches in one synchronised window, best of
            three windows; bytes = residual and label bytes read plus written; the fraction of the copy rate of the same class
  run       one whole Replay.run_device of a 1920x1080 run of 200 frames (96000 records, uploaded from host memory) against
            ldp_sequence_device on the same planes already in HBM, alternating, three times each; the probabilities of both are
            compared word for word.  The difference is what reconstruction costs.

    python scripts/replay_rate.py [--out profiles/replay_rate.json] [--quick]
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
W, H = 1920, 1080
R, C = H // 64, W // 64
PER = R * C
REC = 16516
QPS = (22, 27, 32, 37)
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


def records(frames, first=1):
    """one 1920x1080 sequence, frames first.. in file order: random residuals and QP-slot bytes under real headers, labels in 0..3"""
    n = frames * PER
    rec = np.random.default_rng(4).integers(0, 256, (n, REC), dtype=np.uint8)
    k = np.arange(n)
    rec[:, 2:4] = np.array([W], "<u2").view(np.uint8)
    rec[:, 4:6] = np.array([H], "<u2").view(np.uint8)
    rec[:, 10:14] = (first + k // PER).astype("<u4").view(np.uint8).reshape(-1, 4)
    rec[:, 14:16] = (k % PER // C).astype("<u2").view(np.uint8).reshape(-1, 2)
    rec[:, 16:18] = (k % C).astype("<u2").view(np.uint8).reshape(-1, 2)
    rec[:, 18:20] = 0
    for s, q in enumerate(QPS):
        at = 64 + 4113 * s
        rec[:, at] = q
        rec[:, at + 1: at + 17] &= 3
    return rec


def kernel_rates(pkg, ctx, frames, copies, launches):
    E = pkg.ethcnn
    rec = records(frames)
    n = len(rec)
    d_rec = E.DeviceBuffer(ctx, rec.size)
    d_rec.upload(rec.reshape(-1))
    del rec
    d_src, d_resi, d_lab = E.DeviceBuffer(ctx, n * 8), E.DeviceBuffer(ctx, n * 4096), E.DeviceBuffer(ctx, n * 16)
    moved = 2 * n * (4096 + 16)
    ws = n * (4096 + 128 + 128) + n * (4096 + 16)  # a residual starts on no cache line; its labels sit in the line in front
    ref = copies[0 if ws > LLC else 1]
    out = []
    for order, src in (("file order", np.arange(n, dtype=np.int64)), ("permuted", np.random.default_rng(6).permutation(n).astype(np.int64))):
        d_src.upload(src)
        dt = window(ctx, lambda: E.replay_uncut_device(ctx, d_rec, n, d_src, frames, R, C, 1, d_resi, d_lab), launches)
        out.append(dict(kernel="k_uncut_inter", source_table=order, records_per_launch=n, launches_per_window=launches, windows=3,
                        seconds_per_launch=dt, bytes_read_plus_written_per_s=moved / dt, working_set_bytes=ws, fits_last_level_cache=ws <= LLC,
                        copy_rate_compared=ref["bytes_read_plus_written_per_s"], fraction_of_copy_rate=moved / dt / ref["bytes_read_plus_written_per_s"]))
    for b in (d_rec, d_src, d_resi, d_lab):
        b.free()
    return out


def whole_run(pkg, ctx, frames):
    E = pkg.ethcnn
    rec = records(frames)
    n = len(rec)
    slot = 2
    res = dict(width=W, height=H, frames=frames, records=n, record_bytes=int(rec.size), slot=slot, qp=QPS[slot])
    dp, dq, dl = E.DeviceBuffer(ctx, n * 84), E.DeviceBuffer(ctx, n * 84), E.DeviceBuffer(ctx, n * 16)
    d_planes, d_src = E.DeviceBuffer(ctx, n * 4096), E.DeviceBuffer(ctx, n * 8)
    with pkg.Replay(ctx) as rp:
        t0 = time.perf_counter()
        rp.open(rec.reshape(-1))
        res["open_host_records_seconds"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        plan = E.replay_plan(rec)
        res["host_plan_seconds"] = time.perf_counter() - t0
        d_rec = E.DeviceBuffer(ctx, rec.size)
        d_rec.upload(rec.reshape(-1))
        del rec
        d_src.upload(plan[0]["src"])
        E.replay_uncut_device(ctx, d_rec, n, d_src, frames, R, C, slot, d_planes, dl)
        ctx.synchronize()
        d_rec.free()
        replay, sequence, one_chunk = [], [], []
        for i in range(4):  # pass 0 warms the allocator, the workspace and the code objects
            for times, chunk in ((replay, 0), (one_chunk, frames)):
                rp.set_chunk_frames(chunk)
                t0 = time.perf_counter()
                rp.run_device(0, slot, dp, dl)
                ctx.synchronize()
                if i:
                    times.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.ldp_sequence_device(d_planes, C * 64, R * 64, frames, QPS[slot], 1, dq)
            ctx.synchronize()
            if i:
                sequence.append(time.perf_counter() - t0)
        res["working_bytes_default_chunk"] = (rp.set_chunk_frames(0), rp.run_bytes(0))[1]
    same = np.array_equal(dp.download(np.uint32, n * 21), dq.download(np.uint32, n * 21))
    for b in (dp, dq, dl, d_planes, d_src):
        b.free()
    res.update(replay_run_device=dict(seconds=min(replay), all_seconds=replay, chunk_frames="default (256 MB of planes: 136 frames)"),
               replay_run_device_one_chunk=dict(seconds=min(one_chunk), all_seconds=one_chunk, chunk_frames=frames),
               ldp_sequence_device_on_resident_planes=dict(seconds=min(sequence), all_seconds=sequence),
               reconstruction_seconds=min(replay) - min(sequence), reconstruction_share_of_run=(min(replay) - min(sequence)) / min(replay),
               identical_words=bool(same))
    return res, same


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_rate.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    launches = 5 if a.quick else 50
    res = {}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        ctx.load_synthetic(1, 8.0)
        ctx.load_lstm_synthetic(2, 3.0)
        ctx.set_thresholds(0.0, 0.0)
        copies = [copy_rate(pkg, ctx, (64 << 20) if a.quick else (1 << 30), launches), copy_rate(pkg, ctx, 64 << 20, launches)]
        res["float4_copy"] = copies
        res["kernel"] = sum((kernel_rates(pkg, ctx, f, copies, launches) for f in ((4, 8) if a.quick else (42, 136))), [])
        res["run"], same = whole_run(pkg, ctx, 6 if a.quick else 200)
    res["not_measured"] = ["files outside the page cache (the records are a numpy array)", "sets near the size of HBM", "more than one GPU"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("replay and the sequence call disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
