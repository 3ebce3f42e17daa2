#!/usr/bin/env python
"""Time per member-frame of a synthetic "test set" of Low-Delay-P residual sequences of different sizes and lengths, four ways,
alternated in one job (the method of scripts/ldp_group_rate.py: inputs resident in HBM, one synchronised host-clock window per
measurement, best of three windows with the spread):
  batch   one LdpBatch.run_device call for all sequences (one bundle per QP band)
  groups  one LdpGroup.sequence_device call per geometry (its four QPs: one length and one first frame each)
  solo    one ethcnn_ldp_sequence_device call per sequence, each after loading its bundle into the context (6 MB packed and
          uploaded inside the timed window: what a user of one context pays when the set is run in file order)
  solo_by_band   the same calls ordered by QP band, the bundle loaded only when the band changes (four loads)
The set: four sizes (416x240, 832x480, 1280x720, 1920x1080), each at four QPs, each size with a length of its own.  The outputs of
`batch` and `groups` are compared byte for byte with those of `solo`, every sequence.  The split comes from the context's stage timers
(HIP events around the stages).  Then the same for Replay.feed over a synthetic inter record set of small and medium runs: the runs
one at a time against feed(batch=...), the calibrator's histograms compared.
    python scripts/ldp_batch_rate.py [--frames 60] [--out profiles/ldp_batch_rate.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((416, 240), (832, 480), (1280, 720), (1920, 1080))
QPS = (22, 27, 32, 37)
REC, SLOT_BASE, SLOT_BYTES = 16516, 64, 4113
REPLAY_RUNS = ((192, 128, 1, 12), (320, 192, 1, 8), (448, 256, 2, 10), (640, 384, 1, 6), (128, 64, 3, 16), (256, 256, 1, 9))  # w, h, f0, frames


def window(ctx, fn, units):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6 / units


def stats(ts):
    return {"best": min(ts), "spread": max(ts) - min(ts), "windows": ts}


def sequences(e, ctx, blobs, frames, res):
    rng = np.random.default_rng(1)
    lengths = [max(2, frames * (6 - g) // 6) for g in range(len(SIZES))]  # 60, 50, 40, 30 at --frames 60
    seqs, bufs, groups = [], [], []
    for g, (w, h) in enumerate(SIZES):
        n, nf = e.ctus_per_frame(w, h), lengths[g]
        lum = rng.integers(0, 256, size=(nf + len(QPS) - 1, h, w), dtype=np.uint8)  # one pool: member m reads frames m .. m + nf - 1
        d_l = ctx.alloc(lum.size)
        d_l.upload(lum.reshape(-1))
        del lum
        bufs.append(d_l)
        group = e.LdpGroup(ctx, len(QPS))
        for m in range(len(QPS)):
            group.load_lstm_blob(m, blobs[m])
        groups.append(group)
        for m, qp in enumerate(QPS):
            out = [ctx.alloc(nf * n * 21 * 4) for _ in range(3)]  # batch, groups, solo
            bufs += out
            seqs.append({"g": g, "w": w, "h": h, "n": n, "nf": nf, "qp": qp, "bundle": m, "luma": d_l.ptr + m * w * h, "out": out})
    batch = e.LdpBatch(ctx, len(QPS))
    for m in range(len(QPS)):
        batch.load_lstm_blob(m, blobs[m])
    call = [{"d_luma": q["luma"], "width": q["w"], "height": q["h"], "nframes": q["nf"], "qp": q["qp"], "i_frame_first": 1, "bundle": q["bundle"],
             "d_probs": q["out"][0]} for q in seqs]

    def run_batch():
        batch.run_device(call)

    def run_groups():
        for g, (w, h) in enumerate(SIZES):
            mine = [q for q in seqs if q["g"] == g]
            groups[g].sequence_device([q["luma"] for q in mine], w, h, lengths[g], QPS, 1, [q["out"][1] for q in mine])

    def run_solo():
        for q in seqs:
            ctx.load_lstm_blob(blobs[q["bundle"]])
            ctx.ldp_sequence_device(q["luma"], q["w"], q["h"], q["nf"], q["qp"], 1, q["out"][2])

    def run_solo_by_band():
        for m in range(len(QPS)):
            ctx.load_lstm_blob(blobs[m])
            for q in seqs:
                if q["bundle"] == m:
                    ctx.ldp_sequence_device(q["luma"], q["w"], q["h"], q["nf"], q["qp"], 1, q["out"][2])

    forms = {"batch": run_batch, "groups": run_groups, "solo": run_solo, "solo_by_band": run_solo_by_band}
    units = sum(q["nf"] for q in seqs)
    for fn in forms.values():  # warm-up: allocations, first launches
        fn()
    times = {name: [] for name in forms}
    for _ in range(3):  # alternated
        for name, fn in forms.items():
            times[name].append(window(ctx, fn, units))
    ctx.synchronize()
    words = lambda q, i: q["out"][i].download(np.uint32, q["nf"] * q["n"] * 21)
    same = {"batch": all(np.array_equal(words(q, 0), words(q, 2)) for q in seqs), "groups": all(np.array_equal(words(q, 1), words(q, 2)) for q in seqs)}
    split = {}
    for name, fn in forms.items():
        ctx.set_profiling(2)
        ctx.reset_stage_times()
        fn()
        ctx.synchronize()
        ms = ctx.stage_times()["ms"]
        ctx.set_profiling(0)
        split[name] = {"front_end": (ms["tile"] + ms["trunk"] + ms["fc1"]) * 1e3 / units, "recurrence": ms["heads"] * 1e3 / units,
                       "gates": ms["gate"] * 1e3 / units}
    plan = e.ldp_batch_plan([q["n"] for q in seqs], [q["nf"] for q in seqs])
    res["sequences"] = {"set": [{"width": w, "height": h, "ctus": e.ctus_per_frame(w, h), "frames": lengths[g], "qps": list(QPS)} for g, (w, h) in enumerate(SIZES)],
                        "member_frames": units, "batch_plan": plan, "identical_to_solo": same, "split_us_per_member_frame": split,
                        "us_per_member_frame": {name: stats(ts) for name, ts in times.items()}}
    batch.close()
    for group in groups:
        group.close()
    for b in bufs:
        b.free()
    return all(same.values())


def records(rng):
    recs = []
    for seq, (w, h, f0, nf) in enumerate(REPLAY_RUNS):
        for f in range(f0, f0 + nf):
            for line in range(h // 64):
                for col in range(w // 64):
                    r = np.full(REC, 255, np.uint8)
                    r[2:6] = np.array([w, h], "<u2").view(np.uint8)
                    r[10:14] = np.array([f], "<u4").view(np.uint8)
                    r[14:20] = np.array([line, col, seq], "<u2").view(np.uint8)
                    for s, qp in enumerate(QPS):
                        at = SLOT_BASE + SLOT_BYTES * s
                        r[at] = qp
                        r[at + 1:at + 17] = rng.integers(0, 4, 16)
                        r[at + 17:at + 17 + 4096] = rng.integers(0, 256, 4096)
                    recs.append(r)
    rec = np.stack(recs)
    return rec[rng.permutation(len(rec))]


def replay(e, ctx, blobs, res):
    rec = records(np.random.default_rng(2))
    ctx.set_thresholds(0.0, 0.0)  # open gates, as for any input of a calibrator
    ctx.load_lstm_blob(blobs[2])
    units = sum(r[3] for r in REPLAY_RUNS)
    with e.Replay(ctx) as rp, e.LdpBatch(ctx, 1) as batch:
        rp.open(rec)
        batch.load_lstm_blob(0, blobs[2])
        hist, times, split = {}, {"per_run": [], "batch": []}, {}
        forms = (("per_run", {}), ("batch", {"batch": batch}))
        for rnd in range(4):  # the first round warms up
            for name, kw in forms:
                with e.Calibrator(ctx) as cal:
                    t = window(ctx, lambda: rp.feed(cal, qp=32, **kw), units)
                    hist[name] = cal.histogram()
                if rnd:
                    times[name].append(t)
        same = bool(np.array_equal(hist["per_run"], hist["batch"]))
        for name, kw in forms:  # the split of the chain's stages by HIP events (the uncut kernel and the calibrator's counting are not staged)
            with e.Calibrator(ctx) as cal:
                ctx.set_profiling(2)
                ctx.reset_stage_times()
                rp.feed(cal, qp=32, **kw)
                ctx.synchronize()
                ms = ctx.stage_times()["ms"]
                ctx.set_profiling(0)
            split[name] = {"front_end": (ms["tile"] + ms["trunk"] + ms["fc1"]) * 1e3 / units, "recurrence": ms["heads"] * 1e3 / units,
                           "gates": ms["gate"] * 1e3 / units}
    ctx.set_thresholds(0.5, 0.5)
    res["replay_feed"] = {"runs": [{"width": w, "height": h, "ctus": (w // 64) * (h // 64), "first_frame": f0, "frames": nf} for w, h, f0, nf in REPLAY_RUNS],
                          "run_frames": units, "identical_histograms": same, "split_us_per_run_frame": split, "us_per_run_frame": {name: stats(ts) for name, ts in times.items()}}
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldp_batch_rate.json"))
    a = ap.parse_args()
    e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    ctx = e.EthCnn(device=0)
    ctx.load_synthetic(21, 1.0)
    ctx.set_thresholds(0.5, 0.5)
    blobs = []
    for m in range(len(QPS)):
        ctx.load_lstm_synthetic(22 + m, 3.0)
        blobs.append(ctx.get_lstm_blob())
    res = {"device": ctx.device_name, "frames": a.frames}
    ok = sequences(e, ctx, blobs, a.frames, res)
    ok = replay(e, ctx, blobs, res) and ok
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not ok:
        sys.stderr.write("ldp_batch_rate: the forms differ\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
