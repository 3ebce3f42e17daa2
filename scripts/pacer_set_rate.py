#!/usr/bin/env python
"""Time of ONE paced round of N sequences of one picture size, two ways (the method of scripts/ldp_sessions_rate.py -- a warm-up, then
`steps` rounds in one synchronised host-clock window, best of the windows with their spread -- but with the two forms ALTERNATED window
by window inside one job, so that both meet the same neighbours on the machine):
  set    one ethcnn_pacer_set_frames_device call over the N frames: two launches whatever N is
  solo   N ethcnn_pacer_frame_device calls on N solo pacers: 2 N launches, the only route without the set
Both forms are called through the C ABI with argument arrays built once, so that the window holds the library's work and not the
binding's.  Frames and outputs are in HBM (an output buffer of its own per frame: the inputs stay as they are).  N = 1, 4, 16 at 416x240
and at 1920x1080, default ladder, budget 0.4, carry mode.  The baked words and the results of the two forms are compared.

Then the figure a user of `resi_to_cu_depth_LDP.py --sessions` sees: the GPU calls of one server round of 4 and 16 directories at
416x240 -- LdpSessions.step into page-locked buffers, and with --budget one PacerSet.frames call in place behind it -- with and without
the budget, alternated in the same way (the server's file handshake is not part of it).
    python scripts/pacer_set_rate.py [--steps 500] [--windows 5] [--out profiles/pacer_set_rate.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((416, 240), (1920, 1080))
COUNTS = (1, 4, 16)
SHARE, MODE, QP = 0.4, "carry", 32


def stats(ts):
    return {"best": min(ts), "spread": max(ts) - min(ts), "windows": ts}


def window(ctx, steps, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def paced_rounds(e, ctx, steps, windows, res):
    lib = ctx.lib
    size = e.PACER_RESULT.itemsize
    for w, h in SIZES:
        nctu = e.ctus_per_frame(w, h)
        for n in COUNTS:
            rng = np.random.default_rng(1000 + n + w)
            probs = (rng.integers(0, 1025, size=(n, nctu, 21)) / 1024.0).astype(np.float32)
            d_in, d_set, d_solo, d_res = ctx.alloc(probs.nbytes), ctx.alloc(probs.nbytes), ctx.alloc(probs.nbytes), ctx.alloc(2 * n * size)
            d_in.upload(probs)
            at = lambda b, j: b.ptr + j * nctu * 84
            pset = e.PacerSet(ctx, n, SHARE, MODE)
            solos = [e.Pacer(ctx, SHARE, MODE) for _ in range(n)]
            arr = (e.PacerSetFrame * n)(*[e.PacerSetFrame(j, at(d_in, j), w, h, at(d_set, j), d_res.ptr + j * size) for j in range(n)])
            solo_args = [(solos[j].h, at(d_in, j), w, h, at(d_solo, j), d_res.ptr + (n + j) * size) for j in range(n)]

            def set_round():
                if lib.ethcnn_pacer_set_frames_device(pset.h, arr, n):
                    raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            def solo_round():
                for a in solo_args:
                    if lib.ethcnn_pacer_frame_device(*a):
                        raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            for _ in range(20):  # warm-up of both: scratch growth, first launches
                set_round()
                solo_round()
            ts = {"set": [], "solo": []}
            for k in range(windows):  # alternated, and the order inside a pair alternates too
                for name in (("set", "solo") if k % 2 == 0 else ("solo", "set")):
                    ts[name].append(window(ctx, steps, set_round if name == "set" else solo_round))
            # both forms have paced the same frames the same number of times: carry, frame count and bytes must agree
            ctx.synchronize()
            same = bool(np.array_equal(d_set.download(np.uint32, probs.size), d_solo.download(np.uint32, probs.size)))
            records = d_res.download(np.uint8, 2 * n * size)
            same = same and records[:n * size].tobytes() == records[n * size:].tobytes()
            launches = pset.launches
            pset.close()
            for p in solos:
                p.close()
            for b in (d_in, d_set, d_solo, d_res):
                b.free()
            row = {"ctus_per_frame": nctu, "set": {"us_per_round": stats(ts["set"])}, "solo": {"us_per_round": stats(ts["solo"])}, "identical": same,
                   "set_launches_per_round": launches / float(20 + windows * steps)}
            row["solo_over_set"] = row["solo"]["us_per_round"]["best"] / row["set"]["us_per_round"]["best"]
            res.setdefault("%dx%d" % (w, h), {})[str(n)] = row
    return all(r["identical"] for s in res.values() for r in s.values())


def server_rounds(e, ctx, steps, windows, res):
    """the server's GPU calls of one round at 416x240: the step alone, and the step with the paced call behind it (open gates in both)"""
    w, h = SIZES[0]
    nctu = e.ctus_per_frame(w, h)
    for n in (4, 16):
        lum = np.random.default_rng(100 + n).integers(0, 256, size=(n, h, w), dtype=np.uint8)
        ins, outs = [], []
        for j in range(n):
            b = ctx.host_buffer(w * h)
            b[:] = lum[j].reshape(-1)
            ins.append(b.reshape(h, w))
            outs.append(ctx.host_buffer(nctu * 84).view(np.float32))
        with e.LdpSessions(ctx, 1) as s, e.PacerSet(ctx, 32, SHARE, MODE) as pset:
            s.load_lstm_synthetic(0, 22, 3.0)
            ids = [s.open(w, h) for _ in range(n)]
            count = [0]   # (the first step is frame 1: from a zero state)

            def plain_round():
                count[0] += 1
                return s.step([{"session": ids[j], "luma": ins[j], "qp": QP, "i_frame": count[0], "bundle": 0, "probs_out": outs[j]} for j in range(n)])

            def paced_round():
                depths = plain_round()
                pset.frames([{"slot": ids[j], "probs": depths[j], "width": w, "height": h, "out": depths[j]} for j in range(n)])

            for _ in range(5):
                plain_round()
                paced_round()
            ts = {"plain": [], "paced": []}
            for k in range(windows):
                for name in (("plain", "paced") if k % 2 == 0 else ("paced", "plain")):
                    ts[name].append(window(ctx, steps, plain_round if name == "plain" else paced_round))
        ctx.free_host_buffers()
        row = {"plain": {"us_per_round": stats(ts["plain"])}, "paced": {"us_per_round": stats(ts["paced"])}}
        row["paced_minus_plain_us"] = row["paced"]["us_per_round"]["best"] - row["plain"]["us_per_round"]["best"]
        res[str(n)] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pacer_set_rate.json"))
    a = ap.parse_args()
    e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    ctx = e.EthCnn(device=0)
    ctx.load_synthetic(21, 1.0)
    res = {"device": ctx.device_name, "steps": a.steps, "windows": a.windows, "budget": SHARE, "mode": MODE, "sizes": {}, "server_416x240": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = paced_rounds(e, ctx, a.steps, a.windows, res["sizes"])
    with open(a.out, "w") as f:   # (kept even if the second part fails)
        json.dump(res, f, indent=1)
    ctx.set_thresholds(0.0, 0.0)
    server_rounds(e, ctx, max(a.steps // 5, 20), a.windows, res["server_416x240"])
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not ok:
        sys.stderr.write("pacer_set_rate: the two forms differ\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
