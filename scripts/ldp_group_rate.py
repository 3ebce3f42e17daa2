#!/usr/bin/env python
"""Time per member-frame of K Low-Delay-P residual sequences, three ways, alternated in one job (the method of
scripts/ldp_sequence_rate.py: inputs resident in HBM, one synchronised host-clock window per measurement, best of three windows with
the spread):
  group          one LdpGroup.sequence_device call for the K members
  solo_reload    K ethcnn_ldp_sequence_device calls back to back, each after loading its member's bundle into the context (what a
                 user of one context has to do today); solo: the same K calls with the bundle left as it is
  loops          K per-frame loops (ethcnn_resi_vectors_device + ethcnn_lstm_step_device), the bundle left as it is
The outputs of `group` are compared byte for byte with those of `solo_reload` (every member) and with the loop of the member whose
bundle is loaded (the last).  The recurrence share comes from the context's stage timers (HIP events around the stages).
    python scripts/ldp_group_rate.py [--frames 200] [--out profiles/ldp_group_rate.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 2, 4, 8)
QPS = (22, 27, 32, 37, 24, 29, 34, 39)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldp_group_rate.json"))
    a = ap.parse_args()
    e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    ctx = e.EthCnn(device=0)
    ctx.load_synthetic(21, 1.0)
    ctx.set_thresholds(0.5, 0.5)
    blobs = []
    for m in range(max(KS)):
        ctx.load_lstm_synthetic(22 + m, 3.0)
        blobs.append(ctx.get_lstm_blob())
    res = {"device": ctx.device_name, "frames": a.frames, "geometries": []}
    rng = np.random.default_rng(1)
    ok, nf = True, a.frames
    lib, hnd = ctx.lib, ctx.h
    for (w, h) in ((416, 240), (1920, 1080), (2560, 1600)):
        n, kmax = e.ctus_per_frame(w, h), max(KS)
        # one pool of frames: member m reads frames m .. m + nf - 1 of it
        lum = rng.integers(0, 256, size=(nf + kmax - 1, h, w), dtype=np.uint8)
        d_l = ctx.alloc(lum.size)
        d_l.upload(lum.reshape(-1))
        del lum
        pbytes = nf * n * 21 * 4
        d_v, d_s = ctx.alloc(n * 448 * 4), [ctx.alloc(n * 896 * 4), ctx.alloc(n * 896 * 4)]
        d_pg, d_ps = [ctx.alloc(pbytes) for _ in range(kmax)], [ctx.alloc(pbytes) for _ in range(kmax)]
        d_pl = ctx.alloc(pbytes)
        geo = {"width": w, "height": h, "ctus": n, "k": []}
        for k in KS:
            lumas = [d_l.ptr + m * w * h for m in range(k)]
            group = e.LdpGroup(ctx, k)
            for m in range(k):
                group.load_lstm_blob(m, blobs[m])

            def run_group():
                group.sequence_device(lumas, w, h, nf, QPS[:k], 1, d_pg[:k])

            def run_solo(reload):
                for m in range(k):
                    if reload:
                        ctx.load_lstm_blob(blobs[m])
                    ctx.ldp_sequence_device(lumas[m], w, h, nf, QPS[m], 1, d_ps[m])

            def run_loops():
                for m in range(k):
                    for t in range(nf):
                        ctx._chk(lib.ethcnn_resi_vectors_device(hnd, lumas[m] + t * w * h, w, h, w, d_v.ptr))
                        ctx._chk(lib.ethcnn_lstm_step_device(hnd, d_v.ptr, d_s[(t + 1) & 1].ptr if t else None, n, QPS[m], 1 + t, d_s[t & 1].ptr,
                                                             d_pl.ptr + t * n * 21 * 4))

            def window(fn):
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / (nf * k)

            forms = {"group": run_group, "solo_reload": lambda: run_solo(True), "solo": lambda: run_solo(False), "loops": run_loops}
            for fn in forms.values():  # warm-up (allocations, first launches); leaves the bundle of member k - 1 loaded
                fn()
            run_solo(True)
            times = {name: [] for name in forms}
            for _ in range(3):  # alternated
                for name in ("group", "solo_reload", "solo", "loops"):
                    times[name].append(window(forms[name]))
            # identity: every member against its solo call; the last member's bundle is loaded, and the loops end with that member
            run_solo(True)
            ctx.synchronize()
            same = all(np.array_equal(d_pg[m].download(np.uint32, nf * n * 21), d_ps[m].download(np.uint32, nf * n * 21)) for m in range(k))
            same_loop = bool(np.array_equal(d_pg[k - 1].download(np.uint32, nf * n * 21), d_pl.download(np.uint32, nf * n * 21)))
            split = {}
            for name in ("group", "solo"):
                ctx.set_profiling(2)
                ctx.reset_stage_times()
                forms[name]()
                ctx.synchronize()
                ms = ctx.stage_times()["ms"]
                ctx.set_profiling(0)
                split[name] = {"front_end": (ms["tile"] + ms["trunk"] + ms["fc1"]) * 1e3 / (nf * k), "recurrence": ms["heads"] * 1e3 / (nf * k),
                               "gates": ms["gate"] * 1e3 / (nf * k)}
            entry = {"k": k, "identical_to_solo": bool(same), "identical_to_loop": same_loop, "split_us_per_member_frame": split,
                     "recurrence_blocks": k * ((n + 15) // 16 + ((n + 15) // 16 + 1) // 2 + ((n + 15) // 16 + 3) // 4)}
            for name, ts in times.items():
                entry[name + "_us_per_member_frame"] = {"best": min(ts), "spread": max(ts) - min(ts), "windows": ts}
            geo["k"].append(entry)
            if not (same and same_loop):
                sys.stderr.write("ldp_group_rate: %dx%d, K = %d: the forms differ\n" % (w, h, k))
                ok = False
            group.close()
        res["geometries"].append(geo)
        for b in [d_l, d_v, d_pl] + d_s + d_pg + d_ps:
            b.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
