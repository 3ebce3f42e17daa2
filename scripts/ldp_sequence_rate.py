#!/usr/bin/env python
"""Per-frame time of a whole Low-Delay-P residual sequence: (a) the per-frame device path (ethcnn_resi_vectors_device +
ethcnn_lstm_step_device in a loop) against (b) ethcnn_ldp_sequence_device, inputs resident in HBM, alternated in one job, one
synchronised host-clock window per measurement, best of three windows with the spread; both outputs compared byte for byte in the
same process.  The split of (b) comes from the context's stage timers (HIP events around the stages).
    python scripts/ldp_sequence_rate.py [--frames 200] [--out profiles/ldp_sequence_rate.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LINK_CYCLES = 45      # measured link of a dependent 16x16x4 chain (profiles/r03_chain_probe.txt)
ISSUE_CYCLES = 32     # a v_mfma_f32_16x16x4_f32 occupies its SIMD's matrix pipe for 32 cycles (64 FLOP / clk / SIMD)
CLOCK_MHZ = 2400.0    # MI355X peak engine clock: the floors below are lower bounds, the real clock under load is lower


def link_counts():
    """levels 64, 32, 16 (N = 64 / 128 / 256 hidden units, N2 = 3 N / 4 fc2 outputs), restated from csrc/ethcnn_lstm_seq.h
    (kLstmSeqChainLinks, kLstmSeqHeadLinks): a gate chain runs over [x, h] = 2 N inputs, four per MFMA; fc2 over N, fc3 over N2"""
    ns = (64, 128, 256)
    return {"chain": [2 * n // 4 for n in ns], "fc2": [n // 4 for n in ns], "fc3": [(3 * n // 4) // 4 for n in ns]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldp_sequence_rate.json"))
    a = ap.parse_args()
    e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    ctx = e.EthCnn(device=0)
    ctx.load_synthetic(21, 1.0)
    ctx.load_lstm_synthetic(22, 3.0)
    ctx.set_thresholds(0.5, 0.5)
    res = {"device": ctx.device_name, "frames": a.frames, "geometries": []}
    rng = np.random.default_rng(1)
    links, ok = link_counts(), True
    chain, fc2, head = links["chain"][2], links["fc2"][2], links["fc2"][2] + links["fc3"][2]
    for (w, h) in ((416, 240), (1920, 1080), (2560, 1600)):
        n, nf = e.ctus_per_frame(w, h), a.frames
        lum = rng.integers(0, 256, size=(nf, h, w), dtype=np.uint8)
        d_l = ctx.alloc(lum.size)
        d_l.upload(lum.reshape(-1))
        d_v, d_s = ctx.alloc(n * 448 * 4), [ctx.alloc(n * 896 * 4), ctx.alloc(n * 896 * 4)]
        d_pa, d_pb = ctx.alloc(nf * n * 21 * 4), ctx.alloc(nf * n * 21 * 4)
        lib, hnd = ctx.lib, ctx.h

        def loop():
            for t in range(nf):
                ctx._chk(lib.ethcnn_resi_vectors_device(hnd, d_l.ptr + t * w * h, w, h, w, d_v.ptr))
                ctx._chk(lib.ethcnn_lstm_step_device(hnd, d_v.ptr, d_s[(t + 1) & 1].ptr if t else None, n, 32, 1 + t, d_s[t & 1].ptr,
                                                     d_pa.ptr + t * n * 21 * 4))

        def seq():
            ctx.ldp_sequence_device(d_l, w, h, nf, 32, 1, d_pb)

        def window(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e6 / nf

        loop(), seq()  # warm-up (allocations, first launches)
        ta, tb = [], []
        for _ in range(3):  # alternated
            ta.append(window(loop))
            tb.append(window(seq))
        pa, pb = d_pa.download(np.uint32, nf * n * 21), d_pb.download(np.uint32, nf * n * 21)
        ctx.set_profiling(2)
        ctx.reset_stage_times()
        seq()
        ctx.synchronize()
        ms = ctx.stage_times()["ms"]
        ctx.set_profiling(0)
        res["geometries"].append({
            "width": w, "height": h, "ctus": n,
            "loop_us_per_frame": {"best": min(ta), "spread": max(ta) - min(ta), "windows": ta},
            "sequence_us_per_frame": {"best": min(tb), "spread": max(tb) - min(tb), "windows": tb},
            "identical": bool(np.array_equal(pa, pb)),
            # HIP events around the stages: tile + trunk + fc1 = front-end passes, heads = the recurrence launch, gate = the post-pass
            "sequence_split_us_per_frame": {"front_end": (ms["tile"] + ms["trunk"] + ms["fc1"]) * 1e3 / nf, "recurrence": ms["heads"] * 1e3 / nf,
                                            "gates": ms["gate"] * 1e3 / nf},
            "recurrence_level16": {
                # one wave = one hidden tile: four interleaved gate chains of `chain` links each, then its fc2 tile (`head` links incl. fc3)
                "chain_links_per_frame": chain, "head_links_per_frame": head, "mfma_per_wave_per_frame": 4 * chain + fc2,
                "latency_floor_us": (chain + head) * LINK_CYCLES / CLOCK_MHZ,              # if the four chains hid each other completely
                "matrix_pipe_floor_us": (4 * chain + fc2) * 4 * ISSUE_CYCLES / CLOCK_MHZ,   # four waves share a SIMD's matrix pipe: the bound
            },
        })
        if not res["geometries"][-1]["identical"]:
            sys.stderr.write("ldp_sequence_rate: %dx%d: the sequence call and the per-frame loop differ\n" % (w, h))
            ok = False
        for b in [d_l, d_v, d_pa, d_pb] + d_s:
            b.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
