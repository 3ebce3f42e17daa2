"""Rates of the partition-search simulator on one MI355X -> profiles/sim_rate.json.  A record, not a gate.

  gpu    the C4 job's geometry -- 4928x3264 (77 x 51 whole CTUs a frame), 425 frames = 1,668,975 CTUs -- with probabilities (140 MB)
         and labels (27 MB) resident in HBM.  Three measurements, each after a warm-up call, one synchronous call per window between
         two synchronisations, best of three: the pack (add_frames_device into an empty set whose memory is already allocated), one
         1026-candidate sweep (down0 around the reference's LDP values, LDP gates) and an evaluation of one candidate.
  numpy  the restatement of the tests (tests/sim_ref.py) over the same arrays on the same box: the one candidate, and every
         --numpy-stride'th candidate of the sweep (the whole sweep would take the restatement tens of minutes); its counters are
         compared with the GPU's for equality and its time is quoted per candidate x CTU.

    python scripts/sim_rate.py [--out profiles/sim_rate.json] [--quick] [--numpy-stride 64]
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


def _best(ctx, fn, before=None):
    fn()  # warm-up: code object, first launch, buffers
    times = []
    for _ in range(3):
        if before:
            before()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return out, min(times), times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_rate.json"))
    ap.add_argument("--quick", action="store_true", help="25 frames (a functional check, not a measurement)")
    ap.add_argument("--numpy-stride", type=int, default=64)
    a = ap.parse_args(argv)
    import sim_ref
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    frames = 25 if a.quick else FRAMES
    nctu = (W // 64) * (H // 64)
    n = frames * nctu
    rng = np.random.default_rng(1)
    probs = rng.random((frames, nctu, 21), dtype=np.float32)
    labels = rng.integers(0, 4, size=(frames, H // 16, W // 16), dtype=np.uint8)
    base = sim_ref.thr((614, 717, 819), (410, 307, 205))  # 0.4 0.6 0.3 0.7 0.2 0.8 on the grid
    res = {"width": W, "height": H, "frames": frames, "ctus": n, "bytes_read_by_pack": int(probs.nbytes + labels.nbytes), "set_bytes": n * 64}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        dp, dl = ctx.alloc(probs.nbytes), ctx.alloc(labels.nbytes)
        dp.upload(probs)
        dl.upload(labels)
        with pkg.PartitionSim(ctx) as sim:
            _, t_pack, all_pack = _best(ctx, lambda: sim.add_frames_device(dp, dl, W, H, frames), before=sim.reset)
            info = sim.info()
            (values, sweep), t_sweep, all_sweep = _best(ctx, lambda: sim.sweep(base, "down0", "ldp"))
            one, t_one, all_one = _best(ctx, lambda: sim.eval(base, "ldp"))
        dp.free()
        dl.free()
    window = "one synchronous call between two synchronisations, best of three, after a warm-up call"
    res["info"] = info
    res["gpu"] = {"window": window,
                  "pack": dict(seconds=t_pack, all_seconds=all_pack, ctus_per_s=n / t_pack, bytes_per_s=(res["bytes_read_by_pack"] + n * 64) / t_pack),
                  "sweep_1026": dict(seconds=t_sweep, all_seconds=all_sweep, candidate_ctus_per_s=values.size * n / t_sweep),
                  "eval_1": dict(seconds=t_one, all_seconds=all_one, candidate_ctus_per_s=n / t_one)}
    s = sim_ref.Set()
    t0 = time.perf_counter()
    s.add_frames(probs, labels, W, H)
    t_ref_pack = time.perf_counter() - t0
    _, cands = s.sweep_candidates(base[()], 0)
    pick = np.arange(0, cands.size, max(1, a.numpy_stride))
    t0 = time.perf_counter()
    want = s.evaluate(cands[pick], sim_ref.GATES_LDP)
    t_ref = time.perf_counter() - t0
    res["numpy"] = dict(pack_seconds=t_ref_pack, candidates=int(pick.size), seconds=t_ref, candidate_ctus_per_s=pick.size * n / t_ref, runs=1,
                        threads=os.environ.get("OMP_NUM_THREADS"))
    same = bool(sim_ref.equal(sweep[pick], want) and sim_ref.equal(one, sweep[values == base["down_k"][0]]) and info == s.info())
    res["identical_counts"] = same
    res["not_measured"] = ["the host entries (they add a pageable upload)", "the per-CTU layout", "the relation of the weighted check count to HM's encoding time",
                           "other GPUs of the pool"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the GPU counters and the numpy restatement disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
