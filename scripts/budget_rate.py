"""Rate of the two search-budget kernels on one MI355X -> profiles/budget_rate.json (method: scripts/decide_rate.py).  A record, not a gate.

  copy     the float4 grid-stride copy (ethcnn_bench_copy), re-measured here: a 1 GiB buffer (beyond the 256 MB last-level cache)
           and a 64 MiB one (inside it)
  cost     ethcnn_budget_cost_device with the default ladder (513 rungs + the full search) over the C4 job's geometry -- 4928x3264 (77 x 51
           whole CTUs a frame), 425 frames = 1,668,975 CTUs -- with the set resident in HBM, against ethcnn_sim_eval of the same 513
           candidates over the same set in the same job: the same compares and descents, summed per frame instead of over the set,
           so the ratio is the finding.  After a warm-up, LAUNCHES synchronous calls in one window, best of three windows.
  bake     ethcnn_budget_bake_device over the same set (64 B read, 84 B written per CTU) against the float4 copy rate of the working
           set's size class.
  check    the per-frame counters summed over the frames against ethcnn_sim_eval's checked[0..3], and the baked rows of frame 0 read
           back under the companion thresholds against ethcnn_decide of frame 0's rung

    python scripts/budget_rate.py [--out profiles/budget_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from decide_rate import FRAMES, H, LLC, W, copy_rate, window  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_rate.json"))
    ap.add_argument("--quick", action="store_true", help="25 frames, 3 launches (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    E = pkg.ethcnn
    frames, launches = (25, 3) if a.quick else (FRAMES, 20)
    nctu = (W // 64) * (H // 64)
    n = frames * nctu
    rng = np.random.default_rng(1)
    probs = rng.random((frames, nctu, 21), dtype=np.float32)
    ladder = E.budget_default_ladder()
    k = ladder.size
    rung = rng.integers(0, k, size=frames).astype(np.int32)
    res = {"width": W, "height": H, "frames": frames, "ctus": n, "rungs": k, "gates": "none"}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        copies = [copy_rate(pkg, ctx, (64 << 20) if a.quick else (1 << 30), launches), copy_rate(pkg, ctx, 64 << 20, launches)]
        res["float4_copy"] = copies
        with pkg.PartitionSim(ctx) as sim:
            sim.add_frames(probs, None, W, H)
            d_checked, d_probs = ctx.alloc(frames * (k + 1) * 16), ctx.alloc(n * 84)
            t_cost = window(ctx, lambda: sim.budget_cost_device(ladder, 0, W, H, frames, d_checked), launches)
            t_eval = window(ctx, lambda: sim.eval(ladder, "none"), launches)
            work = n * k
            res["cost"] = dict(kernel="k_budget_cost", ctus_per_launch=n, rungs_counted=k + 1, launches_per_window=launches, windows=3,
                               seconds_per_launch=t_cost, ctu_rungs_per_s=n * (k + 1) / t_cost,
                               sim_eval=dict(kernel="k_sim_eval", candidates=k, seconds_per_call=t_eval, ctu_candidates_per_s=work / t_eval,
                                             note="the host entry: it uploads the candidates and downloads 513 x 184 bytes of counters"),
                               seconds_over_sim_eval=t_cost / t_eval, rate_over_sim_eval=(n * (k + 1) / t_cost) / (work / t_eval),
                               window="synchronous calls (launch + wait each) in one window, best of three")
            t_bake = window(ctx, lambda: sim.budget_bake_device(ladder, rung, 0, W, H, frames, d_probs), launches)
            moved = n * (64 + 84)
            ref = copies[0 if moved > LLC else 1]
            res["bake"] = dict(kernel="k_budget_bake", ctus_per_launch=n, launches_per_window=launches, windows=3, seconds_per_launch=t_bake,
                               ctus_per_s=n / t_bake, bytes_read_plus_written_per_s=moved / t_bake, working_set_bytes=moved,
                               fits_last_level_cache=moved <= LLC, copy_rate_compared=ref["bytes_read_plus_written_per_s"],
                               fraction_of_copy_rate=moved / t_bake / ref["bytes_read_plus_written_per_s"],
                               note="every call also uploads the per-frame thresholds (24 bytes a frame) and waits for them",
                               window="synchronous calls (launch + wait each) in one window, best of three")
            checked = d_checked.download(np.uint32, frames * (k + 1) * 4).reshape(frames, k + 1, 4)
            same = bool(np.array_equal(checked[:, :k].astype(np.uint64).sum(axis=0), sim.eval(ladder, "none")["checked"]))
            baked = d_probs.download(np.float32, nctu * 21).reshape(nctu, 21)
            want = sim.decide(ladder[rung[0]], "none", 512, 0, nctu, want=("codes",))["codes"]
            with pkg.PartitionSim(ctx) as again:
                again.add_frames(baked, None, W, H)
                hinge = bool(np.array_equal(again.decide(E.budget_companion_thr(), "none", want=("codes",))["codes"], want))
            d_checked.free()
            d_probs.free()
    res["identical_counts"], res["hinge_holds_on_frame_0"] = same, hinge
    res["not_measured"] = ["the host forms (they add pageable downloads)", "ethcnn_budget_control end to end", "frames cut into slices (fewer frames than waves)",
                           "other GPUs of the pool"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (same and hinge):
        raise SystemExit("the per-frame counters or the baked rows disagree with the existing kernels")
    return 0


if __name__ == "__main__":
    sys.exit(main())
