"""Rate of the expected wrong decisions on one MI355X -> profiles/risk_rate.json.

  set       the C4 geometry of scripts/ladder_rate.py and scripts/sim_rate.py, resident in HBM: 4928x3264 x 425 frames = 1,668,975 CTUs,
            labels uniform in 0..3, probabilities a noisy teacher of them on the grid k / 128.
  eval      PartitionSim.eval_risk (k_sim_risk) against PartitionSim.eval under gates none (k_sim_eval) on the same 1026 candidates, the
            sweep of down0 around the companion thresholds: wall time of the whole call after a warm-up, best of three, in one job.
  step      PartitionSim.build_ladder_risk (k_ladder_step_risk) against PartitionSim.build_ladder (k_ladder_step) for the first 64 rungs
            at grid 8 and at grid 1: wall time of the whole call, best of three, and that time per step, in the same job.
  The two ratios risk / labelled are the findings.

    python scripts/risk_rate.py [--out profiles/risk_rate.json] [--quick]
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("ladder_rate", os.path.join(ROOT, "scripts", "ladder_rate.py"))
ladder_rate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ladder_rate)
RUNGS = ladder_rate.RUNGS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "risk_rate.json"))
    ap.add_argument("--quick", action="store_true", help="a small set: a check of the script, not a measurement")
    args = ap.parse_args()
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    w, h, frames = (4928, 3264, 425) if not args.quick else (1280, 704, 6)
    result = {"device": None, "quick": bool(args.quick), "width": w, "height": h, "frames": frames, "rungs_asked": RUNGS}
    with pkg.EthCnn(device=0) as ctx:
        result["device"] = ctx.device_name
        probs, labels = ladder_rate.make_set(w, h, frames, 7)
        with pkg.PartitionSim(ctx) as sim:
            sim.add_frames(probs, labels, w, h)
            del probs
            info = sim.info()
            result.update(ctus=info["ctus"], labelled_ctus=info["labelled_ctus"])
            cands = np.repeat(e.sim_thr((768, 768, 768), (256, 256, 256)).reshape(1), 1026)
            cands["down_k"][:, 0] = np.arange(-1, 1025)
            sim.eval(cands[:64], "none")   # warm-up
            sim.eval_risk(cands[:64])
            t_eval, counts = ladder_rate.best_of(lambda: sim.eval(cands, "none"))
            t_risk, risk = ladder_rate.best_of(lambda: sim.eval_risk(cands))
            pairs = info["ctus"] * cands.size
            result["eval"] = {"candidates": int(cands.size), "sim_eval_seconds": t_eval, "eval_risk_seconds": t_risk, "eval_risk_over_sim_eval": t_risk / t_eval,
                              "sim_eval_ctu_candidates_per_second": pairs / t_eval, "eval_risk_ctu_candidates_per_second": pairs / t_risk,
                              "last_exp_wrong_stop": [int(x) for x in risk["exp_wrong_stop"][-1]], "last_wrong_stop": [int(x) for x in counts["wrong_stop"][-1]]}
            print("eval", json.dumps(result["eval"]), flush=True)
            result["grids"] = {}
            for grid in (8, 1):
                sim.build_ladder(grid=grid, max_rungs=4)   # warm-up
                sim.build_ladder_risk(grid=grid, max_rungs=4)
                t_lab, lad = ladder_rate.best_of(lambda: sim.build_ladder(grid=grid, max_rungs=RUNGS))
                t_rsk, rlad = ladder_rate.best_of(lambda: sim.build_ladder_risk(grid=grid, max_rungs=RUNGS))
                s_lab, s_rsk = max(len(lad["cost"]) - 1, 1), max(len(rlad["cost"]) - 1, 1)
                result["grids"][str(grid)] = {"labelled_rungs": len(lad["cost"]), "risk_rungs": len(rlad["cost"]), "labelled_seconds_per_step": t_lab / s_lab,
                                              "risk_seconds_per_step": t_rsk / s_rsk, "risk_step_over_labelled_step": (t_rsk / s_rsk) / (t_lab / s_lab),
                                              "risk_last_cost_share": int(rlad["cost"][-1]) / int(rlad["cost"][0])}
                print("grid", grid, json.dumps(result["grids"][str(grid)]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
