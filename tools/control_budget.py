#!/usr/bin/env python
"""Holds a per-frame search budget with an unchanged encoder.

HM reads Thr_info.txt once, so one file sets an average over a sequence and guarantees nothing for a single frame.  But HM's rule only
compares each probability with up and down: a cu_depth.dat that holds 1.0 where a node is to be split only, 0.0 where current only and
0.5 where both, read under the fixed companion file "0.75 0.25 0.75 0.25 0.75 0.25", makes the unchanged encoder carry out any decision.
This tool counts on the GPU, for every frame, the checks that each rung of a ladder of candidate thresholds leaves, picks per frame the
most thorough rung whose weighted checks stay within SHARE of that frame's full search, and writes the picked decisions as such a
cu_depth.dat (include/ethcnn.h "search budget").

    control_budget.py --budget SHARE [--mode frame|carry] [--ladder default|FILE] [--order ai|ldp] [--weights W64 W32 W16 W8]
                      [--out cu_depth.dat] [--thr-out Thr_info.txt] [--per-frame] [--device N] CASE...

  --budget SHARE     0..1, rounded to parts per million.
  --mode             frame (default): every frame on its own.  carry: what a frame leaves of its allowance goes to the next one; the
                     carry starts at 0 with every case and after a frame that is over budget.
  --ladder           default: 513 rungs, rung j = up (1024 - j) / 1024 and down (j - 1) / 1024 on all three levels (rung 0 is the full
                     search).  FILE: one rung per line, six values in --order, the most thorough first (at most 4096).
  --out FILE         the baked cu_depth.dat: float32 [frames][CTUs][21], the cases in the order given (temp file + rename).
  --thr-out FILE     the companion Thr_info.txt in --order: the encoder must read THIS file beside the baked cu_depth.dat.
  --per-frame        CSV on stdout: case, frame, rung, the rung's six grid values, cost, full, share, over_budget; when a case comes
                     with labels also the frame's bad and labelled CTUs under its rung.
  A frame whose cheapest rung is still above the budget takes that rung and is flagged over_budget.

Cases, --weights and --input-bit-depth / --input-chroma-format are those of simulate_thresholds.py, but every case must come as
frames of a picture (--case, --yuv).
Predictions are made with open gates; a --case file is taken as what the encoder would read.  The summary (stderr) gives the achieved
share over the whole input and the number of over-budget frames.

What this is not: the weighted check count is a proxy, and its relation to HM's encoding time or to BD-rate has not been measured.
"""
import importlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("simulate_thresholds", os.path.join(ROOT, "tools", "simulate_thresholds.py"))
sim_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim_tool)
cal_tool = sim_tool.cal_tool
Usage = sim_tool.Usage
_spec = importlib.util.spec_from_file_location("search_budget", os.path.join(ROOT, "hevc-complexity-reduction_amd", "search_budget.py"))
_sb = importlib.util.module_from_spec(_spec)   # (by path: the package itself is imported only when a GPU is about to be used)
_spec.loader.exec_module(_sb)
MAX_RUNGS = _sb.MAX_RUNGS


def read_ladder(path, order):
    """one rung per line, six values in `order` -> (up_k [K][3], down_k [K][3]) on the grid; ValueError names the line (the parser is
    the launchers': hevc-complexity-reduction_amd/search_budget.py)"""
    return _sb.read_ladder(path, order)


def parse(argv):
    """-> (options, cases): this tool's options are taken out, the cases go through the calibrate tool's parser.  Usage: the command
    line's form is wrong; ValueError: a value is (a share, a mode, a ladder file)"""
    opt = {"budget": None, "mode": "frame", "ladder": "default", "order": None, "weights": [64, 16, 4, 1], "out": None, "thr_out": None, "per_frame": False,
           "labels": False, "device": 0}
    one = {"--budget": ("budget", str), "--mode": ("mode", str), "--ladder": ("ladder", str), "--order": ("order", str), "--out": ("out", str),
           "--thr-out": ("thr_out", str), "--device": ("device", int)}
    rest, i = [], 0
    while i < len(argv):
        a = argv[i]
        i += 1
        if a in ("-h", "--help"):
            raise Usage("")
        elif a in one:
            v, i = cal_tool._take(argv, i, 1, a)
            opt[one[a][0]] = one[a][1](v[0])
        elif a == "--weights":
            v, i = cal_tool._take(argv, i, 4, a)
            opt["weights"] = [int(x) for x in v]
        elif a == "--per-frame":
            opt["per_frame"] = True
        else:
            rest.append(a)
    if opt["budget"] is None:
        raise Usage("--budget SHARE says which share of the full search a frame may take")
    if not (opt["out"] or opt["thr_out"] or opt["per_frame"]):
        raise Usage("nothing to do: give --out, --thr-out or --per-frame")
    if opt["order"] not in ("ai", "ldp") and (opt["thr_out"] or opt["ladder"] != "default"):
        raise Usage("--order ai|ldp says how a ladder file is read and the companion file written")
    if opt["order"] not in (None, "ai", "ldp"):
        raise Usage("--order is ai or ldp")
    try:
        share = float(opt["budget"])
    except ValueError:
        share = -1.0
    if not 0.0 <= share <= 1.0:
        raise ValueError("--budget %s is not a share of the full search, 0..1" % opt["budget"])
    opt["budget_ppm"] = int(round(share * 1e6))
    if opt["mode"] not in ("frame", "carry"):
        raise ValueError("--mode %s: the modes are frame and carry" % opt["mode"])
    if min(opt["weights"]) < 0 or max(opt["weights"]) >= 1 << 32:
        raise ValueError("--weights lie in 0..2^32-1")
    opt["rungs"] = None if opt["ladder"] == "default" else read_ladder(opt["ladder"], opt["order"])
    _, cases = cal_tool.parse(rest, labels_optional=True)
    for c in cases:
        if c["kind"] == "case" and c["labels"] == "-":
            c["labels"] = None
        if c["kind"] == "samples":
            raise Usage("a budget is held per frame of a picture: give --case or --yuv cases, not --samples")
        if c.get("labels"):
            opt["labels"] = True
    return opt, cases


def run(opt, cases, out=sys.stdout, err=sys.stderr):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    note = lambda s: err.write(s + "\n")
    ladder = e.budget_default_ladder() if opt["rungs"] is None else e.sim_thr(*opt["rungs"])
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        sim = pkg.PartitionSim(ctx)
        baked, rows = [], []
        cost_sum = full_sum = over_sum = frames_sum = 0
        for k, c in enumerate(cases):
            first = sim.info()["ctus"]
            cal_tool.add_cases(pkg, ctx, sim, [c], note)
            w, h = c["w"], c["h"]
            per = e.ctus_per_frame(w, h)
            nf = (sim.info()["ctus"] - first) // per
            got = sim.budget_control(opt["budget_ppm"] / 1e6, opt["mode"], ladder, opt["weights"], first, w, h, nf, probs=bool(opt["out"]))
            if opt["out"]:
                baked.append(got["probs"])
            cost_sum += sum(int(x) for x in got["cost"])
            full_sum += sum(int(x) for x in got["full"])
            over_sum += int(got["over"].sum())
            frames_sum += nf
            for f in range(nf):
                r = ladder[got["rung"][f]]
                row = [k, f, int(got["rung"][f])] + [int(x) for x in r["up_k"]] + [int(x) for x in r["down_k"]]
                row += [int(got["cost"][f]), int(got["full"][f]), sim_tool._share(int(got["cost"][f]), int(got["full"][f])), int(got["over"][f])]
                if opt["labels"] and opt["per_frame"]:
                    codes = sim.decide(r, "none", 512, first + f * per, per, want=("codes",))["codes"]
                    row += [int(((codes[:, 21] & e.SIM_FLAG_BAD) != 0).sum()), int(((codes[:, 21] & e.SIM_FLAG_LABELLED) != 0).sum())]
                rows.append(row)
        if opt["thr_out"]:
            e.sim_write_thr_info(opt["thr_out"], e.budget_companion_thr(), opt["order"])
    finally:
        ctx.close()
    if opt["out"]:
        tmp = "%s.tmp.%d" % (opt["out"], os.getpid())
        try:
            with open(tmp, "wb") as f:
                for p in baked:
                    f.write(np.ascontiguousarray(p, dtype="<f4").tobytes())
            os.replace(tmp, opt["out"])
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        note("wrote %s: %d CTUs" % (opt["out"], sum(p.shape[0] for p in baked)))
    if opt["thr_out"]:
        note("wrote %s (%s order): %s" % (opt["thr_out"], opt["order"], open(opt["thr_out"]).read().strip()))
    if opt["per_frame"]:
        out.write("case,frame,rung,up0,up1,up2,down0,down1,down2,cost,full,share,over_budget" + (",bad_ctus,labelled_ctus" if opt["labels"] else "") + "\n")
        for r in rows:
            out.write(("%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.6f,%d" + (",%d,%d" if opt["labels"] else "") + "\n") % tuple(r))
    note("budget %.6f (%s): %.6f of the full search over %d frames, %d over budget" % (opt["budget_ppm"] / 1e6, opt["mode"],
                                                                                     sim_tool._share(cost_sum, full_sum), frames_sum, over_sum))
    return {"rows": rows, "cost": cost_sum, "full": full_sum, "over": over_sum, "frames": frames_sum}


def main(argv):
    try:
        opt, cases = parse(list(argv[1:]))
    except Usage as e:
        sys.stderr.write(__doc__)
        if str(e):
            sys.stderr.write("\nerror: %s\n" % e)
        return 2
    except (ValueError, OSError) as e:  # a bad share, mode or ladder file: refused before a GPU is touched
        sys.stderr.write("control_budget.py: error: %s\n" % e)
        return 1
    try:
        run(opt, cases)
    except (ValueError, OSError, RuntimeError) as e:  # (libethcnn errors are RuntimeErrors)
        sys.stderr.write("control_budget.py: error: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
