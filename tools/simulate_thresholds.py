#!/usr/bin/env python
"""Simulates what HM's pruned CU search does under a Thr_info.txt, before any encoder run.

HM visits a CU when the decision above it let it through, takes "split only" when p > up[depth], "current only" when p <= down[depth]
and checks both in between (TEncCu.cpp:419-463 of HM-16.5_Test_AI).  This tool evaluates that rule on the GPU over every CTU of the
given predictions (include/ethcnn.h "partition-search simulation") and counts the rate-distortion checks that remain per CU size --
absolutely and as a share of the full search's -- and, with labels, the nodes forced against their label and the CTUs whose labelled
partition the pruned search can no longer reach.

    simulate_thresholds.py MODE [--gates ai|ldp|none] [--weights W64 W32 W16 W8] [--reliability FILE] [--json] [--device N] CASE...

Modes:
  --thr-info FILE --order ai|ldp
        scores one file (its six values are rounded to the grid k / 1024).  Beside the check counts it prints, with or without labels,
        the EXPECTED wrongly split and wrongly stopped nodes per level (include/ethcnn.h "partition-search simulation: expected wrong
        decisions"): a node forced to stop is wrong with its split probability, a node forced to split with the complement.  They
        are counted on the probabilities as given (gates none).  --reliability FILE reads those probabilities from a table that
        calibrate_thresholds.py --reliability-out made from labelled material; the default is the identity, which takes the model
        at its word.
  --sweep COORD [--start FILE --order ai|ldp]
        COORD is down0, up0, down1, up1, down2 or up2: the operating curve over every value of that threshold, the other five as in
        the start file (default: the full search), as CSV.
  --search --max-bad-ppm N [--start FILE] [--max-rounds R] --out Thr_info.txt --order ai|ldp
        coordinate descent over the six thresholds: the least weighted check count whose share of bad CTUs stays within N parts per
        million.  Needs labels.  Starts from the full search unless --start is given.

Cases are those of calibrate_thresholds.py, with labels optional:
  --case LABELS PROBS W H [--skip-label-frames N]     (LABELS may be - for none)
        THE FILE MUST HAVE BEEN PREDICTED WITH OPEN GATES (a Thr_info.txt of zeros / set_thresholds(0, 0)), or --gates none must be
        given: the predictors' batch gates zero whole sub-batches of p32 / p16, and this tool cannot know how a file it is given was
        made.  With --gates none the probabilities are taken as what the encoder will read.
  --yuv SEQ W H QP [--labels L] --model-dir D [--ldp [--frame-begin 1]]
  --samples FILE --model PREFIX --qp Q [--net ai|ldp]
  --samples FILE --ldp --model-dir D --qp Q [--batch]  (an inter sample file replayed through the deployed Low-Delay-P chain; its
        CTUs come as frames, so the gates apply to them as to a --yuv case)

--input-bit-depth N and --input-chroma-format 400|420|422|444 give the source format of the All-Intra --yuv cases, as in
calibrate_thresholds.py (refused without such a case unless they say 8-bit 4:2:0).

--gates defaults to --order: input predicted by this tool has open gates, and the simulator applies the gates that a predictor
reading the candidate file would (tokens [1] and [3]).  CTUs of a --samples case without --ldp belong to no sub-batch and are never gated.
--weights default to 64 16 4 1: cost proportional to the CU's area.

What this is not: the weighted check count is a proxy, and its relation to HM's encoding time or to BD-rate has not been measured; a
"bad CTU" assumes that the full search would return the labelled partition.  The expected wrong decisions are as good as the model's
calibration: the identity table assumes a calibrated model, and the 32x32 and 16x16 probabilities come from a model trained under
teacher forcing.
"""
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("calibrate_thresholds", os.path.join(ROOT, "tools", "calibrate_thresholds.py"))
cal_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cal_tool)
Usage = cal_tool.Usage

COORDS = ("down0", "up0", "down1", "up1", "down2", "up2")
SIZES = ("64x64", "32x32", "16x16", "8x8")


def parse(argv):
    """-> (options, cases): this tool's options are taken out, the cases go through the calibrate tool's parser"""
    opt = {"thr_info": None, "order": None, "sweep": None, "search": False, "max_bad_ppm": None, "start": None, "max_rounds": 16, "out": None,
           "gates": None, "weights": [64, 16, 4, 1], "reliability": None, "json": False, "device": 0}
    rest, i = [], 0
    one = {"--thr-info": ("thr_info", str), "--order": ("order", str), "--sweep": ("sweep", str), "--max-bad-ppm": ("max_bad_ppm", int),
           "--start": ("start", str), "--max-rounds": ("max_rounds", int), "--out": ("out", str), "--gates": ("gates", str), "--device": ("device", int), "--reliability": ("reliability", str)}
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
        elif a == "--search":
            opt["search"] = True
        elif a == "--json":
            opt["json"] = True
        else:
            rest.append(a)
    if (opt["thr_info"] is not None) + (opt["sweep"] is not None) + opt["search"] != 1:
        raise Usage("exactly one of --thr-info FILE, --sweep COORD and --search")
    if opt["order"] not in ("ai", "ldp") and (opt["thr_info"] or opt["start"] or opt["search"]):
        raise Usage("--order ai|ldp says how a Thr_info file is read and written")
    if opt["order"] not in (None, "ai", "ldp"):
        raise Usage("--order is ai or ldp")
    if opt["sweep"] is not None and opt["sweep"] not in COORDS:
        raise Usage("--sweep takes one of %s" % " ".join(COORDS))
    if opt["search"] and (opt["max_bad_ppm"] is None or opt["out"] is None):
        raise Usage("--search needs --max-bad-ppm N and --out PATH")
    if opt["max_bad_ppm"] is not None and not 0 <= opt["max_bad_ppm"] <= 1000000:
        raise Usage("--max-bad-ppm is parts per million, 0..1000000")
    if opt["max_rounds"] < 0 or min(opt["weights"]) < 0:
        raise Usage("--max-rounds and --weights are not negative")
    if opt["gates"] is None:
        opt["gates"] = opt["order"] or "none"
    if opt["gates"] not in ("ai", "ldp", "none"):
        raise Usage("--gates is ai, ldp or none")
    if opt["reliability"] is not None and opt["thr_info"] is None:
        raise Usage("--reliability goes with --thr-info: --sweep and --search do not count expected wrong decisions")
    _, cases = cal_tool.parse(rest, labels_optional=True)
    for c in cases:
        if c["kind"] == "case" and c["labels"] == "-":
            c["labels"] = None
    return opt, cases


def read_thr_info(path, order):
    """six tokens -> (up_k [3], down_k [3]) on the grid: the k with k / 1024 nearest to each value"""
    tok = open(path).read().split()
    if len(tok) < 6:
        raise ValueError("%s: a Thr_info file holds six values" % path)
    k = [int(round(float(t) * 1024)) for t in tok[:6]]
    a, b = k[0::2], k[1::2]
    up, down = (a, b) if order == "ai" else (b, a)
    if min(up) < 0 or max(up) > 1024 or min(down) < -1 or max(down) > 1024:
        raise ValueError("%s: thresholds outside [0, 1] (down: [-1/1024, 1])" % path)
    return up, down


def _share(a, b):
    return float(a) / float(b) if b else 0.0


def report(counts, full, info, weights):
    """one candidate's counters as a dict of plain integers and shares"""
    c = {f: [int(x) for x in np.atleast_1d(counts[f])] for f in counts.dtype.names}
    c["bad_ctus"] = c["bad_ctus"][0]
    cost = sum(w * x for w, x in zip(weights, c["checked"]))
    full_checked = [int(x) for x in full["checked"]]
    full_cost = sum(w * x for w, x in zip(weights, full_checked))
    c.update(checked_share=[_share(x, y) for x, y in zip(c["checked"], full_checked)], full_checked=full_checked, cost=cost, full_cost=full_cost,
             cost_share=_share(cost, full_cost), bad_share=_share(c["bad_ctus"], info["labelled_ctus"]))
    return c


def run(opt, cases, out=sys.stdout, err=sys.stderr):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    note = lambda s: err.write(s + "\n")
    rel = e.risk_read(opt["reliability"]) if opt["reliability"] else None   # (an unreadable table: refused before a GPU is touched)
    start = e.sim_thr(*(read_thr_info(opt["start"], opt["order"]) if opt["start"] else e.SIM_FULL_SEARCH))
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        sim = pkg.PartitionSim(ctx)
        cal_tool.add_cases(pkg, ctx, sim, cases, note)
        info = sim.info()
        full = sim.eval(e.sim_thr(*e.SIM_FULL_SEARCH), "none")[0]
        result = {"info": info, "gates": opt["gates"], "weights": opt["weights"]}
        if opt["sweep"] is not None:
            values, counts = sim.sweep(start, opt["sweep"], opt["gates"])
            rows = [report(c, full, info, opt["weights"]) for c in counts]
            result.update(coord=opt["sweep"], values=[int(v) for v in values], rows=rows)
            if not opt["json"]:
                out.write("k,threshold,checked64,checked32,checked16,checked8,cost,cost_share,bad_ctus,bad_share\n")
                for v, r in zip(values, rows):
                    out.write("%d,%.10f,%d,%d,%d,%d,%d,%.6f,%d,%.6f\n" % ((v, v / 1024.0) + tuple(r["checked"]) + (r["cost"], r["cost_share"], r["bad_ctus"],
                                                                                                                    r["bad_share"])))
        else:
            if opt["search"]:
                thr, counts, rounds = sim.search(start, opt["gates"], opt["weights"], opt["max_bad_ppm"], opt["max_rounds"])
                sim.write_thr_info(opt["out"], thr, opt["order"])
                result.update(rounds=rounds, out=opt["out"], max_bad_ppm=opt["max_bad_ppm"])
            else:
                thr = e.sim_thr(*read_thr_info(opt["thr_info"], opt["order"]))
                counts = sim.eval(thr, opt["gates"])[0]
            r = report(counts, full, info, opt["weights"])
            if not opt["search"]:
                sim.set_reliability(rel)
                risk = sim.eval_risk(thr)[0]
                r.update(exp_wrong_split=[int(x) for x in risk["exp_wrong_split"]], exp_wrong_stop=[int(x) for x in risk["exp_wrong_stop"]],
                         risk_one=e.RISK_ONE, reliability=opt["reliability"] or "identity")
            result.update(up_k=[int(x) for x in thr["up_k"]], down_k=[int(x) for x in thr["down_k"]], order=opt["order"], **r)
    finally:
        ctx.close()
    if opt["json"]:
        out.write(json.dumps(result) + "\n")
        return result
    if opt["sweep"] is not None:
        return result
    out.write("%d CTUs (%d whole, %d labelled, %d rejected, %d sub-batches); gates: %s\n" % (info["ctus"], info["whole_ctus"], info["labelled_ctus"],
                                                                                           info["rejected_ctus"], info["sub_batches"], opt["gates"]))
    out.write("up   %s\ndown %s\n" % (" ".join("%.10f" % (k / 1024.0) for k in result["up_k"]), " ".join("%.10f" % (k / 1024.0) for k in result["down_k"])))
    for d, name in enumerate(SIZES):
        out.write("%-5s  checked %d of %d (%.4f of the full search)\n" % (name, r["checked"][d], r["full_checked"][d], r["checked_share"][d]))
    out.write("weighted checks (weights %s): %d of %d (%.4f of the full search)\n" % (" ".join(str(w) for w in opt["weights"]), r["cost"], r["full_cost"],
                                                                                      r["cost_share"]))
    for d, name in enumerate(SIZES[:3]):
        out.write("%-5s  split only %d  current only %d  both %d  frame edge %d" % (name, r["split_only"][d], r["current_only"][d], r["both"][d],
                                                                                    r["edge_split"][d]))
        if info["labelled_ctus"]:
            out.write("  wrongly split %d  wrongly stopped %d" % (r["wrong_split"][d], r["wrong_stop"][d]))
        out.write("\n")
    if info["labelled_ctus"]:
        out.write("bad CTUs: %d of %d labelled (%.6f)\n" % (r["bad_ctus"], info["labelled_ctus"], r["bad_share"]))
    if "exp_wrong_split" in r:
        counted = info["ctus"] - info["rejected_ctus"]
        for d, name in enumerate(SIZES[:3]):
            out.write("%-5s  expected wrongly split %.3f  expected wrongly stopped %.3f\n" % (name, r["exp_wrong_split"][d] / float(r["risk_one"]),
                                                                                           r["exp_wrong_stop"][d] / float(r["risk_one"])))
        total = sum(r["exp_wrong_split"]) + sum(r["exp_wrong_stop"])
        out.write("expected wrong nodes: %.3f over %d CTUs (%.1f per million CTUs); table: %s; gates: none\n"
                  % (total / float(r["risk_one"]), counted, _share(total * 10 ** 6, counted * r["risk_one"]), r["reliability"]))
    if opt["search"]:
        out.write("search: %d round(s), at most %d ppm bad CTUs; wrote %s (%s order): %s" % (result["rounds"], opt["max_bad_ppm"], opt["out"], opt["order"],
                                                                                           open(opt["out"]).read()))
    return result


def main(argv):
    try:
        opt, cases = parse(list(argv[1:]))
    except (Usage, ValueError) as e:
        sys.stderr.write(__doc__)
        if str(e):
            sys.stderr.write("\nerror: %s\n" % e)
        return 2
    try:
        run(opt, cases)
    except (ValueError, OSError, RuntimeError) as e:  # (libethcnn errors are RuntimeErrors)
        sys.stderr.write("error: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
