#!/usr/bin/env python
"""Builds a ladder for the search budget from labelled predictions.

control_budget.py and the online pacer hold a per-frame budget by picking a rung of a ladder of six-threshold candidates; the default
ladder moves all three levels together and never looks at a label.  This tool walks on the GPU from the full search downwards: every
step moves ONE of the six thresholds to the nearest grid value that lowers the weighted check count, and of the six possible moves it
takes the one that costs the fewest newly bad CTUs per unit of cost saved (include/ethcnn.h "search budget: building a ladder").  The
rungs it writes are read by control_budget.py --ladder FILE and, through ETHCNN_SEARCH_BUDGET_LADDER=FILE, by the launchers.

    build_ladder.py [--grid G] [--max-bad-ppm N] [--weights W64 W32 W16 W8] [--rungs K] [--out FILE --order ai|ldp] [--csv FILE]
                    [--no-labels [--reliability FILE] [--max-risk-ppm N]] [--device N] CASE...

  --grid G           the thresholds move on multiples of G / 1024; a power of two in 1..1024 (default 8).
  --max-bad-ppm N    a move that would leave more than N parts per million of the labelled CTUs bad is not made (default 1000000: no cap).
  --rungs K          thin the path to at most K rungs, evenly spaced in cost; the first and the last rung are kept (default 4096).
  --out FILE         the ladder file: one rung per line, six values in --order, the most thorough first (temp file + rename).
  --csv FILE         one row per rung: the six thresholds, the cost, the share of the full search, the bad CTUs in parts per million of
                     the labelled ones, and the coordinate that moved (- for the first rung; of a thinned ladder: the last move made).
  Without --out and --csv the CSV goes to stdout.
  --no-labels        builds the ladder from the predictions alone: a move is weighed by the EXPECTED wrong decisions it leaves
                     (include/ethcnn.h "partition-search simulation: expected wrong decisions") instead of the bad CTUs; labels that a
                     case carries are not used.  --reliability FILE reads the table of calibrate_thresholds.py --reliability-out
                     (default: the identity, which takes the model at its word); --max-risk-ppm N caps the expected wrong nodes per
                     million CTUs (default: no cap).  The CSV then carries the six expected counts, in nodes, in place of bad_ppm.
                     --max-bad-ppm does not go with it, and the two other options do not go without it.

Cases, --weights and --input-bit-depth / --input-chroma-format are those of simulate_thresholds.py.  WITHOUT --no-labels, LABELS ARE
REQUIRED: at least one case must come with them (a --case with LABELS, a --yuv case with --labels, a --samples case).  Predictions are made with open gates;
a --case file is taken as what the encoder would read.

What this is not: the weighted check count is a proxy, and its relation to HM's encoding time or to BD-rate has not been measured; a
"bad CTU" assumes that the full search would return the labelled partition; the walk is greedy, not optimal.  With --no-labels the
figure is as good as the model's calibration: the identity table assumes a calibrated model, and the 32x32 and 16x16 probabilities
come from a model trained under teacher forcing.
"""
import importlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("simulate_thresholds", os.path.join(ROOT, "tools", "simulate_thresholds.py"))
sim_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim_tool)
cal_tool = sim_tool.cal_tool
Usage = sim_tool.Usage
COORDS = sim_tool.COORDS
MAX_RUNGS = 4096


def parse(argv):
    """-> (options, cases): this tool's options are taken out, the cases go through the calibrate tool's parser.  Usage: the command
    line's form is wrong; ValueError: a value is, or no case carries labels"""
    opt = {"grid": 8, "max_bad_ppm": 10 ** 6, "weights": [64, 16, 4, 1], "rungs": MAX_RUNGS, "out": None, "order": None, "csv": None, "device": 0,
           "no_labels": False, "reliability": None, "max_risk_ppm": None}
    one = {"--grid": ("grid", int), "--max-bad-ppm": ("max_bad_ppm", int), "--rungs": ("rungs", int), "--out": ("out", str), "--order": ("order", str),
           "--csv": ("csv", str), "--device": ("device", int), "--reliability": ("reliability", str), "--max-risk-ppm": ("max_risk_ppm", int)}
    given = set()
    rest, i = [], 0
    while i < len(argv):
        a = argv[i]
        i += 1
        if a in ("-h", "--help"):
            raise Usage("")
        elif a == "--no-labels":
            opt["no_labels"] = True
        elif a in one:
            given.add(a)
            v, i = cal_tool._take(argv, i, 1, a)
            try:
                opt[one[a][0]] = one[a][1](v[0])
            except ValueError:
                raise Usage("%s takes %s" % (a, "an integer" if one[a][1] is int else "a value"))
        elif a == "--weights":
            v, i = cal_tool._take(argv, i, 4, a)
            try:
                opt["weights"] = [int(x) for x in v]
            except ValueError:
                raise Usage("--weights takes four integers")
        else:
            rest.append(a)
    if opt["order"] not in ("ai", "ldp") and opt["out"]:
        raise Usage("--order ai|ldp says how the ladder file is written")
    if opt["order"] not in (None, "ai", "ldp"):
        raise Usage("--order is ai or ldp")
    if not opt["no_labels"] and given & {"--reliability", "--max-risk-ppm"}:
        raise Usage("--reliability and --max-risk-ppm go with --no-labels")
    if opt["no_labels"] and "--max-bad-ppm" in given:
        raise Usage("--max-bad-ppm counts labelled CTUs: with --no-labels the cap is --max-risk-ppm")
    _, cases = cal_tool.parse(rest, labels_optional=True)
    if not cases:
        raise Usage("no case given")
    g = opt["grid"]
    if not (1 <= g <= 1024 and g & (g - 1) == 0):
        raise ValueError("--grid %d is not a power of two in 1..1024" % g)
    if not 0 <= opt["max_bad_ppm"] <= 10 ** 6:
        raise ValueError("--max-bad-ppm is parts per million, 0..1000000")
    if not 1 <= opt["rungs"] <= MAX_RUNGS:
        raise ValueError("--rungs lies in 1..%d" % MAX_RUNGS)
    if min(opt["weights"]) < 0 or max(opt["weights"]) >= 1 << 32:
        raise ValueError("--weights lie in 0..2^32-1")
    if opt["max_risk_ppm"] is not None and not 0 <= opt["max_risk_ppm"] < 1 << 64:
        raise ValueError("--max-risk-ppm is expected wrong nodes per million CTUs, 0..2^64-1")
    labelled = False
    for c in cases:
        if c["kind"] == "case" and c["labels"] == "-":
            c["labels"] = None
        labelled = labelled or c["kind"] == "samples" or bool(c.get("labels"))
    if not labelled and not opt["no_labels"]:
        raise ValueError("a ladder is built from labels: give at least one case with them (--case LABELS ..., --yuv ... --labels L, --samples ...), or say "
                         "--no-labels to build it from the predictions alone")
    return opt, cases


def run(opt, cases, out=sys.stdout, err=sys.stderr):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    note = lambda s: err.write(s + "\n")
    risk = opt["no_labels"]
    rel = e.risk_read(opt["reliability"]) if opt["reliability"] else None   # (an unreadable table: refused before a GPU is touched)
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        sim = pkg.PartitionSim(ctx)
        cal_tool.add_cases(pkg, ctx, sim, cases, note)
        info = sim.info()
        counted = info["ctus"] - info["rejected_ctus"]
        if risk:
            if counted == 0:
                raise ValueError("the cases hold no CTU with valid probabilities")
            sim.set_reliability(rel)
            lad = sim.build_ladder_risk(opt["weights"], opt["grid"], MAX_RUNGS, 2 ** 64 - 1 if opt["max_risk_ppm"] is None else opt["max_risk_ppm"])
        else:
            if info["labelled_ctus"] == 0:
                raise ValueError("the cases hold no labelled CTU (labels count on whole CTUs with valid probabilities only)")
            lad = sim.build_ladder(opt["weights"], opt["grid"], MAX_RUNGS, opt["max_bad_ppm"])
    finally:
        ctx.close()
    built = len(lad["cost"])
    keep = e.ladder_thin(lad["cost"], opt["rungs"])
    lad = {k: v[keep] for k, v in lad.items()}
    full = int(lad["cost"][0])
    rows = []
    for i in range(len(keep)):
        t = lad["thr"][i]
        if risk:   # the six expected counts, in nodes
            harm = [int(x) / float(e.RISK_ONE) for x in lad["exp_wrong_split"][i]] + [int(x) / float(e.RISK_ONE) for x in lad["exp_wrong_stop"][i]]
        else:
            harm = [int(lad["bad_ctus"][i]) * 10 ** 6 / float(info["labelled_ctus"])]
        rows.append([int(x) for x in t["up_k"]] + [int(x) for x in t["down_k"]] + [int(lad["cost"][i]), sim_tool._share(int(lad["cost"][i]), full)] + harm +
                    [COORDS[int(lad["coord"][i])] if lad["coord"][i] >= 0 else "-"])
    if opt["out"]:
        e.ladder_write(opt["out"], lad["thr"], opt["order"])
        note("wrote %s (%s order): %d rungs" % (opt["out"], opt["order"], len(keep)))
    if risk:
        head = "up0,up1,up2,down0,down1,down2,cost,share,exp_wrong_split0,exp_wrong_split1,exp_wrong_split2,exp_wrong_stop0,exp_wrong_stop1,exp_wrong_stop2,moved\n"
        line = "%d,%d,%d,%d,%d,%d,%d,%.6f,%.3f,%.3f,%.3f,%.3f,%.3f,%.3f,%s\n"
    else:
        head, line = "up0,up1,up2,down0,down1,down2,cost,share,bad_ppm,moved\n", "%d,%d,%d,%d,%d,%d,%d,%.6f,%.1f,%s\n"
    text = head + "".join(line % tuple(r) for r in rows)
    if opt["csv"]:
        tmp = "%s.tmp.%d" % (opt["csv"], os.getpid())
        try:
            with open(tmp, "w") as f:
                f.write(text)
            os.replace(tmp, opt["csv"])
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        note("wrote %s" % opt["csv"])
    elif not opt["out"]:
        out.write(text)
    if risk:
        last = int(lad["risk"][-1])
        note("ladder: %d rungs built on grid %d over %d CTUs without labels (table: %s), %d kept; the last takes %.6f of the full search with %.1f expected "
             "wrong nodes per million CTUs" % (built, opt["grid"], counted, opt["reliability"] or "identity", len(keep), rows[-1][7],
                                               sim_tool._share(last * 10 ** 6, counted * e.RISK_ONE)))
    else:
        note("ladder: %d rungs built on grid %d over %d labelled CTUs, %d kept; the last takes %.6f of the full search with %.1f ppm bad CTUs"
             % (built, opt["grid"], info["labelled_ctus"], len(keep), rows[-1][7], rows[-1][8]))
    return {"rows": rows, "built": built, "kept": [int(i) for i in keep], "thr": lad["thr"]}


def main(argv):
    try:
        opt, cases = parse(list(argv[1:]))
    except Usage as e:
        sys.stderr.write(__doc__)
        if str(e):
            sys.stderr.write("\nerror: %s\n" % e)
        return 2
    except (ValueError, OSError) as e:  # a bad grid, cap or weight, or no labels: refused before a GPU is touched
        sys.stderr.write("build_ladder.py: error: %s\n" % e)
        return 1
    try:
        run(opt, cases)
    except (ValueError, OSError, RuntimeError) as e:  # (libethcnn errors are RuntimeErrors)
        sys.stderr.write("build_ladder.py: error: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
