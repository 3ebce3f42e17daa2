#!/usr/bin/env python
"""Calibrates Thr_info.txt -- the upper / lower threshold of each of the three partition levels -- from labelled predictions.

HM takes "split only" when p > up[depth] and "current only" when p <= down[depth] and runs the full rate-distortion search in
between, so the six values decide both how often the encoder is forced into a wrong partition and how much of the search it still
runs.  This tool counts, on the GPU, where the probabilities of truly split and truly unsplit CTUs / 32x32 / 16x16 blocks fall
(1025 bins per level and truth: include/ethcnn.h "threshold calibration"; truth as in tools/score_cu_depth.py) and picks, per level,
the largest `down` that wrongly stops at most --eps-down parts per million of the truly split samples and the smallest `up` that
wrongly forces at most --eps-up parts per million of the truly unsplit ones.

    calibrate_thresholds.py [--eps-down E1 E2 E3] [--eps-up E1 E2 E3] [--out Thr_info.txt --order ai|ldp] [--hist FILE] [--reliability-out FILE] [--json] [--device N]
                            [--reached [--gates none|ai|ldp]] [--input-bit-depth N] [--input-chroma-format 400|420|422|444] CASE...

Any number of cases, accumulated into one histogram:

  --case LABELS PROBS W H [--skip-label-frames N]
        the scorer's inputs: an Info_*_CUDepth.dat and a cu_depth.dat (float32 [frames][ctus][21]).  THE FILE MUST HAVE BEEN
        PREDICTED WITH OPEN GATES (a Thr_info.txt of zeros / set_thresholds(0, 0)): the predictors' batch gates zero whole
        sub-batches of p32 / p16, and this tool cannot know how a file it is given was made.
  --yuv SEQ W H QP --labels L --model-dir D [--ldp [--frame-begin 1]]
        predicts SEQ itself, gates open, into a temporary file and adds it.  All-Intra: D holds the model_2000000_qpXX~YY.dat of
        the QP band.  --ldp: SEQ is a residual file (frame k = POC k), D holds model_LDP_2000000_qp22~37.dat and the
        model_LDP_200000_qpXX.dat of the band; frames [frame-begin, end) are predicted and as many label frames passed over.
  --samples FILE --model PREFIX --qp Q [--net ai|ldp]
        a trainer's evaluation (forward only, no gates in that graph) of a validation sample file with the checkpoint PREFIX; the
        truth is the 16 label bytes of QP row Q (All-Intra records: byte 4160 + 16 Q) or of the slot whose QP byte is Q (LDP records).
  --samples FILE --ldp --model-dir D --qp Q [--batch]
        an inter sample file (LDP_Valid.dat, LDP_Test.dat, plain or _shuffled) replayed through the deployed Low-Delay-P chain
        (include/ethcnn.h "sample-set replay"): the residual pictures and label planes of every sequence the file holds are put back
        together on the GPU, in any record order, and predicted as the daemon would, gates open, with the models of D (as for --yuv
        --ldp).  Q selects the QP slot; a file without a slot of that QP is an error.  One line per sequence goes to stderr.
        --batch sends the sequences of the file through the chain together, up to 32 at a time in one recurrence launch per chunk
        (include/ethcnn.h "config #5 offline, batch form"); the output is the same, byte for byte.

--input-bit-depth (8..16; above 8 the file holds 16-bit little-endian samples) and --input-chroma-format give the source format of
the All-Intra --yuv cases of the run (include/ethcnn.h "high-bit-depth and non-4:2:0 sources"); --ldp cases read HM's residual files,
which are always 8-bit 4:2:0, and --case / --samples cases carry no video.  A format other than 8-bit 4:2:0 without an All-Intra
--yuv case is an error.

Budgets default to 50000 ppm (5 %).  --hist FILE also writes the accumulated histogram, uint64 little-endian [3 levels][2 truths][1025 bins].
--reliability-out FILE writes the reliability table of that histogram (include/ethcnn.h "partition-search simulation: expected wrong
decisions": per level and bin the share of truly split samples, made non-decreasing), which simulate_thresholds.py --reliability,
build_ladder.py --no-labels --reliability and ETHCNN_SEARCH_BUDGET_RELIABILITY read.  --order ai writes "up1 down1 up2 down2 up3 down3" (HM-16.5_Test_AI, TEncCu.cpp:250), --order
ldp writes "down1 up1 down2 up2 down3 up3" (HM-16.5_Test_LDP, TEncGOP.cpp:1449): the two encoders differ.  CTUs that are not wholly
inside the picture are left out (HM forces their splits).

--reached calibrates on the nodes HM's pruned search REACHES instead (include/ethcnn.h "threshold calibration on reached nodes").  The
populations above are teacher-forced: a 32x32 block counts only under a CTU that is labelled split, a 16x16 block only when both
ancestors are.  The encoder visits a block whenever the decision above it was "split only", "both" or a frame edge, whatever the label
says.  With --reached the cases go into a partition-search simulator and the levels are chosen top-down: 64x64 first, then 32x32 on the
blocks reached under the chosen 64x64 thresholds, then 16x16; the budgets are shares of the reached split / unsplit nodes, and the
report adds the RD checks that remain per CU size and their weighted share (weights 64 16 4 1) of the full search.  --gates none|ai|ldp
applies the predictors' batch gates as simulate_thresholds.py does; it defaults to --order's value when --out is given, else none.
--hist and --reliability-out then take the histogram of the full search under gates none: every node of every labelled CTU.
"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDP_CNN_FILE = "model_LDP_2000000_qp22~37.dat"
DEFAULT_FORMAT = (8, 420)


class Usage(Exception):
    pass


def _take(argv, i, n, what):
    if i + n > len(argv):
        raise Usage("%s takes %d value(s)" % (what, n))
    return argv[i:i + n], i + n


def parse(argv, labels_optional=False):
    """-> (options, cases); the options after a case belong to it.  labels_optional: a --yuv case may come without --labels (the
    simulation tool, which shares this command line's cases)"""
    opt = {"eps_down": [50000] * 3, "eps_up": [50000] * 3, "out": None, "order": None, "hist": None, "reliability_out": None, "json": False, "device": 0}
    cases, i = [], 0
    fmt = {"--input-bit-depth": DEFAULT_FORMAT[0], "--input-chroma-format": DEFAULT_FORMAT[1]}
    per_case = {"--skip-label-frames": ("skip", int, ("case",)), "--labels": ("labels", str, ("yuv",)), "--model-dir": ("model_dir", str, ("yuv", "samples")),
                "--frame-begin": ("frame_begin", int, ("yuv",)), "--model": ("model", str, ("samples",)), "--qp": ("qp", int, ("samples",)),
                "--net": ("net", str, ("samples",))}
    while i < len(argv):
        a = argv[i]
        i += 1
        if a in ("-h", "--help"):
            raise Usage("")
        elif a in ("--eps-down", "--eps-up"):
            v, i = _take(argv, i, 3, a)
            opt[a[2:].replace("-", "_")] = [int(x) for x in v]
        elif a in ("--out", "--order", "--hist", "--reliability-out", "--device"):
            v, i = _take(argv, i, 1, a)
            opt[a[2:].replace("-", "_")] = int(v[0]) if a == "--device" else v[0]
        elif a == "--json":
            opt["json"] = True
        elif a == "--reached":
            opt["reached"] = True
        elif a == "--gates":
            v, i = _take(argv, i, 1, a)
            opt["gates"] = v[0]
        elif a in fmt:
            v, i = _take(argv, i, 1, a)
            if not v[0].isdigit():
                raise Usage("%s takes a number" % a)
            fmt[a] = int(v[0])
        elif a == "--case":
            v, i = _take(argv, i, 4, a)
            cases.append({"kind": "case", "labels": v[0], "probs": v[1], "w": int(v[2]), "h": int(v[3]), "skip": 0})
        elif a == "--yuv":
            v, i = _take(argv, i, 4, a)
            cases.append({"kind": "yuv", "yuv": v[0], "w": int(v[1]), "h": int(v[2]), "qp": int(v[3]), "ldp": False, "frame_begin": 1})
        elif a == "--samples":
            v, i = _take(argv, i, 1, a)
            cases.append({"kind": "samples", "file": v[0], "net": "ai", "ldp": False})
        elif a == "--ldp":
            if not cases or cases[-1]["kind"] not in ("yuv", "samples"):
                raise Usage("--ldp follows a --yuv or a --samples case")
            cases[-1]["ldp"] = True
        elif a == "--batch":
            if not cases or cases[-1]["kind"] != "samples" or not cases[-1]["ldp"]:
                raise Usage("--batch follows a --samples FILE --ldp case")
            cases[-1]["batch"] = True
        elif a in per_case:
            key, conv, kinds = per_case[a]
            if not cases or cases[-1]["kind"] not in kinds:
                raise Usage("%s follows a --%s case" % (a, kinds[0]))
            v, i = _take(argv, i, 1, a)
            cases[-1][key] = conv(v[0])
        else:
            raise Usage("unknown argument %r" % a)
    if not cases:
        raise Usage("no case given")
    for c in cases:
        need = {"case": (), "yuv": ("model_dir",) if labels_optional else ("labels", "model_dir"),
                "samples": ("model_dir", "qp") if c.get("ldp") else ("model", "qp")}[c["kind"]]
        for k in need:
            if k not in c:
                raise Usage("a --%s case needs --%s" % (c["kind"], k.replace("_", "-")))
        if c["kind"] == "samples" and c["net"] not in ("ai", "ldp"):
            raise Usage("--net is ai or ldp")
        if c["kind"] == "samples" and (("model" in c or c["net"] != "ai") if c["ldp"] else "model_dir" in c):
            raise Usage("a --samples case takes --model PREFIX [--net], or --ldp --model-dir D (a replay)")
    # the source format of the run's All-Intra --yuv cases (checked here, before a GPU is touched; add_cases sets it on the context)
    opt["source_format"] = (fmt["--input-bit-depth"], fmt["--input-chroma-format"])
    if not 8 <= opt["source_format"][0] <= 16:
        raise Usage("--input-bit-depth is 8..16")
    if opt["source_format"][1] not in (400, 420, 422, 444):
        raise Usage("--input-chroma-format is 400, 420, 422 or 444")
    video = [c for c in cases if c["kind"] == "yuv" and not c["ldp"]]
    if opt["source_format"] != DEFAULT_FORMAT and not video:
        raise Usage("--input-bit-depth / --input-chroma-format describe All-Intra --yuv sources, and none is given "
                    "(--ldp residual files are always 8-bit 4:2:0; --case and --samples carry no video)")
    for c in video:
        c["source_format"] = opt["source_format"]
    if (opt["out"] is None) != (opt["order"] is None) or opt["order"] not in (None, "ai", "ldp"):
        raise Usage("--out PATH and --order ai|ldp go together")
    for e in opt["eps_down"] + opt["eps_up"]:
        if not 0 <= e <= 1000000:
            raise Usage("budgets are parts per million, 0..1000000")
    if "gates" in opt and not opt.get("reached"):
        raise Usage("--gates goes with --reached")
    if opt.get("reached"):  # (a run without --reached carries neither key)
        opt.setdefault("gates", opt["order"] if opt["out"] else "none")
        if opt["gates"] not in ("none", "ai", "ldp"):
            raise Usage("--gates is none, ai or ldp")
    return opt, cases


def _label_frames(path, w, h):
    per = (w // 16) * (h // 16)
    lab = np.fromfile(path, dtype=np.uint8)
    if w % 16 or h % 16 or lab.size % per:
        raise ValueError("%s: %d bytes is not a whole number of %dx%d label frames" % (path, lab.size, w, h))
    return lab, lab.size // per


def _add_file_pair(cal, pkg, labels_path, probs_path, w, h, skip, note):
    """labels_path None (the simulation tool only): every predicted frame, without labels"""
    probs = np.fromfile(probs_path, dtype="<f4")
    per = pkg.ethcnn.ctus_per_frame(w, h) * 21
    if probs.size % per:
        raise ValueError("%s: %d floats is not a whole number of %dx%d frames" % (probs_path, probs.size, w, h))
    pf = probs.size // per
    if labels_path is None:
        cal.add_frames(probs, None, w, h, nframes=pf)
        return pf
    lab, lf = _label_frames(labels_path, w, h)
    if skip >= lf:
        raise ValueError("--skip-label-frames %d: the label file holds %d frames" % (skip, lf))
    n = min(lf - skip, pf)
    if lf - skip != pf:
        note("note: %d labelled frames, %d predicted frames: using the first %d" % (lf - skip, pf, n))
    cal.add_frames(probs[:n * per], lab, w, h, skip_label_frames=skip, nframes=n)
    return n


def _sample_labels(records, net, qp, pkg):
    """uint8 file bytes -> (nrecords, depth16 uint8 [n,16]) for the label row / slot of QP qp"""
    e = pkg.ethcnn
    if net == "ai":
        if records.size == 0 or records.size % e.TRAIN_REC:
            raise ValueError("%d bytes is not a whole number of %d-byte All-Intra records" % (records.size, e.TRAIN_REC))
        if not 0 <= qp <= 51:
            raise ValueError("QP %d outside 0..51" % qp)
        rec = records.reshape(-1, e.TRAIN_REC)
        return rec.shape[0], np.ascontiguousarray(rec[:, 4160 + 16 * qp: 4176 + 16 * qp])
    if records.size == 0 or records.size % e.LDP_REC:
        raise ValueError("%d bytes is not a whole number of %d-byte LDP records" % (records.size, e.LDP_REC))
    rec = records.reshape(-1, e.LDP_REC)
    slot_qps = [int(rec[0, e.LDP_SLOT_BASE + e.LDP_SLOT_BYTES * s]) for s in range(4)]
    if qp not in slot_qps:
        raise ValueError("QP %d is not one of the file's slot QPs %s" % (qp, slot_qps))
    at = e.LDP_SLOT_BASE + e.LDP_SLOT_BYTES * slot_qps.index(qp) + 1
    return rec.shape[0], np.ascontiguousarray(rec[:, at: at + 16])


def add_cases(pkg, ctx, cal, cases, note):
    """feeds every case into `cal`: a Calibrator, or anything with its add / add_frames (the simulation tool's PartitionSim)"""
    for c in cases:
        if c["kind"] == "case":
            _add_file_pair(cal, pkg, c["labels"], c["probs"], c["w"], c["h"], c["skip"], note)
        elif c["kind"] == "yuv":
            w, h, qp, d = c["w"], c["h"], c["qp"], c["model_dir"]
            with tempfile.TemporaryDirectory() as tmp:
                dat = os.path.join(tmp, "cu_depth.dat")
                if c["ldp"]:
                    ctx.load_checkpoint(os.path.join(d, LDP_CNN_FILE))
                    ctx.load_lstm_checkpoint(os.path.join(d, pkg.ethcnn.lstm_model_name_for_qp(qp)))
                    ctx.set_thresholds(0.0, 0.0)  # open gates
                    ctx.set_source_format(*DEFAULT_FORMAT)  # (the Low-Delay-P entries do not read it; nothing deep is left in force)
                    frames = os.path.getsize(c["yuv"]) // (w * h * 3 // 2)
                    ctx.ldp_predict_yuv_file(c["yuv"], w, h, qp, dat, c["frame_begin"], frames)
                    skip = c["frame_begin"]
                else:
                    ctx.load_checkpoint(os.path.join(d, pkg.ethcnn.model_name_for_qp(qp)))
                    ctx.set_thresholds(0.0, 0.0)  # open gates
                    ctx.set_source_format(*c.get("source_format", DEFAULT_FORMAT))
                    try:
                        ctx.predict_yuv_file(c["yuv"], w, h, qp, dat)
                    finally:
                        ctx.set_source_format(*DEFAULT_FORMAT)
                    skip = 0
                _add_file_pair(cal, pkg, c.get("labels"), dat, w, h, skip, note)
        elif c["ldp"]:
            qp, d = c["qp"], c["model_dir"]
            ctx.load_checkpoint(os.path.join(d, LDP_CNN_FILE))
            ctx.load_lstm_checkpoint(os.path.join(d, pkg.ethcnn.lstm_model_name_for_qp(qp)))
            ctx.set_thresholds(0.0, 0.0)  # open gates
            with pkg.Replay(ctx) as rp:
                rp.open(c["file"])
                runs = rp.runs()
                for r in runs:
                    if qp not in r["qps"]:
                        raise ValueError("%s: QP %d is not one of the slot QPs %s of sequence %d" % (c["file"], qp, r["qps"], r["seq"]))
                for r in runs:
                    note("sequence %d: %dx%d (%d x %d whole CTUs), frames %d..%d, %d CTUs" % (r["seq"], r["w"], r["h"], r["cols"], r["rows"], r["f0"],
                                                                                            r["f0"] + r["frames"] - 1, r["frames"] * r["nctu"]))
                if c.get("batch"):  # the sequences of the file together, one recurrence launch per chunk: the same counts
                    with pkg.LdpBatch(ctx, 1) as batch:
                        batch.load_lstm_blob(0, ctx.get_lstm_blob())
                        rp.feed(cal, qp=qp, batch=batch)
                else:
                    rp.feed(cal, qp=qp)
        else:
            records = np.fromfile(c["file"], dtype=np.uint8)
            n, depth = _sample_labels(records, c["net"], c["qp"], pkg)
            with pkg.Trainer(ctx, batch=1, dropout=False, net=c["net"]) as tr:
                tr.set_blob(pkg.ethcnn.read_ckpt_blob(c["model"]))
                tr.set_samples(pkg.ethcnn.SET_VALID, records)
                probs = tr.evaluate(pkg.ethcnn.SET_VALID, c["qp"], n=n, want_probs=True)[2]
            cal.add(probs, depth)


def run_reached(pkg, opt, cases, out, note):
    """--reached: the cases go into a PartitionSim, the levels are chosen top-down on the nodes the pruned search reaches"""
    e = pkg.ethcnn
    sizes, weights = ("64x64", "32x32", "16x16", "8x8"), e.BUDGET_WEIGHTS
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        sim = pkg.PartitionSim(ctx)
        add_cases(pkg, ctx, sim, cases, note)
        info = sim.info()
        if info["labelled_ctus"] == 0:
            raise ValueError("no labelled CTU among the %d of the cases (labels are used on CTUs wholly inside the picture)" % info["ctus"])
        rep, thr, counts = sim.calibrate_reached(opt["eps_down"], opt["eps_up"], opt["gates"])
        levels = rep.as_dicts()
        full = sim.eval(e.sim_thr(*e.SIM_FULL_SEARCH), opt["gates"])[0]
        if opt["out"]:
            e.write_thr_info(opt["out"], rep, opt["order"])
        if opt["hist"] or opt["reliability_out"]:
            hist = sim.reach_hist(e.sim_thr(*e.SIM_FULL_SEARCH), "none")[0]  # every node of every labelled CTU
            if opt["hist"]:
                hist.astype("<u8").tofile(opt["hist"])
            if opt["reliability_out"]:
                e.risk_write(opt["reliability_out"], e.risk_from_hist(hist))
                note("wrote %s: the reliability table of %d reached nodes (full search, gates none)" % (opt["reliability_out"], int(hist.sum())))
    finally:
        ctx.close()
    cost = lambda c: sum(w * int(x) for w, x in zip(weights, c["checked"]))
    share = cost(counts) / cost(full) if cost(full) else 0.0
    result = {"levels": levels, "eps_down_ppm": opt["eps_down"], "eps_up_ppm": opt["eps_up"], "out": opt["out"], "order": opt["order"], "reached": True,
              "gates": opt["gates"], "thr": {"up_k": [int(x) for x in thr["up_k"]], "down_k": [int(x) for x in thr["down_k"]]},
              "counts": {f: [int(x) for x in np.atleast_1d(counts[f])] for f in e.SIM_COUNTS.names}, "checked_full": [int(x) for x in full["checked"]],
              "share_of_full_search": share, "ctus": info["ctus"], "labelled_ctus": info["labelled_ctus"], "rejected_ctus": info["rejected_ctus"]}
    if opt["json"]:
        out.write(json.dumps(result) + "\n")
        return result
    out.write("reached nodes of %d labelled CTUs (of %d; %d rejected), gates %s\n" % (info["labelled_ctus"], info["ctus"], info["rejected_ctus"], opt["gates"]))
    for name, lv, ed, eu in zip(sizes, levels, opt["eps_down"], opt["eps_up"]):
        out.write("%s  reached unsplit %d  reached split %d%s%s\n" % (name, lv["n0"], lv["n1"], "  EMPTY CLASS" if lv["empty_class"] else "",
                                                                    "  CROSSED (one threshold for both)" if lv["crossed"] else ""))
        out.write("    down %.10f (k %d)  wrongly stopped %d of %d split (budget %d ppm)\n" % (lv["down"], lv["down_k"], lv["miss"], lv["n1"], ed))
        out.write("    up   %.10f (k %d)  wrongly forced  %d of %d unsplit (budget %d ppm)\n" % (lv["up"], lv["up_k"], lv["fsplit"], lv["n0"], eu))
        out.write("    full search remains for %d (%.4f); accuracy at 0.5: %.4f\n" % (lv["uncertain"], lv["uncertain_share"], lv["accuracy_512"]))
    for d, name in enumerate(sizes):
        out.write("%-5s  checked %d of %d\n" % (name, int(counts["checked"][d]), int(full["checked"][d])))
    out.write("%.6f of the full search (weights %s); bad CTUs %d of %d labelled\n" % (share, " ".join(str(w) for w in weights), int(counts["bad_ctus"]),
                                                                                     info["labelled_ctus"]))
    if opt["out"]:
        out.write("wrote %s (%s order): %s" % (opt["out"], opt["order"], open(opt["out"]).read()))
    return result


def run(opt, cases, out=sys.stdout, err=sys.stderr):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    note = lambda s: err.write(s + "\n")
    if opt.get("reached"):
        return run_reached(pkg, opt, cases, out, note)
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        cal = pkg.Calibrator(ctx)
        add_cases(pkg, ctx, cal, cases, note)
        hist, rejected, skipped = cal.get()
        rep = cal.choose(opt["eps_down"], opt["eps_up"])
        levels = rep.as_dicts()
        if opt["out"]:
            cal.write_thr_info(opt["out"], rep, opt["order"])
        if opt["hist"]:
            hist.astype("<u8").tofile(opt["hist"])
        if opt["reliability_out"]:
            pkg.ethcnn.risk_write(opt["reliability_out"], pkg.ethcnn.risk_from_hist(hist))
            note("wrote %s: the reliability table of %d samples" % (opt["reliability_out"], int(hist.sum())))
    finally:
        ctx.close()
    result = {"levels": levels, "rejected": [int(x) for x in rejected], "skipped_partial": skipped,
              "eps_down_ppm": opt["eps_down"], "eps_up_ppm": opt["eps_up"], "out": opt["out"], "order": opt["order"]}
    if opt["json"]:
        out.write(json.dumps(result) + "\n")
        return result
    for name, lv, ed, eu, rj in zip(("64x64", "32x32", "16x16"), levels, opt["eps_down"], opt["eps_up"], result["rejected"]):
        out.write("%s  unsplit %d  split %d  rejected %d%s%s\n" % (name, lv["n0"], lv["n1"], rj, "  EMPTY CLASS" if lv["empty_class"] else "",
                                                                "  CROSSED (one threshold for both)" if lv["crossed"] else ""))
        out.write("    down %.10f (k %d)  wrongly stopped %d of %d split (budget %d ppm)\n" % (lv["down"], lv["down_k"], lv["miss"], lv["n1"], ed))
        out.write("    up   %.10f (k %d)  wrongly forced  %d of %d unsplit (budget %d ppm)\n" % (lv["up"], lv["up_k"], lv["fsplit"], lv["n0"], eu))
        out.write("    full search remains for %d (%.4f); accuracy at 0.5: %.4f\n" % (lv["uncertain"], lv["uncertain_share"], lv["accuracy_512"]))
    if skipped:
        out.write("%d CTUs not wholly inside the picture were left out\n" % skipped)
    if opt["out"]:
        out.write("wrote %s (%s order): %s" % (opt["out"], opt["order"], open(opt["out"]).read()))
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
