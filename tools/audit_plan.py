#!/usr/bin/env python
"""Audit a 16-bit plan on real pictures, or compare two prediction files, on the GPU (include/ethcnn.h "comparing two predictions").

  audit_plan.py --yuv FILE W H QP --plan 2|3 --model-dir DIR [--first N --step N --count N]
        frames first + i * step, i < count (default 0, 1, 1), of an 8-bit 4:2:0 file through the exact plan and through plan P with the
        checkpoint of the QP's band in DIR (ETHCNN_SYNTHETIC_SEED / ETHCNN_HEAD_GAIN opt into seeded weights when it is absent, as for the
        launcher), open gates; the two results compared.
  audit_plan.py --case A.dat B.dat W H
        two cu_depth.dat files of W x H frames, compared as they are.  No model.

Options: --tol T (default 1e-4, the plans' contract), --thr-info FILE --order ai|ldp (the candidate under which classes and the pruned
search are compared; its six values are rounded to the grid k / 1024), --flags-out FILE (one byte per CTU: bit 0 rejected, bit 1 a value
over tol, bit 2 a class differs, bit 3 the search differs), --device N.

Prints one table: per level max |dp|, the worst CTU as (frame, x, y), values over tol, classes that differ; CTUs whose search differs;
checks per CU size on both sides; fast passes / passes.

Exit status: 0 nothing is over tol; 2 something is; 3 a --yuv source whose audited run took no 16-bit pass (the geometry runs as
single-launch passes, which compute exactly under every plan: the zeros say nothing about the plan); 1 bad arguments, before a context
exists, or a failure.

Not built: deep or non-4:2:0 sources, the Low-Delay-P path (it always computes exactly), several GPUs."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ("64x64", "32x32", "16x16", "8x8")


class Usage(Exception):
    pass


def _take(argv, i, n, name):
    if i + n > len(argv):
        raise Usage("%s takes %d value(s)" % (name, n))
    return argv[i:i + n], i + n


def _int(text, name, lo):
    try:
        v = int(text)
    except ValueError:
        raise Usage("%s: '%s' is not an integer" % (name, text))
    if v < lo:
        raise Usage("%s must be at least %d" % (name, lo))
    return v


def parse(argv):
    opt = {"yuv": None, "case": None, "plan": None, "model_dir": None, "first": 0, "step": 1, "count": 1, "tol": 1e-4, "thr_info": None, "order": None,
           "flags_out": None, "device": 0}
    i = 0
    while i < len(argv):
        a = argv[i]
        i += 1
        if a in ("-h", "--help"):
            raise Usage("")
        elif a == "--yuv":
            v, i = _take(argv, i, 4, a)
            opt["yuv"] = (v[0], _int(v[1], "W", 1), _int(v[2], "H", 1), _int(v[3], "QP", 0))
        elif a == "--case":
            v, i = _take(argv, i, 4, a)
            opt["case"] = (v[0], v[1], _int(v[2], "W", 1), _int(v[3], "H", 1))
        elif a in ("--plan", "--first", "--step", "--count", "--device"):
            v, i = _take(argv, i, 1, a)
            opt[a[2:]] = _int(v[0], a, 1 if a == "--step" else 0)
        elif a in ("--model-dir", "--thr-info", "--order", "--flags-out"):
            v, i = _take(argv, i, 1, a)
            opt[a[2:].replace("-", "_")] = v[0]
        elif a == "--tol":
            v, i = _take(argv, i, 1, a)
            try:
                opt["tol"] = float(v[0])
            except ValueError:
                raise Usage("--tol: '%s' is not a number" % v[0])
            if not opt["tol"] >= 0:
                raise Usage("--tol is a number >= 0")
        else:
            raise Usage("unknown argument '%s'" % a)
    if (opt["yuv"] is None) == (opt["case"] is None):
        raise Usage("exactly one source: --yuv FILE W H QP or --case A.dat B.dat W H")
    w, h = opt["yuv"][1:3] if opt["yuv"] else opt["case"][2:4]
    if w % 8 or h % 8:
        raise Usage("HM pictures have sizes that are multiples of 8: got %d x %d" % (w, h))
    if opt["yuv"]:
        if opt["plan"] not in (2, 3) or opt["model_dir"] is None:
            raise Usage("--yuv needs --plan 2|3 and --model-dir DIR")
        if not os.path.isfile(opt["yuv"][0]):
            raise Usage("%s: no such file" % opt["yuv"][0])
    else:
        if opt["plan"] is not None or opt["model_dir"] is not None:
            raise Usage("--case compares two files: it takes no --plan and no --model-dir")
        per = ((w + 63) // 64) * ((h + 63) // 64) * 84
        sizes = []
        for path in opt["case"][:2]:
            if not os.path.isfile(path):
                raise Usage("%s: no such file" % path)
            sizes.append(os.path.getsize(path))
            if sizes[-1] % per:
                raise Usage("%s: %d bytes are not whole %d x %d frames of %d bytes" % (path, sizes[-1], w, h, per))
        if sizes[0] != sizes[1]:
            raise Usage("the two files hold %d and %d bytes" % tuple(sizes))
    if (opt["thr_info"] is None) != (opt["order"] is None) or opt["order"] not in (None, "ai", "ldp"):
        raise Usage("--thr-info FILE and --order ai|ldp go together")
    return opt


def table(r, width, height, tol, yuv, first=0, step=1, out=sys.stdout):
    cw, ch = (width + 63) // 64, (height + 63) // 64
    out.write("%-6s %-14s %-22s %-16s %s\n" % ("level", "max |dp|", "worst CTU (frame,x,y)", "values over tol", "classes that differ"))
    for l in range(3):
        w = r["worst_ctu"][l]
        where = "-" if w < 0 else "(%d, %d, %d)" % (first + (w // (cw * ch)) * step, w % cw, (w % (cw * ch)) // cw)
        out.write("%-6s %-14.6g %-22s %-16d %s\n" % (SIZES[l], r["max_abs"][l], where, r["over_tol"][l], r["class_diff"][l] if r["with_thr"] else "n/a"))
    out.write("CTUs: %d compared, %d rejected; tolerance %g\n" % (r["ctus"] - r["rejected_ctus"], r["rejected_ctus"], tol))
    if r["with_thr"]:
        out.write("CTUs whose pruned search differs: %d\n" % r["search_diff_ctus"])
        out.write("checks per CU size (%s): a %s | b %s\n" % (" ".join(SIZES), " ".join(str(x) for x in r["checked_a"]), " ".join(str(x) for x in r["checked_b"])))
    else:
        out.write("CTUs whose pruned search differs: n/a (no --thr-info)\n")
    if yuv:
        out.write("fast passes / passes: %d / %d (plan %d)\n" % (r["fast_passes"], r["passes"], r["plan"]))


def run(opt):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    e = pkg.ethcnn
    thr = e.read_thr_info_k(opt["thr_info"], opt["order"]) if opt["thr_info"] else None
    ctx = pkg.EthCnn(device=opt["device"])
    try:
        if opt["yuv"]:
            path, w, h, qp = opt["yuv"]
            pkg.video_to_cu_depth.restore_model(ctx, qp, opt["model_dir"])
            r = ctx.audit_plan_yuv_file(path, w, h, qp, opt["plan"], opt["first"], opt["step"], opt["count"], opt["tol"], thr)
            table(r, w, h, opt["tol"], True, opt["first"], opt["step"])
            if r["fast_passes"] == 0:
                sys.stdout.write("no pass of the audited run took the 16-bit path: this geometry runs as single-launch passes, which compute exactly under "
                                 "every plan; the zeros above say nothing about plan %d\n" % opt["plan"])
                return 3
        else:
            pa, pb, w, h = opt["case"]
            a, b = np.fromfile(pa, dtype="<f4"), np.fromfile(pb, dtype="<f4")
            r = ctx.compare_frames(a, b, w, h, opt["tol"], thr, want_flags=bool(opt["flags_out"]))
            if opt["flags_out"]:
                r["flags"].tofile(opt["flags_out"])
            table(r, w, h, opt["tol"], False)
        return 2 if sum(r["over_tol"]) else 0
    finally:
        ctx.close()


def main(argv):
    try:
        opt = parse(argv[1:])
        if opt["yuv"] and opt["flags_out"]:
            raise Usage("--flags-out goes with --case (the audit keeps no per-CTU flags)")
        if opt["thr_info"]:
            if ROOT not in sys.path:
                sys.path.insert(0, ROOT)
            importlib.import_module("hevc-complexity-reduction_amd").ethcnn.read_thr_info_k(opt["thr_info"], opt["order"])  # before a context exists
    except Usage as u:
        sys.stderr.write((str(u) + "\n" if str(u) else "") + __doc__ + "\n")
        return 1
    except (ValueError, OSError) as err:
        sys.stderr.write("audit_plan: %s\n" % err)
        return 1
    try:
        return run(opt)
    except Exception as err:  # a failure of the library: its message, exit status 1
        sys.stderr.write("audit_plan: %s\n" % err)
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
