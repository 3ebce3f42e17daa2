"""Build the All-Intra sample files on the GPU: the driver of Extract_Data/extract_data_AI.py:129-181, with command-line flags in
place of its module constants.  The records are cut in HBM by the library (SampleSet, include/ethcnn.h "sample sets"); this file
finds the input files and names the outputs.

    python extract_data_AI.py --yuv-dir YUV_All --info-dir AI_Info --out-dir Data             # AI_Train_<n>.dat (+ _shuffled), Valid, Test
    python extract_data_AI.py --yuv-dir . --info-dir . --sequences my.txt --set train --qps 32
    python extract_data_AI.py --yuv-dir UHD --info-dir UHD_Info --sequences uhd.txt --input-bit-depth 10      # Main10 sources

Inputs per sequence: <yuv-dir>/<name>.yuv and, per QP, the one file matching <info-dir>/Info*_<name>_*qp<QP>*CUDepth.dat.
Outputs: AI_<Train|Valid|Test>_<count>.dat, byte-identical to the reference's, and <that>_shuffled: the same records permuted by
--seed (the library's permutation; the reference's own order comes from Python's unseeded random and cannot be reproduced).
--input-bit-depth / --input-chroma-format give the source format of every YUV of the run; a --sequences line
`name width height [bit_depth [chroma]]` overrides them for its sequence.  Records hold the luma narrowed to 8 bits by the rule of
include/ethcnn.h.
"""
import argparse
import importlib
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sequence_table as di  # noqa: E402


def parse_args(argv, inter=False):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0] if not inter else None)
    ap.add_argument("--yuv-dir", required=True, help="directory of the residual YUVs (resi*_<name>_*qp<QP>*.yuv)" if inter else "directory of <name>.yuv")
    ap.add_argument("--info-dir", required=True, help="directory of Info*_<name>_*qp<QP>*CUDepth.dat")
    if inter:
        ap.add_argument("--config", choices=("LDP", "LDB", "RA"), default="LDP")
    ap.add_argument("--qps", type=int, nargs="+", default=list(di.QP_LIST))
    ap.add_argument("--seed", type=int, default=0, help="of the _shuffled file's permutation")
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--set", choices=("train", "valid", "test", "all"), default="all")
    ap.add_argument("--sequences", metavar="FILE", help="`name width height` lines replacing the built-in table and index lists" +
                    ("" if inter else "; All-Intra lines may go on with `bit_depth [chroma]`"))
    if not inter:  # (HM's residual files are always 8-bit 4:2:0: the inter driver does not take the options)
        di.add_format_args(ap)
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def add_sequences(sset, a, rows):
    for name, w, h, depth, chroma in rows:
        sset.add_sequence(w, h, di.find_one(a.yuv_dir, name + ".yuv"), [di.info_file(a.info_dir, name, q) for q in a.qps], bit_depth=depth,
                          chroma=chroma)


def write_set(sset, prefix, which, a):
    """<prefix>_<Set>_<count>.dat and its _shuffled copy; returns the first path"""
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "%s_%s_%d.dat" % (prefix, di.SET_NAMES[which], sset.count))
    sset.write(path)
    sset.write(path + "_shuffled", seed=a.seed)
    print("%s : %d samples" % (path, sset.count))
    return path


def main(argv=None):
    a = parse_args(argv)
    fmt = di.source_format(a)
    sets = [(which, di.select(a.sequences, di.AI_INDEX, which, fmt)) for which in (("train", "valid", "test") if a.set == "all" else (a.set,))]
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    with pkg.EthCnn(device=a.device) as ctx:  # (bad options and --sequences lines have been refused by now)
        for which, rows in sets:
            with pkg.SampleSet(ctx, "ai", a.qps) as sset:
                add_sequences(sset, a, rows)
                write_set(sset.build(), "AI", which, a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
