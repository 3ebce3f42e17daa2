"""Regenerates tests/golden/extract_golden.npz: the UNSHUFFLED output bytes of the reference's own Extract_Data scripts
(extract_data_AI.py, extract_data_LDP_LDB_RA.py: numpy only) on the seeded inputs of tests/extract_cases.py.  Needs the reference
checkout; run from anywhere:  python tests/golden/gen_extract_golden.py [reference root]
The label bytes of the "real" case are cut from the reference's AI_Info 768x512 files (frames 0.., top-left corner) and stored too."""
import contextlib
import glob
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import extract_cases as ec  # noqa: E402
from conftest import REFERENCE  # noqa: E402


def real_labels(ref, case):
    c, out = ec.CASES[case], []
    for name, w, h, frames in c["seqs"]:
        for qp in c["qps"]:
            (path,) = glob.glob(os.path.join(ref, "AI_Info", "Info*_IntraTest_768x512_qp%d_*CUDepth.dat" % qp))
            full = np.fromfile(path, dtype=np.uint8).reshape(-1, 512 // 16, 768 // 16)
            out.append(full[:frames, :h // 16, :w // 16].reshape(-1))
    return np.concatenate(out)


def run_reference(ref, case, directory, real):
    """the reference's generate_data on the case's files -> the bytes of <CONFIG>_Train_<n>.dat"""
    sys.path.insert(0, os.path.join(ref, "Extract_Data"))
    import extract_data_AI as ref_ai
    import extract_data_LDP_LDB_RA as ref_inter
    c = ec.CASES[case]
    seqs = ec.make_inputs(case, directory, real)
    names = [s[0] for s in seqs]
    widths, heights = np.array([s[1] for s in seqs]), np.array([s[2] for s in seqs])
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            if c["kind"] == "ai":
                ref_ai.generate_data(directory + "/", directory + "/", names, widths, heights, c["qps"], list(range(len(seqs))), "Train")
            else:
                ref_inter.generate_data(directory + "/", directory + "/", names, widths, heights, c["qps"], list(range(len(seqs))), "Train",
                                        c["config"])
    finally:
        os.chdir(cwd)
    path = os.path.join(directory, "%s_Train_%d.dat" % (c["config"], ec.EXPECTED_COUNT[case]))
    return np.fromfile(path, dtype=np.uint8)


def generate(ref):
    out = {}
    for case, c in ec.CASES.items():
        real = real_labels(ref, case) if c["labels"] == "real" else None
        if real is not None:
            out["labels_" + case] = real
        with tempfile.TemporaryDirectory() as d:
            out["records_" + case] = run_reference(ref, case, d, real)
    return out


if __name__ == "__main__":
    arrays = generate(sys.argv[1] if len(sys.argv) > 1 else REFERENCE)
    np.savez_compressed(ec.GOLDEN, **arrays)
    print({k: v.shape for k, v in arrays.items()}, os.path.getsize(ec.GOLDEN))
