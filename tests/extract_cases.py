"""The cases of tests/golden/extract_golden.npz and their inputs, regenerated from seeds (shared by tests/golden/gen_extract_golden.py,
which runs the reference's two Extract_Data scripts on them, and by the tests that run this project's extractor on the same files).
Label bytes of the "real" case are a cut of one of the reference's AI_Info files and travel in the fixture itself."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extract_golden.npz")

# name -> kind, config (file-name prefix), QP list, [(sequence name, width, height, frames)], seed, label source
CASES = {
    "ai4": dict(kind="ai", config="AI", qps=[22, 27, 32, 37], seqs=[("SeqA_200x136", 200, 136, 3), ("SeqB_128x64", 128, 64, 2)], seed=11,
                labels="real"),
    "ai1": dict(kind="ai", config="AI", qps=[32], seqs=[("SeqA_200x136", 200, 136, 3), ("SeqB_128x64", 128, 64, 2)], seed=12, labels="seed"),
    "ldp": dict(kind="inter", config="LDP", qps=[22, 27, 32, 37], seqs=[("SeqA_200x136", 200, 136, 3), ("SeqB_128x64", 128, 64, 2)], seed=13,
                labels="seed"),
    "ra": dict(kind="inter", config="RA", qps=[22, 27, 32, 37], seqs=[("SeqC_64x64", 64, 64, 12), ("SeqD_64x64", 64, 64, 9)], seed=14,
               labels="seed"),
}
EXPECTED_COUNT = {"ai4": 22, "ai1": 22, "ldp": 14, "ra": 19}


def label_shape(w, h, frames):
    return (frames, h // 16, w // 16)


def synth_yuv(rng, w, h, frames):
    """4:2:0 frames: a luma ramp with 3 bits of noise (compresses in the fixture; every byte still position-dependent), noise chroma"""
    out = []
    for f in range(frames):
        y = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5 + 17 * f + rng.integers(0, 8, (h, w))) % 256
        out.append(y.astype(np.uint8).tobytes())
        out.append(rng.integers(0, 256, w * h // 2, dtype=np.uint8).tobytes())
    return b"".join(out)


def make_inputs(case, directory, real_labels=None):
    """Writes the case's YUV and label files into `directory` (named so that the reference's glob patterns find them).
    real_labels: for a "real" case, the uint8 array the fixture holds (concatenated per sequence and QP in loop order).
    Returns [(name, width, height, [yuv paths], [label paths])]."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    os.makedirs(directory, exist_ok=True)
    out, at = [], 0
    for name, w, h, frames in c["seqs"]:
        yuvs, labs = [], []
        if c["kind"] == "ai":
            yuvs.append(os.path.join(directory, name + ".yuv"))
            with open(yuvs[0], "wb") as f:
                f.write(synth_yuv(rng, w, h, frames))
        for qp in c["qps"]:
            if c["kind"] == "inter":
                yuvs.append(os.path.join(directory, "resi_%s_%s_qp%d_nf%d.yuv" % (c["config"], name, qp, frames)))
                with open(yuvs[-1], "wb") as f:
                    f.write(synth_yuv(rng, w, h, frames))
            n = int(np.prod(label_shape(w, h, frames)))
            if c["labels"] == "real":
                lab = np.asarray(real_labels[at:at + n], dtype=np.uint8)
                at += n
            else:
                lab = rng.integers(0, 4, n, dtype=np.uint8)
            labs.append(os.path.join(directory, "Info_20170810_%s_%s_qp%d_nf%d_CUDepth.dat" % (c["config"], name, qp, frames)))
            with open(labs[-1], "wb") as f:
                f.write(lab.tobytes())
        out.append((name, w, h, yuvs, labs))
    return out


def load_golden():
    return np.load(GOLDEN)


# ---- numpy restatement of the record layouts (include/ethcnn.h "sample sets"), checked against the fixture by test_extract_cpu.py
def ra_display(i, n):
    if i == 0:
        return 0
    gop, table = (i - 1) // 8, [7, 3, 1, 0, 2, 5, 4, 6]
    table = [x for x in table if x < min(n - 1 - gop * 8, 8)]
    return 1 + table[(i - 1) % 8] + gop * 8


def np_cut_ai(luma, labels, qps):
    """luma [F, H, W], labels [nqps][F, H // 16, W // 16] -> records [F * (H // 64) * (W // 64), 4992]"""
    F, H, W = luma.shape
    nl, nc = H // 64, W // 64
    rec = np.full((F, nl, nc, 4992), 255, dtype=np.uint8)
    tiles = luma[:, :nl * 64, :nc * 64].reshape(F, nl, 64, nc, 64).transpose(0, 1, 3, 2, 4)
    rec[..., :4096] = tiles.reshape(F, nl, nc, 4096)
    for q, lab in zip(qps, labels):
        d = lab[:, :nl * 4, :nc * 4].reshape(F, nl, 4, nc, 4).transpose(0, 1, 3, 2, 4)
        rec[..., 4160 + 16 * q:4176 + 16 * q] = d.reshape(F, nl, nc, 16)
    return rec.reshape(-1, 4992)


def np_cut_inter(lumas, labels, qps, frame_numbers, seq):
    """lumas [4][F, H, W] and labels [4][F, H // 16, W // 16], already in the order the records take; frame_numbers [F]"""
    F, H, W = lumas[0].shape
    nl, nc = H // 64, W // 64
    rec = np.full((F, nl, nc, 16516), 255, dtype=np.uint8)
    rec[..., 0] = 1

    def le(at, nbytes, value):
        for k in range(nbytes):
            rec[..., at + k] = (np.asarray(value) >> (8 * k)) & 255

    le(2, 2, W)
    le(4, 2, H)
    le(10, 4, np.asarray(frame_numbers, dtype=np.int64)[:, None, None])
    le(14, 2, np.arange(nl)[None, :, None])
    le(16, 2, np.arange(nc)[None, None, :])
    le(18, 2, seq)
    for s in range(4):
        at = 64 + 4113 * s
        rec[..., at] = qps[s]
        d = labels[s][:, :nl * 4, :nc * 4].reshape(F, nl, 4, nc, 4).transpose(0, 1, 3, 2, 4)
        rec[..., at + 1:at + 17] = d.reshape(F, nl, nc, 16)
        t = lumas[s][:, :nl * 64, :nc * 64].reshape(F, nl, 64, nc, 64).transpose(0, 1, 3, 2, 4)
        rec[..., at + 17:at + 4113] = t.reshape(F, nl, nc, 4096)
    return rec.reshape(-1, 16516)


def read_luma(path, w, h):
    a = np.fromfile(path, dtype=np.uint8).reshape(-1, w * h * 3 // 2)
    return a[:, :w * h].reshape(-1, h, w)


def np_records(case, seqs):
    """the case's whole sample file from the files make_inputs wrote, by the restatement above"""
    c, out = CASES[case], []
    for iseq, (name, w, h, yuvs, labs) in enumerate(seqs):
        labels = [np.fromfile(p, dtype=np.uint8).reshape(-1, h // 16, w // 16) for p in labs]
        if c["kind"] == "ai":
            out.append(np_cut_ai(read_luma(yuvs[0], w, h), labels, c["qps"]))
        else:
            lumas = [read_luma(p, w, h) for p in yuvs]
            n = lumas[0].shape[0]
            enc = list(range(1, n))
            disp = [ra_display(i, n) if c["config"] == "RA" else i for i in enc]
            out.append(np_cut_inter([l[disp] for l in lumas], [l[disp] for l in labels], c["qps"], enc, iseq))
    return np.concatenate(out).reshape(-1)
