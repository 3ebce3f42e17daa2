"""Deep and non-4:2:0 re-encodings of the cases of extract_cases.py (shared by test_extract16_cpu.py and test_gpu_extract16.py).

A deep sample is s16 = (s8 << (bit_depth - 8)) | low with low random in [0, 2^(bit_depth - 8)): the narrowing rule of include/ethcnn.h,
min(s16 >> (bit_depth - 8), 255), gives s8 back exactly.  A re-encoded file therefore has to yield the records that
tests/golden/extract_golden.npz holds for the 8-bit 4:2:0 file, byte for byte: no fixture of its own is needed."""
import os

import numpy as np

import extract_cases as ec

# name -> (bit_depth, chroma) per sequence of an All-Intra case (both cases have two sequences)
FORMS = {
    "d10_420": [(10, 420), (10, 420)],
    "d8_444": [(8, 444), (8, 444)],  # 8 bits: the unchanged 8-bit cut kernel, other frame offsets
    "d12_400": [(12, 400), (12, 400)],
    "mixed": [(10, 422), (8, 420)],
    "d16_420": [(16, 420), (16, 420)],
}
CHROMA_SAMPLES = {400: lambda w, h: 0, 420: lambda w, h: w * h // 2, 422: lambda w, h: w * h, 444: lambda w, h: 2 * w * h}


def widen(luma8, bit_depth, rng):
    """uint8 -> uint16 samples of that depth that narrow back to luma8"""
    shift = bit_depth - 8
    low = rng.integers(0, 1 << shift, luma8.shape, dtype=np.uint16) if shift else np.uint16(0)
    return (luma8.astype(np.uint16) << shift) | low


def frame_bytes(w, h, bit_depth, chroma):
    return (w * h + CHROMA_SAMPLES[chroma](w, h)) * (2 if bit_depth > 8 else 1)


def reencode(luma8, path, bit_depth, chroma, rng):
    """luma8 [F, H, W] -> a planar file of that format: the luma widened, chroma planes of noise of the size the format demands"""
    F, H, W = luma8.shape
    dtype = "<u2" if bit_depth > 8 else np.uint8
    with open(path, "wb") as f:
        for k in range(F):
            y = widen(luma8[k], bit_depth, rng) if bit_depth > 8 else luma8[k]
            f.write(np.ascontiguousarray(y, dtype=dtype).tobytes())
            f.write(rng.integers(0, 1 << bit_depth, CHROMA_SAMPLES[chroma](W, H)).astype(dtype).tobytes())


def make_inputs(case, form, directory, golden):
    """extract_cases.make_inputs, then every YUV rewritten in place in the form's format of its sequence.
    Returns [(name, width, height, [yuv path], [label paths], bit_depth, chroma)]."""
    seqs = ec.make_inputs(case, str(directory), golden["labels_" + case] if "labels_" + case in golden.files else None)
    rng = np.random.default_rng(1000 + ec.CASES[case]["seed"])
    out = []
    for (name, w, h, yuvs, labs), (depth, chroma) in zip(seqs, FORMS[form]):
        luma = ec.read_luma(yuvs[0], w, h).copy()
        reencode(luma, yuvs[0], depth, chroma, rng)
        assert os.path.getsize(yuvs[0]) == luma.shape[0] * frame_bytes(w, h, depth, chroma)
        out.append((name, w, h, yuvs, labs, depth, chroma))
    return out


def sequences_file(path, seqs, columns):
    """a --sequences file of the re-encoded inputs; columns 3: `name width height`, 4: + bit_depth, 5: + chroma"""
    with open(str(path), "w") as f:
        for s in seqs:
            f.write(" ".join(str(x) for x in (s[0], s[1], s[2], s[5], s[6])[:columns]) + "\n")
    return str(path)
