"""Caller-owned buffers of the Low-Delay-P chain's device entries ("Caller-owned buffers the suite reaches"): luma
planes at a pitch, a frame stride and a byte offset of the caller's, and device allocations with guard bands around the part that
is handed over.  No GPU is needed to import this module; guarded() and check_guards() take a context.

The lists here are the ones the tests parametrise over: tests/test_gpu_ldp_buffers.py runs them, tests/test_ldp_buffers_cpu.py holds
them against DESIGN.md and checks what they cover."""
import itertools

import numpy as np

GUARD = 256             # bytes of guard band on each side, at least
NAN_WORD = 0x7FC0ABCD   # float buffers: a quiet NaN with a payload no kernel produces
ALT_WORD = 0x447A0000   # the second poison around inputs: 1000.0f, a value that would decide a sigmoid instead of poisoning it
LUMA_FILL = (0xEE, 0x11)  # the two poisons of everything in a luma buffer that is not a pixel
STAGE_BYTES = 64 << 20  # seq_host_run (csrc/ethcnn_ldp.cpp) stages luma in pieces of at most this many bytes

# (width, height): CTU counts 1, 8, 12, 17, 1056 -- a group of one valid lane; one ragged group, width no multiple of 16; one ragged
# group; a full group plus one CTU (2 / 1 / 1 recurrence blocks per level); a second gate mini-batch of 32 CTUs
SHAPES = [(64, 64), (203, 77), (200, 136), (1088, 64), (2112, 2048)]

# (entry, pointer, required alignment in bytes): every caller pointer of the five entries.  16: the kernels touch it with 16-byte
# accesses; 4: dword accesses only; 1: any byte address.  The table in DESIGN.md section 25 has one row per entry of this list.
POINTER_ROWS = [
    ("ethcnn_resi_vectors_device", "d_luma", 1),
    ("ethcnn_resi_vectors_device", "d_vec", 4),
    ("ethcnn_lstm_step_device", "d_vec", 16),
    ("ethcnn_lstm_step_device", "d_state_in", 16),
    ("ethcnn_lstm_step_device", "d_state_out", 16),
    ("ethcnn_lstm_step_device", "d_probs", 4),
    ("ethcnn_ldp_sequence_device", "d_luma", 1),
    ("ethcnn_ldp_sequence_device", "d_state_in", 16),
    ("ethcnn_ldp_sequence_device", "d_probs", 4),
    ("ethcnn_ldp_group_sequence_device", "d_luma[m]", 1),
    ("ethcnn_ldp_group_sequence_device", "d_state_in[m]", 16),
    ("ethcnn_ldp_group_sequence_device", "d_probs[m]", 4),
    ("ethcnn_ldp_batch_run_device", "seqs[j].d_luma", 1),
    ("ethcnn_ldp_batch_run_device", "seqs[j].d_state_in", 16),
    ("ethcnn_ldp_batch_run_device", "seqs[j].d_probs", 4),
]
REFUSAL_ROWS = [r for r in POINTER_ROWS if r[2] > 1]


def solo_geometries(w, h):
    """The layouts of the solo geometry cases for a w x h picture: (pitch, frame_stride, offset, chunk, i_frame_first), the whole
    product of pitch = w + {1, 7, 64}, frame_stride = pitch * h + {13, pitch * (h // 2)}, offset {1, 5, 15} and chunk {0, 2}; the first
    frame number walks through 0, 1, 3 so that it meets every offset and every chunk (tests/test_ldp_buffers_cpu.py asserts that)."""
    out = []
    for k, (dp, tall, off, chunk) in enumerate(itertools.product((1, 7, 64), (False, True), (1, 5, 15), (0, 2))):
        pitch = w + dp
        out.append((pitch, pitch * h + (pitch * (h // 2) if tall else 13), off, chunk, (0, 1, 3)[(k + k // 2 + k // 6) % 3]))
    return out


def nctu(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def frames(seed, w, h, nf):
    """residual-like luma with quieter bands that move from frame to frame, so that mini-batches and frames differ"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(nf, h, w), dtype=np.uint8)
    for t in range(nf):
        r0 = (t * h // nf) // 2
        out[t, r0: r0 + h // 2] = (out[t, r0: r0 + h // 2] // (8 << (t % 3)) + 120).astype(np.uint8)
    return out


def state(seed, n):
    """a (c, h) state [n, 2, 448] inside the cell's ranges"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-5, 5, (n, 448)), rng.uniform(-1, 1, (n, 448))], 1).astype(np.float32)


def pitched_bytes(w, h, nf, pitch, frame_stride, offset):
    """the size of the buffer pitched() returns: the lead-in, nf - 1 strides and the last frame up to the end of its stride (or of its
    last pixel row, for a stride shorter than a frame)"""
    return offset + (nf - 1) * frame_stride + max(frame_stride, (h - 1) * pitch + w)


def lay_out(lum, pitch, frame_stride, offset, fill):
    """the frames lum [nf, h, w] in one uint8 array: row y of frame t starts at offset + t * frame_stride + y * pitch; every byte that
    is not a pixel (lead-in, pitch gap, gap between frames, tail) equals fill"""
    nf, h, w = lum.shape
    assert pitch >= w and frame_stride >= (h - 1) * pitch + w and offset >= 0
    out = np.full(pitched_bytes(w, h, nf, pitch, frame_stride, offset), fill, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(out[offset:], shape=(nf, h, w), strides=(frame_stride, pitch, 1))
    rows[...] = lum
    return out


def pitched(seed, w, h, nf, pitch, frame_stride, offset, fill):
    """-> (bytes, frames): the pictures of frames(seed, w, h, nf) laid out by lay_out, and their contiguous [nf, h, w] copy"""
    lum = frames(seed, w, h, nf)
    return lay_out(lum, pitch, frame_stride, offset, fill), lum


def unpitch(buf, w, h, nf, pitch, frame_stride, offset):
    """the [nf, h, w] pixels of a pitched buffer, by the formula"""
    return np.stack([np.stack([buf[offset + t * frame_stride + y * pitch: offset + t * frame_stride + y * pitch + w] for y in range(h)])
                     for t in range(nf)])


def pattern_bytes(pattern, nbytes):
    """nbytes of poison: a byte value (0..255) repeated, or a 32-bit word (little-endian) repeated from the start of the allocation"""
    if 0 <= pattern <= 0xFF:
        return np.full(nbytes, pattern, dtype=np.uint8)
    return np.resize(np.array([pattern], dtype="<u4").view(np.uint8), nbytes)


class Guarded(object):
    """a device allocation of lead + nbytes + tail bytes, all of it filled with the pattern; ptr is the address of the inner nbytes"""

    def __init__(self, ctx, nbytes, lead, tail, pattern):
        assert lead >= GUARD and tail >= GUARD
        self.ctx, self.nbytes, self.lead, self.tail, self.pattern = ctx, int(nbytes), int(lead), int(tail), pattern
        self.buf = ctx.alloc(self.lead + self.nbytes + self.tail)
        assert self.buf.ptr % 16 == 0, "lead alone decides the alignment of the inner address"
        self.buf.upload(pattern_bytes(pattern, self.buf.nbytes))
        self.ptr = self.buf.ptr + self.lead

    def upload(self, arr, at=0):
        """arr -> the inner bytes from byte `at` on"""
        arr = np.ascontiguousarray(arr)
        assert 0 <= at and at + arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.ethcnn_memcpy_h2d(self.ctx.h, self.ptr + at, arr.ctypes.data, arr.nbytes))

    def free(self):
        self.buf.free()


def guarded(ctx, nbytes, lead=GUARD, tail=GUARD, pattern=NAN_WORD):
    """-> Guarded: the allocation (.buf) and the inner address (.ptr).  lead decides the alignment of .ptr: the allocation itself is
    aligned to 16 bytes and more (asserted), so lead = 256 + 4 gives an address that is 4-byte but not 16-byte aligned"""
    return Guarded(ctx, nbytes, lead, tail, pattern)


def check_guards(g, dtype=np.float32, what=""):
    """downloads the whole allocation, asserts that both bands still hold the pattern bit for bit, returns the payload"""
    g.ctx.synchronize()
    whole = g.buf.download(np.uint8, g.buf.nbytes)
    want = pattern_bytes(g.pattern, whole.size)
    for name, lo, hi in (("in front of", 0, g.lead), ("behind", g.lead + g.nbytes, whole.size)):
        bad = np.nonzero(whole[lo:hi] != want[lo:hi])[0]
        assert bad.size == 0, "%s: %d bytes of the guard band %s the buffer were overwritten, the first at byte %d of the band" % (
            what, bad.size, name, int(bad[0]))
    return whole[g.lead: g.lead + g.nbytes].copy().view(dtype)
