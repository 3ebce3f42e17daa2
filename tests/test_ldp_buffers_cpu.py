"""No GPU: the helpers of tests/ldp_buffers.py (pitched luma, poison patterns), the oracle's indifference to the layout of a plane, and
the pointer / alignment table of DESIGN.md section 25 against the list tests/test_gpu_ldp_buffers.py parametrises over."""
import os
import re

import numpy as np
import pytest

import ldp_buffers as lb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("w,h", lb.SHAPES[:4])
def test_pitched_round_trips_and_fill_changes_no_pixel(w, h):
    nf = 3
    for pitch, fs, off, chunk, first in lb.solo_geometries(w, h)[::5]:
        a, lum = lb.pitched(w + h, w, h, nf, pitch, fs, off, 0xEE)
        b, lum_b = lb.pitched(w + h, w, h, nf, pitch, fs, off, 0x11)
        assert a.dtype == np.uint8 and a.ndim == 1 and a.size == lb.pitched_bytes(w, h, nf, pitch, fs, off)
        assert lum.shape == (nf, h, w) and lum.flags["C_CONTIGUOUS"] and np.array_equal(lum, lb.frames(w + h, w, h, nf))
        assert np.array_equal(lb.unpitch(a, w, h, nf, pitch, fs, off), lum) and np.array_equal(lb.unpitch(b, w, h, nf, pitch, fs, off), lum_b)
        assert np.array_equal(lum, lum_b)
        # everything that is not a pixel is fill: lead-in, pitch gaps, the gap between frames, the tail
        pixel = np.zeros(a.size, bool)
        for t in range(nf):
            for y in range(h):
                pixel[off + t * fs + y * pitch: off + t * fs + y * pitch + w] = True
        assert int(pixel.sum()) == nf * h * w and not pixel[:off].any() and not pixel[-1]
        assert (a[~pixel] == 0xEE).all() and (b[~pixel] == 0x11).all() and np.array_equal(a[pixel], b[pixel])


def test_the_solo_geometries_cover_what_they_claim():
    for w, h in lb.SHAPES[:4]:
        g = lb.solo_geometries(w, h)
        assert len(set(g)) == 36
        assert {p - w for p, s, o, c, f in g} == {1, 7, 64} and {o for p, s, o, c, f in g} == {1, 5, 15}
        assert all(s - p * h in (13, p * (h // 2)) for p, s, o, c, f in g) and 13 != (w + 1) * (h // 2)
        assert {(c, f) for p, s, o, c, f in g} == {(c, f) for c in (0, 2) for f in (0, 1, 3)}
        assert {(o, f) for p, s, o, c, f in g} == {(o, f) for o in (1, 5, 15) for f in (0, 1, 3)}
        assert {(p - w, f) for p, s, o, c, f in g} == {(d, f) for d in (1, 7, 64) for f in (0, 1, 3)}
        assert {(s - p * h == 13, f) for p, s, o, c, f in g} == {(t, f) for t in (True, False) for f in (0, 1, 3)}
        # no layout has 16-byte aligned rows and none is packed: a stride is neither w * h nor pitch * h
        assert all(s not in (w * h, p * h) and o % 16 for p, s, o, c, f in g)


def test_poison_patterns():
    assert lb.pattern_bytes(0xEE, 5).tolist() == [0xEE] * 5
    word = lb.pattern_bytes(lb.NAN_WORD, 10)
    assert word.tolist() == [0xCD, 0xAB, 0xC0, 0x7F, 0xCD, 0xAB, 0xC0, 0x7F, 0xCD, 0xAB]
    assert np.isnan(lb.pattern_bytes(lb.NAN_WORD, 8).view("<f4")).all() and lb.pattern_bytes(lb.ALT_WORD, 4).view("<f4")[0] == 1000.0
    assert lb.GUARD >= 256 and lb.STAGE_BYTES == 64 << 20


@pytest.mark.parametrize("w,h", lb.SHAPES[:4])
def test_the_oracle_is_indifferent_to_the_layout(oracle, w, h):
    blob = oracle.synth_blob(21, 1.0)
    lum = lb.frames(900 + w, w, h, 2)
    want = [oracle.resi_vectors(blob, lum[t], w, h) for t in range(2)]
    for pitch, fs, off, chunk, first in lb.solo_geometries(w, h)[::7]:
        for fill in lb.LUMA_FILL:
            buf = lb.lay_out(lum, pitch, fs, off, fill)
            for t in range(2):
                got = oracle.resi_vectors(blob, buf[off + t * fs:], w, h, pitch=pitch)
                assert np.array_equal(got.view(np.uint32), want[t].view(np.uint32)), (pitch, fs, off, fill, t)


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = text.index("### 25.1 Caller-owned buffers the suite reaches")
    end = text.find("\n## ", at)
    rows = []
    for line in text[at: end if end > 0 else len(text)].splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) == 5 and cells[0].startswith("`ethcnn_"):
            rows.append(cells)
    return rows


def test_the_design_table_is_the_list_the_gpu_module_runs():
    rows = _design_rows()
    assert [(r[0].strip("`"), r[1].strip("`"), int(r[3].split()[0])) for r in rows] == lb.POINTER_ROWS
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_ldp_buffers.py")).read()
    have = set(re.findall(r"^def (test_\w+)\(", gpu, re.M))
    for r in rows:
        named = re.findall(r"`(test_\w+)`", r[4])
        assert named, "no test named for %s %s" % (r[0], r[1])
        assert set(named) <= have, (r[0], r[1], sorted(set(named) - have))
        # the accesses name a file and a line of the library's sources that exist
        for path, line in re.findall(r"`(ethcnn_\w+\.(?:hip|h|cpp)):(\d+)`", r[2]):
            src = open(os.path.join(ROOT, "hevc-complexity-reduction_amd", "csrc", path)).read().splitlines()
            assert int(line) <= len(src), (path, line)
    assert "lb.REFUSAL_ROWS" in gpu and [r for r in lb.POINTER_ROWS if r[2] > 1] == lb.REFUSAL_ROWS


def test_every_refusal_is_written_into_the_header():
    hdr = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    for entry in sorted({r[0] for r in lb.POINTER_ROWS}):
        assert entry in hdr
    assert hdr.count("16-byte aligned") >= 4 and "d_vec 4 bytes" in hdr and "d_state_out 16 bytes" in hdr
