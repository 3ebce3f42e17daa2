"""CPU: the host side of high-bit-depth and non-4:2:0 sources (include/ethcnn.h): the narrowing rule min(s >> (bit_depth - 8), 255) on
the host, the frame sizes of the source formats, argument validation that needs no device, and the launcher's environment parsing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = list(range(8, 17))


def rule(s, bd):
    return np.minimum(s.astype(np.uint32) >> (bd - 8), 255).astype(np.uint8)


@pytest.mark.parametrize("bd", DEPTHS)
def test_every_sample_value_at_every_depth(pkg, bd):
    """all 65536 values through the SSE2 body (and, placed behind a multiple of 16, through the scalar tail)"""
    f = pkg.ethcnn.narrow_rows_host
    s = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(f(s, bd), rule(s, bd))
    for start in range(16):  # every value also in the tail: 65521 = 16 * 4095 + 1 samples, the last one alone behind the body
        t = np.roll(s, start)[:65521]
        assert np.array_equal(f(t, bd), rule(t, bd))
    tail = np.concatenate([np.zeros(16, np.uint16), s[-15:]])  # the largest values in a 15-sample tail
    assert np.array_equal(f(tail, bd), rule(tail, bd))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000])
@pytest.mark.parametrize("bd", DEPTHS)
def test_lengths_cover_body_and_tail(pkg, n, bd):
    rng = np.random.default_rng(100 * bd + n)
    s = rng.integers(0, 65536, size=n + 1, dtype=np.uint16)
    s[rng.integers(0, n)] = 65535
    for off in (0, 1):  # an odd sample offset: the source is then not 16-byte aligned
        got = pkg.ethcnn.narrow_rows_host(s[off:off + n], bd)
        assert got.dtype == np.uint8 and np.array_equal(got, rule(s[off:off + n], bd))


def test_narrow_rows_host_writes_only_n_bytes_and_checks_its_arguments(pkg):
    lib = pkg.load_library()
    src = np.full(40, 1023, dtype=np.uint16)
    dst = np.full(64, 0xAB, dtype=np.uint8)
    assert lib.ethcnn_narrow_rows_host(src.ctypes.data, dst.ctypes.data + 3, 37, 10) == 0
    assert np.all(dst[:3] == 0xAB) and np.all(dst[3:40] == 255) and np.all(dst[40:] == 0xAB)
    for bd in (7, 17, 0, -1):
        assert lib.ethcnn_narrow_rows_host(src.ctypes.data, dst.ctypes.data, 4, bd) == pkg.ethcnn.ERR_ARG
        with pytest.raises(pkg.EthCnnError):
            pkg.ethcnn.narrow_rows_host(src, bd)
    assert lib.ethcnn_narrow_rows_host(None, dst.ctypes.data, 4, 10) == pkg.ethcnn.ERR_ARG
    assert lib.ethcnn_narrow_rows_host(None, None, 0, 10) == 0


def test_source_frame_bytes(pkg):
    f = pkg.ethcnn.source_frame_bytes
    for (w, h) in ((416, 240), (200, 136), (1920, 1080), (64, 64)):
        n = w * h
        assert f(w, h) == (n, n * 3 // 2) == f(w, h, 8, 420)
        assert f(w, h, 8, 400) == (n, n) and f(w, h, 8, 422) == (n, 2 * n) and f(w, h, 8, 444) == (n, 3 * n)
        assert f(w, h, 10, 400) == (2 * n, 2 * n) and f(w, h, 10, 420) == (2 * n, 3 * n)
        assert f(w, h, 10, 422) == (2 * n, 4 * n) and f(w, h, 10, 444) == (2 * n, 6 * n)
        assert f(w, h, 16, 420) == f(w, h, 9, 420) == (2 * n, 3 * n)
    # 8-bit 4:2:0 is the reference's width * height * 3 // 2, odd sizes included
    for (w, h) in ((201, 135), (3, 3), (1, 1), (5, 4)):
        assert f(w, h, 8, 420) == (w * h, w * h * 3 // 2)
    # odd subsampled dimensions elsewhere
    for args in ((201, 136, 10, 420), (200, 135, 10, 420), (201, 136, 8, 422), (201, 136, 10, 422), (201, 135, 12, 420)):
        with pytest.raises(pkg.EthCnnError) as ei:
            f(*args)
        assert ei.value.code == pkg.ethcnn.ERR_ARG
    assert f(200, 135, 10, 422) == (2 * 200 * 135, 4 * 200 * 135)  # 4:2:2 halves the width only
    assert f(201, 135, 10, 444) == (2 * 201 * 135, 6 * 201 * 135) and f(201, 135, 10, 400) == (2 * 201 * 135,) * 2
    for args in ((64, 64, 7, 420), (64, 64, 17, 420), (64, 64, 8, 411), (64, 64, 8, 0), (0, 64, 8, 420), (64, -1, 8, 420)):
        with pytest.raises(pkg.EthCnnError):
            f(*args)
    lib = pkg.load_library()
    fmt = pkg.ethcnn.SourceFormat(10, 420)
    a = ctypes.c_int64(-5)
    assert lib.ethcnn_source_frame_bytes(ctypes.addressof(fmt), 64, 64, None, ctypes.byref(a)) == 0 and a.value == 3 * 64 * 64  # outputs optional
    assert lib.ethcnn_source_frame_bytes(ctypes.addressof(fmt), 64, 64, ctypes.byref(a), None) == 0 and a.value == 2 * 64 * 64
    assert lib.ethcnn_source_frame_bytes(None, 64, 64, None, ctypes.byref(a)) == pkg.ethcnn.ERR_ARG


def test_entries_reject_a_null_context_without_a_device(pkg):
    """what the ABI can check with no context (a context needs a device): null pointers are argument errors, never a crash"""
    lib, E = pkg.load_library(), pkg.ethcnn.ERR_ARG
    fmt = pkg.ethcnn.SourceFormat(10, 420)
    assert lib.ethcnn_set_source_format(None, ctypes.addressof(fmt)) == E
    assert lib.ethcnn_get_source_format(None, ctypes.addressof(fmt)) == E
    assert lib.ethcnn_set_narrow_chunk(None, 1) == E
    buf = np.zeros(64, np.uint16)
    out = np.zeros(64 * 21, np.float32)
    assert lib.ethcnn_narrow_luma_device(None, buf.ctypes.data, 8, 8, 16, 128, 1, 10, buf.ctypes.data, 16, 128) == E
    assert lib.ethcnn_predict_luma16_device(None, buf.ctypes.data, 8, 8, 16, 128, 1, 10, 32, out.ctypes.data) == E
    assert lib.ethcnn_predict_luma16(None, buf.ctypes.data, 8, 8, 16, 128, 1, 10, 32, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == E


def test_launcher_environment_parsing(pkg, monkeypatch):
    v = pkg.video_to_cu_depth
    monkeypatch.delenv("ETHCNN_INPUT_BIT_DEPTH", raising=False)
    monkeypatch.delenv("ETHCNN_INPUT_CHROMA_FORMAT", raising=False)
    assert v.source_format_from_env() == (8, 420)
    monkeypatch.setenv("ETHCNN_INPUT_BIT_DEPTH", "10")
    assert v.source_format_from_env() == (10, 420)
    monkeypatch.setenv("ETHCNN_INPUT_CHROMA_FORMAT", "444")
    assert v.source_format_from_env() == (10, 444)
    for name, bad in (("ETHCNN_INPUT_BIT_DEPTH", "7"), ("ETHCNN_INPUT_BIT_DEPTH", "ten"), ("ETHCNN_INPUT_BIT_DEPTH", "17"),
                      ("ETHCNN_INPUT_CHROMA_FORMAT", "411"), ("ETHCNN_INPUT_CHROMA_FORMAT", "4:2:0")):
        monkeypatch.setenv("ETHCNN_INPUT_BIT_DEPTH", "10")
        monkeypatch.setenv("ETHCNN_INPUT_CHROMA_FORMAT", "420")
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError, match=name):
            v.source_format_from_env()


def test_launchers_refuse_a_bad_format_before_anything_else(tmp_path):
    """a bad variable value is a non-zero exit with a message and no cu_depth.dat -- decided before a context (a device) is needed"""
    np.zeros(64 * 64 * 3, np.uint8).tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text("0.5 0.5 0.5 0.5 0.5 0.5\n")
    tool = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "video_to_cu_depth")
    for cmd in ([sys.executable, os.path.join(ROOT, "video_to_cu_depth.py")], [tool]):
        for env in ({"ETHCNN_INPUT_BIT_DEPTH": "11bit"}, {"ETHCNN_INPUT_CHROMA_FORMAT": "421"}, {"ETHCNN_INPUT_BIT_DEPTH": "32"}):
            r = subprocess.run(cmd + ["seq.yuv", "64", "64", "32"], cwd=str(tmp_path), capture_output=True, text=True,
                               env=dict(os.environ, ETHCNN_SYNTHETIC_SEED="1", **env))
            assert r.returncode not in (0, -11, -6) and list(env)[0] in r.stderr, (cmd, env, r.stderr)
            assert not (tmp_path / "cu_depth.dat").exists()
