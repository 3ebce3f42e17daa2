"""CPU: what the batch form of the offline Low-Delay-P call (include/ethcnn.h "config #5 offline, batch form") settles without a GPU:
the exported symbols, the memory sum, the chunk and block plan, and the driver's handling of --list."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ethcnn_ldp_batch_create", "ethcnn_ldp_batch_destroy", "ethcnn_ldp_batch_last_error", "ethcnn_ldp_batch_bundles",
       "ethcnn_ldp_batch_load_lstm_checkpoint", "ethcnn_ldp_batch_load_lstm_blob", "ethcnn_ldp_batch_load_lstm_synthetic",
       "ethcnn_ldp_batch_get_lstm_blob", "ethcnn_ldp_batch_run_device", "ethcnn_ldp_batch_get_state", "ethcnn_ldp_batch_state_ctus",
       "ethcnn_ldp_batch_set_chunk", "ethcnn_ldp_batch_bytes", "ethcnn_ldp_batch_plan",
       "ethcnn_replay_batch_bytes", "ethcnn_replay_batch_device", "ethcnn_replay_batch_feed_calib", "ethcnn_replay_batch_feed_sim"]
MIXED = [(64, 64), (200, 136), (416, 240), (1920, 1080)]


def _nctu(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def test_the_batch_symbols_are_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ethcnn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ethcnn_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in NEW:
        assert name in declared, "include/ethcnn.h does not declare %s" % name
        assert hasattr(lib, name), "libethcnn.so lacks %s" % name
        assert name in pkg.ethcnn.SIGNATURES
    assert {n for n in declared if n.startswith("ethcnn_ldp_batch_") or n.startswith("ethcnn_replay_batch_")} == set(NEW)
    assert "ethcnn_ldp_batch_seq" in text and ctypes.sizeof(pkg.ethcnn.LdpBatchSeq) == 64  # (the C struct on LP64)
    for name in ("LdpBatch", "ldp_batch_bytes", "ldp_batch_plan"):
        assert hasattr(pkg.ethcnn, name)
    assert pkg.LdpBatch is pkg.ethcnn.LdpBatch
    for name in ("load_lstm_checkpoint", "load_lstm_blob", "load_lstm_synthetic", "get_lstm_blob", "run_device", "run", "get_state", "set_chunk"):
        assert hasattr(pkg.LdpBatch, name), name
    assert hasattr(pkg.Replay, "run_batch") and hasattr(pkg.Replay, "run_batch_device")
    import inspect
    assert {"batch", "bundle_of"} <= set(inspect.signature(pkg.Replay.feed).parameters)


def _formula(sizes, nframes, chunk):
    """the documented sum: sum_j min(nframes_j, Fc) nctu_j 1792 + sum_j roundup16(nctu_j) 3584, Fc = chunk or max(1, 256 MB // sum_j
    nctu_j 1792)"""
    n = [_nctu(w, h) for w, h in sizes]
    fc = chunk if chunk > 0 else max(1, (256 << 20) // (sum(n) * 1792))
    return sum(min(f, fc) * k * 1792 for f, k in zip(nframes, n)) + sum((k + 15) // 16 * 16 * 3584 for k in n)


@pytest.mark.parametrize("chunk", [0, 1, 7])
@pytest.mark.parametrize("nframes", [[1, 1, 1, 1], [5, 5, 5, 5], [100000] * 4, [1, 5, 100000, 5]])
def test_batch_bytes_is_the_documented_sum(pkg, chunk, nframes):
    f = pkg.ethcnn.ldp_batch_bytes
    ws, hs = [s[0] for s in MIXED], [s[1] for s in MIXED]
    assert f(ws, hs, nframes, chunk) == _formula(MIXED, nframes, chunk)
    for j in range(4):  # and every size alone
        assert f(ws[j:j + 1], hs[j:j + 1], nframes[j:j + 1], chunk) == _formula(MIXED[j:j + 1], nframes[j:j + 1], chunk)
    # 100000 frames of the four sizes do not fit 256 MB: the default chunk cuts them (1 + 12 + 28 + 510 = 551 CTUs a frame -> 271 frames)
    if chunk == 0 and nframes == [100000] * 4:
        assert f(ws, hs, nframes, 0) == _formula(MIXED, [271] * 4, 1 << 30) == 271 * 551 * 1792 + (16 + 16 + 32 + 512) * 3584


def test_batch_bytes_refuses_bad_arguments(pkg):
    f = pkg.ethcnn.ldp_batch_bytes
    for args in (([0], [64], [1], 0), ([64], [0], [1], 0), ([64], [64], [0], 0), ([64], [64], [1], -1), ([], [], [], 0), ([64] * 33, [64] * 33, [1] * 33, 0),
                 ([64, -5], [64, 64], [1, 1], 0), ([64, 64], [64, 64], [1, -1], 0)):
        assert f(*args) < 0, args
    assert f([64] * 32, [64] * 32, [1] * 32, 0) == 32 * (1792 + 16 * 3584)


def _blocks(n):
    g = (n + 15) // 16
    return (g, (g + 1) // 2, (g + 3) // 4)


@pytest.mark.parametrize("n", [1, 12, 17, 65, 1056])
def test_plan_blocks_of_one_sequence(pkg, n):
    plan = pkg.ethcnn.ldp_batch_plan([n], [3])
    assert plan["chunks"] == [{"members": 1, "blocks": _blocks(n)}]
    g = (n + 15) // 16
    assert sum(plan["chunks"][0]["blocks"]) == g + -(-g // 2) + -(-g // 4)
    assert _blocks(1) == (1, 1, 1) and _blocks(17) == (2, 1, 1) and _blocks(65) == (5, 3, 2) and _blocks(1056) == (66, 33, 17)


def test_plan_chunks_drop_the_sequences_that_have_ended(pkg):
    nctus, nframes = [1, 12, 17, 65, 1056], [1, 2, 5, 3, 2]
    plan = pkg.ethcnn.ldp_batch_plan(nctus, nframes, chunk_frames=2)
    assert plan["chunk_frames"] == 2 and len(plan["chunks"]) == 3
    for t, chunk in enumerate(plan["chunks"]):
        alive = [n for n, f in zip(nctus, nframes) if f > 2 * t]
        assert chunk["members"] == len(alive)
        assert chunk["blocks"] == tuple(sum(_blocks(n)[lv] for n in alive) for lv in range(3)), t
    assert [c["members"] for c in plan["chunks"]] == [5, 2, 1]
    one = pkg.ethcnn.ldp_batch_plan(nctus, nframes, chunk_frames=1)
    assert [c["members"] for c in one["chunks"]] == [5, 4, 2, 1, 1]


def test_plan_default_chunk(pkg):
    f = pkg.ethcnn.ldp_batch_plan
    for nctus in ([1], [510], [1, 12, 28, 510], [4096] * 32, [1 << 20]):
        want = max(1, (256 << 20) // (sum(nctus) * 1792))
        plan = f(nctus, [100000] * len(nctus))
        assert plan["chunk_frames"] == want and len(plan["chunks"]) == -(-100000 // want), nctus
    assert f([1 << 20], [3])["chunk_frames"] == 1  # (a frame of 2^20 CTUs alone is above 256 MB: one frame per chunk)
    assert f([12, 12], [5, 9], chunk_frames=4)["chunk_frames"] == 4
    for bad in (([0], [1], 0), ([1], [0], 0), ([1], [1], -1), ([], [], 0), ([1] * 33, [1] * 33, 0)):
        with pytest.raises(pkg.EthCnnError):
            f(*bad)


# ---------------------------------------------------------------------------------------------------------------------- driver ---
@pytest.fixture()
def driver(pkg):
    return importlib.import_module("hevc-complexity-reduction_amd.resi_video_to_cu_depth_LDP")


def _yuv(path, w, h, frames):
    np.zeros(w * h * 3 // 2 * frames, np.uint8).tofile(str(path))
    return str(path)


def test_driver_parses_a_list(driver, tmp_path):
    a, b = _yuv(tmp_path / "a.yuv", 128, 64, 4), _yuv(tmp_path / "b.yuv", 200, 136, 2)
    lst = tmp_path / "set.txt"
    lst.write_text("# an evaluation set\n%s 128 64 32 %s\n\n  %s 200 136 22 %s  \n" % (a, tmp_path / "a.dat", b, tmp_path / "b.dat"))
    assert driver.parse_list(str(lst)) == [(a, 128, 64, 32, str(tmp_path / "a.dat"), 3), (b, 200, 136, 22, str(tmp_path / "b.dat"), 1)]


def test_driver_refuses_a_bad_list_before_a_gpu_is_opened(driver, tmp_path, capsys):
    """every refusal returns 1 with a message and writes nothing; none of them reaches the point where a context is created (on a
    machine without a GPU that would be another error text)"""
    a = _yuv(tmp_path / "a.yuv", 128, 64, 4)
    out = str(tmp_path / "o.dat")
    good = "%s 128 64 32 %s\n" % (a, out)
    cases = [("%s 128 64 32\n" % a, "RESI_YUV WIDTH HEIGHT QP OUT"),
             (good + "%s 128 sixty-four 32 %s.2\n" % (a, out), "numbers"),
             ("%s 128 64 32 %s extra\n" % (a, out), "RESI_YUV WIDTH HEIGHT QP OUT"),
             ("%s 48 64 32 %s\n" % (a, out), "below"),
             ("%s 128 32 32 %s\n" % (a, out), "below"),
             (good + "%s 128 64 22 %s.2\n" % (tmp_path / "none.yuv", out), "cannot read"),
             ("%s 192 64 32 %s\n" % (a, out), "size"),
             (good + good, "same output"),
             ("".join("%s 128 64 32 %s.%d\n" % (a, out, i) for i in range(33)), "more than 32"),
             ("# nothing\n", "no sequence")]
    lst = str(tmp_path / "set.txt")
    for text, msg in cases:
        with open(lst, "w") as f:
            f.write(text)
        assert driver.main(["drv", "--list", lst]) == 1, text
        assert msg in capsys.readouterr().err, text
    assert driver.main(["drv", "--list", str(tmp_path / "missing.txt")]) == 1
    assert "cannot read" in capsys.readouterr().err
    with open(lst, "w") as f:
        f.write(good)
    for extra in (["--also", a, "22", out + ".2"], ["--state-out", out + ".s"], ["--frames", "2"], ["--chunk", "-1"], ["--piece-frames", "-1"]):
        assert driver.main(["drv", "--list", lst] + extra) == 1, extra
        capsys.readouterr()
    assert driver.main(["drv", a, "128", "64", "32", "--list", lst]) == 1
    assert driver.main(["drv"]) == 2  # argparse: neither a sequence nor a list
    capsys.readouterr()
    assert sorted(os.listdir(str(tmp_path))) == ["a.yuv", "set.txt"]
