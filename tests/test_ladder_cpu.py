"""CPU: the host-only part of the ladder search (include/ethcnn.h "search budget: building a ladder") -- the entries the header declares,
the layout of ethcnn_ladder_rung, the argument rules, the thinning against the restatement in tests/ladder_ref.py (Python integers), the
ladder file written by the library and read back by the parser every launcher uses -- and the refusals of tools/build_ladder.py, of the
All-Intra launcher and of both Low-Delay-P daemons under a bad ETHCNN_SEARCH_BUDGET_LADDER, which come before a GPU is touched.  The
kernel and the end-to-end runs are in tests/test_gpu_ladder.py."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ladder_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "build_ladder.py")
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
PY_DAEMON = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
C_DAEMON = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "resi_to_cu_depth_ldp")
ENTRIES = ("check", "build", "thin", "write")
COMPANION = {"ai": "0.75 0.25 0.75 0.25 0.75 0.25", "ldp": "0.25 0.75 0.25 0.75 0.25 0.75"}


def _control_tool():
    spec = importlib.util.spec_from_file_location("control_budget", os.path.join(ROOT, "tools", "control_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_library_and_binding_carry_exactly_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "search budget: building a ladder" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\bint (ethcnn_ladder_\w+)\(", code))
    assert declared == {"ethcnn_ladder_" + n for n in ENTRIES}
    assert set(re.findall(r"\b(ethcnn_ladder_\w+)\(", code)) == declared
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in declared:
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    e = pkg.ethcnn
    assert callable(pkg.PartitionSim.build_ladder)
    for name in ("ladder_check", "ladder_thin", "ladder_write"):
        assert callable(getattr(e, name))


def test_rung_layout_matches_the_documented_one(pkg, tmp_path):
    want = {"thr": (0, 24), "coord": (24, 4), "value": (28, 4), "checked": (32, 32), "bad_ctus": (64, 8)}
    dt = pkg.ethcnn.LADDER_RUNG
    assert dt.itemsize == 72 and {n: (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ethcnn.h"\nint main(void) {\n  printf("%zu", sizeof(ethcnn_ladder_rung));\n' +
                   "".join('  printf(" %%zu", offsetof(ethcnn_ladder_rung, %s));\n' % n for n in dt.names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [72] + [want[n][0] for n in dt.names]


def test_check_agrees_with_the_argument_rules(pkg):
    e = pkg.ethcnn
    lib = pkg.load_library()
    w = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
    for grid in range(-2, 1030):
        want = 0 if grid in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) else e.ERR_ARG
        assert lib.ethcnn_ladder_check(w, grid, 4096, 10 ** 6) == want, grid
    for max_rungs, want in ((1, 0), (4096, 0), (0, e.ERR_ARG), (4097, e.ERR_ARG), (-1, e.ERR_ARG), (2 ** 40, e.ERR_ARG)):
        assert lib.ethcnn_ladder_check(w, 8, max_rungs, 5) == want, max_rungs
    for ppm, want in ((0, 0), (10 ** 6, 0), (10 ** 6 + 1, e.ERR_ARG), (2 ** 32 - 1, e.ERR_ARG)):
        assert lib.ethcnn_ladder_check(w, 8, 64, ppm) == want, ppm
    assert lib.ethcnn_ladder_check(None, 8, 64, 5) == 0     # NULL weight: the default
    for d in range(4):
        wbig = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
        wbig[d] = 2 ** 32
        assert lib.ethcnn_ladder_check(wbig, 8, 64, 5) == e.ERR_ARG and "weight[%d]" % d in lib.ethcnn_last_error(None).decode()
        wbig[d] = 2 ** 32 - 1
        assert lib.ethcnn_ladder_check(wbig, 8, 64, 5) == 0
    # the binding's form and the restatement's
    e.ladder_check()
    e.ladder_check((1, 0, 0, 0), 1, 1, 0)
    for args in (((64, 16, 4, 2 ** 32),), (None, 3), (None, 0), (None, 2048), (None, 8, 0), (None, 8, 4097), (None, 8, 64, 10 ** 6 + 1)):
        with pytest.raises(pkg.EthCnnError) as err:
            e.ladder_check(*args)
        assert err.value.code == e.ERR_ARG
        with pytest.raises(ValueError):
            lref.check(*(list(args) + [None, 8, 64, 5][len(args):]))
    # a NULL simulator never reaches a GPU; the outputs stay as they were
    rungs, n = np.full(2, 7, e.LADDER_RUNG), ctypes.c_int64(-5)
    assert lib.ethcnn_ladder_build(None, w, 8, 2, 5, rungs.ctypes.data, ctypes.byref(n)) == e.ERR_ARG
    assert n.value == -5 and (rungs["coord"] == 7).all()


def _thin_both(e, cost, k):
    got = e.ladder_thin(cost, k).tolist()
    assert got == lref.thin(cost, k), (len(cost), k)
    return got


def _falling(rng, n, hi):
    return sorted({int(x) for x in rng.integers(0, hi, size=4 * n, dtype=np.uint64)}, reverse=True)[:n]


def test_thin_agrees_with_the_restatement_and_keeps_its_promises(pkg):
    e = pkg.ethcnn
    rng = np.random.default_rng(17)
    dup = 0
    for n in (1, 2, 3, 7, 64, 340):
        for hi in (50 * n, 10 ** 6, 2 ** 62):
            cost = _falling(rng, n, hi)
            n_got = len(cost)
            for k in sorted({1, 2, 3, max(1, n_got - 1), n_got, n_got + 1, 33, 4096}):
                got = _thin_both(e, cost, k)
                assert got == sorted(set(got)) and len(got) <= min(k, n_got) and got[0] == 0
                if k == 1 and n_got > 1:
                    assert got == [0]
                if k >= 2:
                    assert got[-1] == n_got - 1                       # the cheapest rung is always kept
                if n_got <= k:
                    assert got == list(range(n_got))                  # the identity
                dup += n_got > k >= 2 and len(got) < k
    # plateaus in target space: one steep step, so that several targets pick the same rung
    cost = [10 ** 9, 10 ** 9 - 1, 10 ** 9 - 2, 5, 4, 3, 2, 1, 0]
    for k in (2, 3, 4, 5, 8):
        got = _thin_both(e, cost, k)
        dup += len(got) < k
    assert _thin_both(e, cost, 5) == [0, 3, 8]
    assert dup
    # costs near 2^64: the product j * (cost[0] - cost[n-1]) needs 128 bits
    top = 2 ** 64 - 1
    cost = [top - i * (2 ** 58) - i * i for i in range(60)]
    for k in (2, 7, 33, 59):
        _thin_both(e, cost, k)
    cost = [top, top - 1, 2 ** 63, 3, 0]
    for k in (1, 2, 3, 4, 5):
        _thin_both(e, cost, k)


def test_thin_refuses_costs_that_do_not_fall_and_bad_arguments(pkg):
    e = pkg.ethcnn
    lib = pkg.load_library()
    for cost in ([5, 5], [9, 7, 8], [1, 2], [3, 2, 2], [0, 0, 0]):
        for k in (1, 2, 3, 10):   # also where n <= K would be the identity
            with pytest.raises(pkg.EthCnnError) as err:
                e.ladder_thin(cost, k)
            assert err.value.code == e.ERR_ARG and "fall strictly" in str(err.value)
            with pytest.raises(ValueError):
                lref.thin(cost, k)
    c = np.array([9, 5, 1], np.uint64)
    idx, k = np.full(3, -7, np.int32), ctypes.c_int64(-9)
    for args in ((None, 3, 2), (c.ctypes.data, 0, 2), (c.ctypes.data, -1, 2), (c.ctypes.data, 3, 0), (c.ctypes.data, 3, -4)):
        assert lib.ethcnn_ladder_thin(*(args + (idx.ctypes.data, ctypes.byref(k)))) == e.ERR_ARG, args[1:]
    assert lib.ethcnn_ladder_thin(c.ctypes.data, 3, 2, None, ctypes.byref(k)) == e.ERR_ARG
    assert lib.ethcnn_ladder_thin(c.ctypes.data, 3, 2, idx.ctypes.data, None) == e.ERR_ARG
    bad = np.array([9, 9, 1], np.uint64)
    assert lib.ethcnn_ladder_thin(bad.ctypes.data, 3, 2, idx.ctypes.data, ctypes.byref(k)) == e.ERR_ARG
    assert (idx == -7).all() and k.value == -9
    assert lib.ethcnn_ladder_thin(c.ctypes.data, 3, 2, idx.ctypes.data, ctypes.byref(k)) == 0 and k.value == 2 and idx[:2].tolist() == [0, 2]


@pytest.mark.parametrize("order", ["ai", "ldp"])
def test_written_ladders_read_back_over_every_grid_value(pkg, tmp_path, order):
    e = pkg.ethcnn
    tool = _control_tool()
    sb = tool._sb
    k = np.arange(1026)
    # every up value 0..1024 and every down value -1..1024 on every level, 1026 rungs
    up = np.stack([k % 1025, (1024 - k) % 1025, (k * 7) % 1025], axis=1)
    down = np.stack([k - 1, (k * 5 + 1) % 1026 - 1, (1025 - k) - 1], axis=1)
    for l in range(3):
        assert set(up[:, l].tolist()) == set(range(1025)) and set(down[:, l].tolist()) == set(range(-1, 1025))
    thr = e.sim_thr(up, down)
    path = str(tmp_path / "ladder.txt")
    e.ladder_write(path, thr, order)
    assert open(path).read() == lref.ladder_lines(up, down, order)
    for reader in (tool.read_ladder, sb.read_ladder):
        got_up, got_down = reader(path, order)
        assert np.array_equal(np.array(got_up), up) and np.array_equal(np.array(got_down), down)
    # the first rung has up_k[0] = 0 and down_k[0] = -1: ten decimals hold -1 / 1024 exactly
    assert open(path).readline().split()[:2] == (["0.0000000000", "-0.0009765625"] if order == "ai" else ["-0.0009765625", "0.0000000000"])
    # the other order reads the same file as something else (or refuses it): the order is part of the file's meaning
    other = "ldp" if order == "ai" else "ai"
    try:
        assert not np.array_equal(np.array(sb.read_ladder(path, other)[0]), up)
    except ValueError:
        pass
    assert sorted(os.listdir(str(tmp_path))) == ["ladder.txt"]       # no temp file is left
    # refusals: nothing is written
    lib = pkg.load_library()
    one = e.sim_thr([[1024, 1024, 1024]], [[-1, -1, -1]])
    gone = str(tmp_path / "gone.txt")
    assert lib.ethcnn_ladder_write(None, one.ctypes.data, 1, 0) == e.ERR_ARG and lib.ethcnn_ladder_write(os.fsencode(gone), None, 1, 0) == e.ERR_ARG
    many = np.ascontiguousarray(np.resize(one, 4097))
    for kk, o in ((0, 0), (4097, 0), (1, 2), (1, -1)):
        assert lib.ethcnn_ladder_write(os.fsencode(gone), many.ctypes.data, kk, o) == e.ERR_ARG
    bad = e.sim_thr([[1024, 1025, 1024]], [[-1, -1, -1]])
    assert lib.ethcnn_ladder_write(os.fsencode(gone), bad.ctypes.data, 1, 0) == e.ERR_ARG
    with pytest.raises(ValueError):
        e.ladder_write(gone, one, "both")
    with pytest.raises(pkg.EthCnnError):
        e.ladder_write(str(tmp_path / "no_such_dir" / "x.txt"), one, order)
    assert sorted(os.listdir(str(tmp_path))) == ["ladder.txt"]


def test_env_parser_names_what_is_wrong(pkg, tmp_path, monkeypatch):
    sb = _control_tool()._sb
    monkeypatch.delenv("ETHCNN_SEARCH_BUDGET_LADDER", raising=False)
    assert sb.ladder_from_env("ai") is None
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_LADDER", "")
    assert sb.ladder_from_env("ldp") is None
    good = tmp_path / "good.txt"
    good.write_text("1 -0.0009765625 1 0 0.5 0.25\n\n0.5 0.25 0.5 0.25 0.5 0.25\n")
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_LADDER", str(good))
    assert sb.ladder_from_env("ai") == ([[1024, 1024, 512], [512, 512, 512]], [[-1, 0, 256], [256, 256, 256]])
    with pytest.raises(ValueError) as err:                  # the same file in the other order: -1 / 1024 is no up
        sb.ladder_from_env("ldp")
    assert "ETHCNN_SEARCH_BUDGET_LADDER" in str(err.value) and "line 1" in str(err.value)
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_LADDER", str(tmp_path / "absent.txt"))
    with pytest.raises(ValueError) as err:
        sb.ladder_from_env("ai")
    assert "absent.txt" in str(err.value) and "cannot be read" in str(err.value)


def _bad_ladders(tmp_path):
    """name -> the word its refusal carries"""
    (tmp_path / "five.txt").write_text("1 0 1 0 1\n")
    (tmp_path / "high.txt").write_text("1 0 1 0 1 0\n1.5 1.5 1 0 1 0\n")
    (tmp_path / "word.txt").write_text("1 0 1 0 one 0\n")
    (tmp_path / "nan.txt").write_text("1 0 1 0 nan 0\n")
    (tmp_path / "empty.txt").write_text("\n\n")
    (tmp_path / "long.txt").write_text("0.5 0.5 0.5 0.5 0.5 0.5\n" * 4097)
    return (("five.txt", "line 1"), ("high.txt", "line 2"), ("word.txt", "line 1"), ("nan.txt", "line 1"), ("empty.txt", "rungs, got 0"),
            ("long.txt", "rungs, got 4097"), ("absent.txt", "cannot be read"))


def _run(cmd, cwd, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run(cmd, cwd=str(cwd), env=e, capture_output=True, text=True, timeout=120)


def test_launcher_refuses_a_bad_ladder_before_a_gpu_is_touched(tmp_path):
    np.zeros(64 * 64 * 3 // 2, np.uint8).tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text(COMPANION["ai"] + "\n")
    bad = _bad_ladders(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    for name, word in bad:
        r = _run([sys.executable, LAUNCHER, "seq.yuv", "64", "64", "32"], tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4",
                 ETHCNN_SEARCH_BUDGET_LADDER=name)
        assert r.returncode == 1 and "video_to_cu_depth: ETHCNN_SEARCH_BUDGET_LADDER" in r.stderr and name in r.stderr and word in r.stderr, (name, r.stderr[-300:])
        assert "Traceback" not in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == before      # no cu_depth.dat, no temp file


@pytest.mark.parametrize("which", ["python", "native"])
def test_daemons_refuse_a_bad_ladder_before_a_gpu_is_touched(pkg, tmp_path, which):
    """both daemons, the same rules and the same words: exit status 1, no signal file, no cu_depth.dat"""
    prog = "resi_to_cu_depth_LDP" if which == "python" else "resi_to_cu_depth_ldp"
    cmd = ([sys.executable, PY_DAEMON, "--python"] if which == "python" else [C_DAEMON, "--quiet"]) + ["--max-frames", "0", "--idle-timeout", "0"]
    (tmp_path / "Thr_info.txt").write_text(COMPANION["ldp"] + "\n")
    bad = _bad_ladders(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    for name, word in bad:
        r = _run(cmd, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER=name)
        assert r.returncode == 1 and (prog + ": ETHCNN_SEARCH_BUDGET_LADDER") in r.stderr and name in r.stderr and word in r.stderr, (name, r.stderr[-300:])
        assert "Traceback" not in r.stderr
    # a ladder that is fine in All-Intra order has a down above an up's range in Low-Delay-P order only when a value leaves [0, 1]: -1/1024
    # as an "up" is refused, with the line
    (tmp_path / "ai.txt").write_text("1 -0.0009765625 1 0 1 0\n")
    r = _run(cmd, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="ai.txt")
    assert r.returncode == 1 and "line 1: thresholds outside" in r.stderr
    os.remove(str(tmp_path / "ai.txt"))
    assert sorted(os.listdir(str(tmp_path))) == before
    # a ladder as the library writes it is accepted: whatever happens next is not that refusal; without a budget the variable is not read
    pkg.ethcnn.ladder_write(str(tmp_path / "good.txt"), pkg.ethcnn.budget_default_ladder()[::8], "ldp")
    r = _run(cmd, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="good.txt")
    assert "ETHCNN_SEARCH_BUDGET_LADDER" not in r.stderr and "companion" not in r.stderr, r.stderr[-300:]
    r = _run(cmd, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET_LADDER="five.txt")
    assert "ETHCNN_SEARCH_BUDGET_LADDER" not in r.stderr, r.stderr[-300:]
    assert "pred_end.sig" not in os.listdir(str(tmp_path)) and "cu_depth.dat" not in os.listdir(str(tmp_path))


def test_tool_refuses_before_a_gpu_is_touched(tmp_path):
    np.zeros((12, 21), "<f4").tofile(str(tmp_path / "p.dat"))
    np.zeros((9 * 13,), np.uint8).tofile(str(tmp_path / "l.dat"))
    nolabels = ["--case", "-", "p.dat", "208", "144"]
    case = ["--case", "l.dat", "p.dat", "208", "144"]
    tool = lambda args: subprocess.run([sys.executable, TOOL] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    for args, word in ((nolabels, "labels"), (["--out", "lad.txt", "--order", "ai"] + nolabels, "labels"), (["--grid", "3"] + case, "--grid"),
                       (["--grid", "2048"] + case, "--grid"), (["--grid", "0"] + case, "--grid"), (["--max-bad-ppm", "1000001"] + case, "--max-bad-ppm"),
                       (["--max-bad-ppm", "-1"] + case, "--max-bad-ppm"), (["--rungs", "0"] + case, "--rungs"), (["--rungs", "4097"] + case, "--rungs"),
                       (["--weights", "1", "2", "3", "4294967296"] + case, "--weights"), (["--weights", "1", "2", "3", "-4"] + case, "--weights")):
        r = tool(args)
        assert r.returncode == 1 and "build_ladder.py: error:" in r.stderr and word in r.stderr and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    # a command line of the wrong form: the usage text, status 2, as the sibling tools
    for args in ([], ["--out", "lad.txt"] + case, ["--out", "lad.txt", "--order", "both"] + case, ["--grid", "eight"] + case, ["--grid"], ["--weights", "1", "2", "3"],
                 ["--weights", "a", "b", "c", "d"] + case, ["--help"]):
        r = tool(args)
        assert r.returncode == 2 and "build_ladder.py" in r.stderr and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    assert sorted(os.listdir(str(tmp_path))) == ["l.dat", "p.dat"]   # no output, no temp file
