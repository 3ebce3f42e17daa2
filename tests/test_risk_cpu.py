"""No GPU: the host side of the expected wrong decisions (include/ethcnn.h "partition-search simulation: expected wrong decisions") --
the entries and layouts, the identity table, the monotone fit against the restatement (tests/risk_ref.py, fractions.Fraction), the table
file and its refusals, the tools' and launchers' refusals before a GPU is touched -- and one check of the definition itself: with
truth flags drawn from the probabilities, the labelled counters of the simulator's restatement land where the expected ones say."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import decide_ref as dref
import risk_ref as rref
import sim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = {n: os.path.join(ROOT, "tools", n + ".py") for n in ("build_ladder", "simulate_thresholds", "calibrate_thresholds")}
LAUNCHER = os.path.join(ROOT, "video_to_cu_depth.py")
PY_DAEMON = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
C_DAEMON = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "resi_to_cu_depth_ldp")
ENTRIES = ("set_reliability", "eval", "identity", "from_hist", "write", "read", "ladder_build")
COMPANION = {"ai": "0.75 0.25 0.75 0.25 0.75 0.25", "ldp": "0.25 0.75 0.25 0.75 0.25 0.75"}


def test_header_library_and_binding_carry_exactly_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "partition-search simulation: expected wrong decisions" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\bint (ethcnn_risk_\w+)\(", code))
    assert declared == {"ethcnn_risk_" + n for n in ENTRIES}
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in declared:
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    e = pkg.ethcnn
    for name in ("set_reliability", "eval_risk", "build_ladder_risk"):
        assert callable(getattr(pkg.PartitionSim, name))
    for name in ("risk_identity", "risk_from_hist", "risk_read", "risk_write"):
        assert callable(getattr(e, name))
    assert e.RISK_ONE == 1 << 20 == rref.ONE and "#define ETHCNN_RISK_ONE (1u << 20)" in code


def test_layouts_match_the_documented_ones(pkg, tmp_path):
    want = {"thr": (0, 24), "coord": (24, 4), "value": (28, 4), "checked": (32, 32), "exp_wrong_split": (64, 24), "exp_wrong_stop": (88, 24)}
    dt = pkg.ethcnn.LADDER_RUNG_RISK
    assert dt.itemsize == 112 and {n: (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names} == want
    assert pkg.ethcnn.SIM_RISK.itemsize == 48 and pkg.ethcnn.SIM_RISK.names == ("exp_wrong_split", "exp_wrong_stop")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ethcnn.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(ethcnn_sim_risk), offsetof(ethcnn_sim_risk, exp_wrong_stop), sizeof(ethcnn_ladder_rung_risk));\n' +
                   "".join('  printf(" %%zu", offsetof(ethcnn_ladder_rung_risk, %s));\n' % n for n in dt.names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [48, 24, 112] + [want[n][0] for n in dt.names]


def test_identity_table(pkg):
    rel = pkg.ethcnn.risk_identity()
    assert rel.dtype == np.uint32 and rel.shape == (3, 1025)
    assert all(int(rel[l, b]) == b * 1024 for l in range(3) for b in range(1025))
    assert np.array_equal(rel, rref.identity()) and rel[0, 1024] == pkg.ethcnn.RISK_ONE and rel[2, 0] == 0


def _hists():
    """name -> uint64 [3, 2, 1025]; every level of every histogram is a case of its own"""
    rng = np.random.default_rng(21)
    b = np.arange(1025)
    out = {}
    # a calibrated model with noise: violators everywhere; bins without a sample inside and at both ends
    n = rng.integers(0, 400, size=(3, 1025))
    n[:, rng.integers(0, 1025, size=300)] = 0
    n[0, :17] = 0
    n[1, 1000:] = 0
    n[2, :3] = 0
    n[2, 1020:] = 0
    split = rng.binomial(n, b / 1024.0)
    out["noisy"] = np.stack([n - split, split], axis=1).astype(np.uint64)
    # an empty level; a level with unsplit samples only; one with split samples only
    h = out["noisy"].copy()
    h[0] = 0
    h[1, 1] = 0
    h[2, 0] = 0
    out["empty level and single classes"] = h
    # counts near 2^40, a steep and a flat stretch; a single bin with samples
    big = (rng.integers(0, 1 << 40, size=(3, 2, 1025), dtype=np.int64)).astype(np.uint64)
    big[0, 1] = np.sort(big[0, 1])
    big[1, :, 5:900] = 0
    big[2] = 0
    big[2, :, 512] = (3, 1 << 40)
    out["near 2^40"] = big
    # an over-confident model: the true share is flatter than the probability; and a decreasing one, which pools into one block
    n = rng.integers(50, 500, size=(3, 1025))
    split = rng.binomial(n, 0.25 + 0.5 * b / 1024.0)
    split[2] = rng.binomial(n[2], 1.0 - b / 1024.0)
    out["over-confident and decreasing"] = np.stack([n - split, split], axis=1).astype(np.uint64)
    return out


@pytest.mark.parametrize("name", sorted(_hists()))
def test_from_hist_agrees_with_the_restatement(pkg, name):
    hist = _hists()[name]
    got = pkg.ethcnn.risk_from_hist(hist)
    assert got.dtype == np.uint32 and got.shape == (3, 1025)
    assert np.array_equal(got, rref.from_hist(hist)), name
    assert (np.diff(got.astype(np.int64), axis=1) >= 0).all() and got.max() <= pkg.ethcnn.RISK_ONE
    for l in range(3):
        if hist[l].sum() == 0:
            assert np.array_equal(got[l], rref.identity()[l])
        elif hist[l, 1].sum() == 0:
            assert not got[l].any()
        elif hist[l, 0].sum() == 0:
            assert (got[l] == pkg.ethcnn.RISK_ONE).all()
    if name == "over-confident and decreasing":
        assert len(set(got[2].tolist())) == 1 and len(set(got[0].tolist())) > 8    # a decreasing share pools into one block; a rising one keeps steps
    if name == "near 2^40":
        assert len(set(got[2].tolist())) == 1 and got[2, 0] == ((1 << 40) << 20) // ((1 << 40) + 3)


def test_from_hist_refuses_null(pkg):
    lib = pkg.ethcnn.load_library()
    rel = np.zeros((3, 1025), np.uint32)
    assert lib.ethcnn_risk_from_hist(None, rel.ctypes.data) == pkg.ethcnn.ERR_ARG and lib.ethcnn_risk_identity(None) == pkg.ethcnn.ERR_ARG
    with pytest.raises(ValueError):
        pkg.ethcnn.risk_from_hist(np.zeros(7, np.uint64))


def test_table_file_round_trip_and_refusals(pkg, tmp_path):
    e = pkg.ethcnn
    rng = np.random.default_rng(22)
    rel = rng.integers(0, e.RISK_ONE + 1, size=(3, 1025)).astype(np.uint32)
    rel[0, 0], rel[2, 1024] = 0, e.RISK_ONE
    path = str(tmp_path / "rel.txt")
    e.risk_write(path, rel)
    assert open(path).read() == rref.table_text(rel)
    assert np.array_equal(e.risk_read(path), rel)
    assert os.listdir(str(tmp_path)) == ["rel.txt"]                     # no temp file is left
    e.risk_write(path, e.risk_identity())                                 # an existing file is replaced
    assert np.array_equal(e.risk_read(path), rref.identity())
    good = rref.table_text(rel)
    lines = good.splitlines()
    bad = {"truncated": "\n".join(lines[:3]) + "\n", "a value short": good[:good.rstrip().rfind(" ")] + "\n", "cut in a token": good[:len(good) // 2],
           "mis-headed": good.replace("reliability 1", "reliability 2", 1), "no header": "\n".join(lines[1:]) + "\n", "empty": "",
           "a value too many": good + "5\n", "out of range": good.replace(" %d " % rel[1, 7], " %d " % (e.RISK_ONE + 1), 1),
           "negative": good.replace(" %d " % rel[1, 7], " -3 ", 1), "a word": good.replace(" %d " % rel[1, 7], " x7 ", 1),
           "a fraction": good.replace(" %d " % rel[1, 7], " 0.5 ", 1), "huge": good.replace(" %d " % rel[1, 7], " 99999999999999999999 ", 1)}
    keep = np.full((3, 1025), 7, np.uint32)
    lib = e.load_library()
    for name, text in bad.items():
        p = tmp_path / "bad.txt"
        p.write_text(text)
        out = keep.copy()
        assert lib.ethcnn_risk_read(os.fsencode(str(p)), out.ctypes.data) == e.ERR_FORMAT, name
        assert (out == 7).all(), name
        with pytest.raises(pkg.EthCnnError) as err:
            e.risk_read(str(p))
        assert err.value.code == e.ERR_FORMAT and "bad.txt" in str(err.value), name
    with pytest.raises(pkg.EthCnnError) as err:
        e.risk_read(str(tmp_path / "absent.txt"))
    assert err.value.code == e.ERR_IO
    over = rel.copy()
    over[1, 3] = e.RISK_ONE + 1
    with pytest.raises(pkg.EthCnnError) as err:
        e.risk_write(str(tmp_path / "over.txt"), over)
    assert err.value.code == e.ERR_ARG and not os.path.exists(str(tmp_path / "over.txt"))
    with pytest.raises(ValueError):
        e.risk_write(str(tmp_path / "over.txt"), rel[:2])


def test_the_restatement_agrees_with_the_partition_decisions():
    """two routes to the counter inside the restatement: the vectorised descent and the per-node codes of decide_ref"""
    rng = np.random.default_rng(23)
    s = ref.Set()
    s.add_frames((rng.integers(0, 129, size=(2, 12, 21)) / 128.0).astype(np.float32), None, 200, 136)   # partial CTUs right and below
    probs = (rng.integers(0, 129, size=(40, 21)) / 128.0).astype(np.float32)
    probs[5, 3] = np.nan
    s.add(probs)
    rel = rng.integers(0, rref.ONE + 1, size=(3, 1025))
    cands = dref.candidates(rng, 12)
    for table in (None, rel):
        split, stop = rref.evaluate(s, cands, table, chunk=5)
        for i, c in enumerate(cands):
            assert rref.from_codes(s, dref.decide(s, c)["codes"], table) == (split[i], stop[i]), i
    assert any(sum(a) for a in split) and any(sum(b) for b in stop)
    full = rref.evaluate(s, ref.thr(*ref.FULL))
    assert full == ([[0, 0, 0]], [[0, 0, 0]])                           # the full search forces nothing


def test_the_definition_expected_counts_are_where_drawn_truths_land():
    """200,000 CTUs, level 0: the truth flag of every CTU is drawn as Bernoulli(bin / 1024).  Under three candidates the labelled
    counters wrong_split[0] + wrong_stop[0] of sim_ref lie within 5 sigma of risk / 2^20, sigma^2 = the sum of r (1 - r) over the
    forced nodes (checked with this seed: the three deviations are 1.29, 0.43 and 1.06 sigma)."""
    rng = np.random.default_rng(24)
    n = 200000
    bins = rng.integers(0, 1025, size=n)
    probs = np.full((n, 21), 0.5, np.float32)
    probs[:, 0] = (bins / 1024.0).astype(np.float32)                    # k / 1024 is exact in fp32: bin(p) = k
    truth = rng.random(n) < bins / 1024.0
    depth = np.where(truth[:, None], 3, 0).astype(np.uint8) * np.ones((1, 16), np.uint8)   # sum d = 48 > 8: split; 0: unsplit
    s = ref.Set()
    s.add(probs, depth)
    assert np.array_equal(s.bins[:, 0], bins) and np.array_equal(s.truth[:, 0], truth)
    cands = ref.thr([(700, 1024, 1024), (512, 1024, 1024), (900, 1024, 1024)], [(300, -1, -1), (512, -1, -1), (100, -1, -1)])
    counts = s.evaluate(cands, ref.GATES_NONE, chunk=1)
    split, stop = rref.evaluate(s, cands, None, chunk=1)
    for i, c in enumerate(cands):
        up, down = int(c["up_k"][0]), int(c["down_k"][0])
        forced = (bins > up) | (bins <= down)
        r = bins[forced] / 1024.0
        sigma = math.sqrt(float((r * (1.0 - r)).sum()))
        wrong = int(counts[i]["wrong_split"][0]) + int(counts[i]["wrong_stop"][0])
        expected = (split[i][0] + stop[i][0]) / float(rref.ONE)
        print("candidate %d: wrong %d, expected %.1f, sigma %.1f: %.2f sigma" % (i, wrong, expected, sigma, abs(wrong - expected) / sigma))
        assert split[i][1:] == [0, 0] and stop[i][1:] == [0, 0] and forced.sum() > 40000
        assert abs(wrong - expected) <= 5.0 * sigma


# ------------------------------------------------------------------------------------------- refusals before a GPU is touched ---
def _run(cmd, cwd, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run(cmd, cwd=str(cwd), env=e, capture_output=True, text=True, timeout=120)


def _bad_tables(tmp_path):
    good = rref.table_text(rref.identity())
    (tmp_path / "short.txt").write_text(good[:1000])
    (tmp_path / "head.txt").write_text(good.replace("ethcnn-reliability", "reliability", 1))
    (tmp_path / "high.txt").write_text(good.replace(" 2048 ", " 1048577 ", 1))
    return ("short.txt", "head.txt", "high.txt", "absent.txt")


def test_tools_refuse_before_a_gpu_is_touched(tmp_path):
    np.zeros((12, 21), "<f4").tofile(str(tmp_path / "p.dat"))
    np.zeros((9 * 13,), np.uint8).tofile(str(tmp_path / "l.dat"))
    (tmp_path / "thr.txt").write_text(COMPANION["ai"] + "\n")
    nolabels, case = ["--case", "-", "p.dat", "208", "144"], ["--case", "l.dat", "p.dat", "208", "144"]
    tables = _bad_tables(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    tool = lambda name, args: subprocess.run([sys.executable, TOOLS[name]] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    # build_ladder.py: a value that is wrong (status 1) ...
    for args, word in ([(["--no-labels", "--reliability", t] + nolabels, t) for t in tables] +
                       [(["--no-labels", "--max-risk-ppm", "-1"] + nolabels, "--max-risk-ppm"), (["--no-labels", "--max-risk-ppm", str(1 << 64)] + case, "--max-risk-ppm"),
                        (["--no-labels", "--grid", "3"] + nolabels, "--grid"), (nolabels, "--no-labels")]):
        r = tool("build_ladder", args)
        assert r.returncode == 1 and "build_ladder.py: error:" in r.stderr and word in r.stderr and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    # ... and a command line of the wrong form (the usage text, status 2)
    for args in (["--reliability", "short.txt"] + case, ["--max-risk-ppm", "5"] + case, ["--no-labels", "--max-bad-ppm", "5"] + nolabels,
                 ["--no-labels", "--max-risk-ppm", "many"] + nolabels, ["--no-labels", "--reliability"], ["--no-labels"]):
        r = tool("build_ladder", args)
        assert r.returncode == 2 and "build_ladder.py" in r.stderr and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    # simulate_thresholds.py
    for t in tables:
        r = tool("simulate_thresholds", ["--thr-info", "thr.txt", "--order", "ai", "--reliability", t] + nolabels)
        assert r.returncode == 1 and "error:" in r.stderr and t in r.stderr and "Traceback" not in r.stderr, (t, r.returncode, r.stderr[-300:])
    for args in (["--sweep", "up0", "--reliability", "short.txt"] + nolabels, ["--thr-info", "thr.txt", "--order", "ai", "--reliability"],
                 ["--search", "--max-bad-ppm", "5", "--out", "o.txt", "--order", "ai", "--reliability", "short.txt"] + case):
        r = tool("simulate_thresholds", args)
        assert r.returncode == 2 and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    # calibrate_thresholds.py
    for args in (case + ["--reliability-out"], ["--reliability-out", "rel.txt"]):
        r = tool("calibrate_thresholds", args)
        assert r.returncode == 2 and "--reliability-out" in r.stderr and "Traceback" not in r.stderr, (args, r.returncode, r.stderr[-300:])
    assert sorted(os.listdir(str(tmp_path))) == before                 # no output, no temp file


def test_launcher_refuses_a_bad_reliability_table_before_a_gpu_is_touched(tmp_path):
    np.zeros(64 * 64 * 3 // 2, np.uint8).tofile(str(tmp_path / "seq.yuv"))
    (tmp_path / "Thr_info.txt").write_text(COMPANION["ai"] + "\n")
    tables = _bad_tables(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    for t in tables:
        r = _run([sys.executable, LAUNCHER, "seq.yuv", "64", "64", "32"], tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4",
                 ETHCNN_SEARCH_BUDGET_LADDER="auto", ETHCNN_SEARCH_BUDGET_RELIABILITY=t)
        assert r.returncode == 1 and "video_to_cu_depth: ETHCNN_SEARCH_BUDGET_RELIABILITY" in r.stderr and t in r.stderr and "Traceback" not in r.stderr, (t, r.stderr[-300:])
    # auto is the launcher's word, not a file: under a Thr_info.txt that is not the companion line the refusal is that of every budget run
    (tmp_path / "Thr_info.txt").write_text("0.5 0.5 0.5 0.5 0.5 0.5\n")
    r = _run([sys.executable, LAUNCHER, "seq.yuv", "64", "64", "32"], tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="auto")
    assert r.returncode == 1 and "companion" in r.stderr and "cannot be read" not in r.stderr
    (tmp_path / "Thr_info.txt").write_text(COMPANION["ai"] + "\n")
    assert sorted(os.listdir(str(tmp_path))) == before                 # no cu_depth.dat, no temp file


def test_env_parser_knows_auto(pkg, tmp_path, monkeypatch):
    sb = pkg.video_to_cu_depth._sb
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_LADDER", "auto")
    monkeypatch.delenv("ETHCNN_SEARCH_BUDGET_RELIABILITY", raising=False)
    assert sb.ladder_from_env("ai", auto=True) == sb.AUTO and pkg.video_to_cu_depth.search_ladder_from_env() == (sb.AUTO, None)
    with pytest.raises(ValueError) as err:
        sb.ladder_from_env("ldp", auto="this loop sees one frame at a time")
    assert "one frame at a time" in str(err.value) and "ETHCNN_SEARCH_BUDGET_LADDER='auto'" in str(err.value)
    pkg.ethcnn.risk_write(str(tmp_path / "rel.txt"), rref.identity()[:, ::-1].copy())
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_RELIABILITY", str(tmp_path / "rel.txt"))
    word, rel = pkg.video_to_cu_depth.search_ladder_from_env()
    assert word == sb.AUTO and np.array_equal(rel, rref.identity()[:, ::-1])
    monkeypatch.setenv("ETHCNN_SEARCH_BUDGET_LADDER", "")
    assert pkg.video_to_cu_depth.search_ladder_from_env() is None      # without auto the table is not read


@pytest.mark.parametrize("which", ["python", "native"])
def test_daemons_refuse_auto_before_a_gpu_is_touched(pkg, tmp_path, which):
    prog = "resi_to_cu_depth_LDP" if which == "python" else "resi_to_cu_depth_ldp"
    cmd = ([sys.executable, PY_DAEMON, "--python"] if which == "python" else [C_DAEMON, "--quiet"]) + ["--max-frames", "0", "--idle-timeout", "0"]
    (tmp_path / "Thr_info.txt").write_text(COMPANION["ldp"] + "\n")
    r = _run(cmd, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_LADDER="auto")
    assert r.returncode == 1 and (prog + ": ETHCNN_SEARCH_BUDGET_LADDER='auto'") in r.stderr and "Traceback" not in r.stderr, r.stderr[-300:]
    assert "cannot see the sequence in advance" in r.stderr and "build_ladder.py --no-labels" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["Thr_info.txt"]
