"""No GPU: the gate thresholds as a property of a sequence (include/ethcnn.h: ethcnn_ldp_sessions_set_ / _clear_ / _get_thresholds and
ethcnn_ldp_set_ / clear_ / get_thresholds_batch and _group) -- the nine entries in the header, the export map, the library and the binding; the start-up checks of
`resi_to_cu_depth_LDP.py --sessions --gates-per-dir` and of `resi_video_to_cu_depth_LDP.py --thr-info-qp`, none of which opens a GPU."""
import fnmatch
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hevc-complexity-reduction_amd")
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
OFFLINE = os.path.join(PKG, "resi_video_to_cu_depth_LDP.py")
# (batch and group carry the form last: the families ethcnn_ldp_batch_* and ethcnn_ldp_group_* are held to closed lists by
# tests/test_ldp_batch_cpu.py and tests/test_ldp_group_cpu.py)
ENTRIES = ["ethcnn_ldp_sessions_%s_thresholds" % verb for verb in ("set", "clear", "get")] + \
          ["ethcnn_ldp_%s_thresholds_%s" % (verb, form) for form in ("batch", "group") for verb in ("set", "clear", "get")]
# three files whose tokens [1] and [3] all differ
THR = {0: "0.4 0.6 0.3 0.7 0.2 0.8", 1: "0.1 0.25 0.9 0.75 0.3 0.9", 2: "0.4 0.5 0.3 0.125 0.2 0.8"}
PAIRS = [(0.6, 0.7), (0.25, 0.75), (0.5, 0.125)]


def test_the_nine_entries_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    globs = re.search(r"global:([^}]*?)local:", open(os.path.join(PKG, "csrc", "ethcnn.map")).read()).group(1).replace(";", " ").split()
    assert len(ENTRIES) == 9
    for d in ("lib", "lib_exp"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, d, "libethcnn.so")]).decode()
        names = set(l.split()[-1] for l in out.splitlines() if l.strip())
        assert [n for n in ENTRIES if n not in names] == [], d
    for n in ENTRIES:
        assert re.search(r"^int %s\(" % n, header, re.M), "%s is not declared in include/ethcnn.h" % n
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), "%s is not exported by csrc/ethcnn.map" % n
        assert n in pkg.ethcnn.SIGNATURES, "%s is not in the binding's table" % n
    for cls in (pkg.LdpSessions, pkg.LdpBatch, pkg.LdpGroup):
        for m in ("set_thresholds", "clear_thresholds", "thresholds_of"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    # the three normative blocks speak of the resolved pair, and the feed entries of their refusal
    assert header.count("RESOLVED pair") == 3
    assert "ethcnn_ldp_clear_thresholds_batch" in open(os.path.join(PKG, "csrc", "ethcnn_replay.cpp")).read()


def _dirs(tmp_path, thr):
    out = []
    for k in sorted(thr):
        d = tmp_path / ("hm%02d" % k)
        d.mkdir()
        if thr[k] is not None:
            (d / "Thr_info.txt").write_text(thr[k])
        out.append(str(d))
    return out


def _tree(tmp_path):
    return sorted((os.path.relpath(os.path.join(dp, f), str(tmp_path)), os.path.getsize(os.path.join(dp, f)))
                  for dp, _, fs in os.walk(str(tmp_path)) for f in fs + ["."])


def _server(tmp_path, dirs, more=()):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    e.update(ETHCNN_SYNTHETIC_SEED="21")
    return subprocess.run([sys.executable, LAUNCHER, "--sessions"] + dirs + list(more) + ["--max-frames", "1", "--idle-timeout", "1"], capture_output=True,
                          text=True, env=e, cwd=str(tmp_path), timeout=120)


def _refused(tmp_path, run, text):
    before = _tree(tmp_path)
    r = run()
    assert r.returncode == 1, (r.returncode, r.stderr[-800:])
    assert text in r.stderr and "Traceback" not in r.stderr, r.stderr[-800:]
    assert _tree(tmp_path) == before, "a refused start-up wrote something"


def test_differing_gate_files_pass_the_start_up_checks_with_the_option(pkg, tmp_path):
    """as far as the start-up checks go (check_sessions, what main calls before it creates a context): the three pairs come back in
    the order of the directories; without the option the same directories are refused in the words they were always refused in"""
    daemon = importlib.import_module("hevc-complexity-reduction_amd.resi_to_cu_depth_LDP")
    dirs = _dirs(tmp_path, THR)
    before = _tree(tmp_path)
    got = daemon.check_sessions(dirs, gates_per_dir=True)
    assert [tuple(np.float32(x) for x in g) for g in got] == [tuple(np.float32(x) for x in p) for p in PAIRS]
    assert daemon.check_sessions(dirs[:1]) == daemon.check_sessions(dirs[:1], gates_per_dir=True)[0]
    with pytest.raises(ValueError) as e:
        daemon.check_sessions(dirs)
    assert "one server has one pair of gates" in str(e.value) and os.path.join(dirs[1], "Thr_info.txt") in str(e.value)
    assert _tree(tmp_path) == before
    _refused(tmp_path, lambda: _server(tmp_path, dirs), "one server has one pair of gates")
    # the option does not lift the other refusals
    with pytest.raises(ValueError) as e:
        daemon.check_sessions(dirs + [os.path.join(dirs[0], "..", "hm00")], gates_per_dir=True)
    assert "listed twice" in str(e.value)


@pytest.mark.parametrize("bad", [None, "0.4 0.6", ""])
def test_an_unreadable_or_malformed_gate_file_is_refused_with_its_path(tmp_path, bad):
    dirs = _dirs(tmp_path, {0: THR[0], 1: THR[1], 2: bad})
    _refused(tmp_path, lambda: _server(tmp_path, dirs, ["--gates-per-dir"]), os.path.join(dirs[2], "Thr_info.txt"))


def test_the_option_belongs_to_sessions(tmp_path):
    r = subprocess.run([sys.executable, LAUNCHER, "--python", "--gates-per-dir", "--max-frames", "1", "--idle-timeout", "1"], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr and "--gates-per-dir" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_beside_a_budget_every_file_must_be_the_companion_line(pkg, tmp_path):
    """with --budget the option has no effect: the gates are opened on the context, so the files must still be the companion line"""
    dirs = _dirs(tmp_path, THR)
    _refused(tmp_path, lambda: _server(tmp_path, dirs, ["--gates-per-dir", "--budget", "0.5"]), "Thr_info.txt")


# ----------------------------------------------------------------------------------------------------------- the offline command ---
def _offline(tmp_path, args):
    e = dict(os.environ, ETHCNN_SYNTHETIC_SEED="21")
    return subprocess.run([sys.executable, OFFLINE] + args, capture_output=True, text=True, env=e, cwd=str(tmp_path), timeout=120)


def _inputs(tmp_path):
    w, h = 64, 64
    (tmp_path / "a.yuv").write_bytes(bytes(w * h * 3 // 2 * 2))
    (tmp_path / "list.txt").write_text("a.yuv 64 64 32 a.dat\na.yuv 64 64 22 b.dat\n")
    (tmp_path / "t32.txt").write_text(THR[1])
    (tmp_path / "two.txt").write_text("0.4 0.6")


@pytest.mark.parametrize("form", ["list", "positional"])
@pytest.mark.parametrize("opts,text", [(["--thr-info-qp", "32", "t32.txt", "--thr-info-qp", "32", "t32.txt"], "QP 32 is given twice"),
                                       (["--thr-info-qp", "32", "nowhere.txt"], "nowhere.txt"),
                                       (["--thr-info-qp", "32", "two.txt"], "two.txt"),
                                       (["--thr-info-qp", "x", "t32.txt"], "QP is not a number")])
def test_thr_info_qp_is_refused_before_a_context_exists(tmp_path, form, opts, text):
    """status 1 and nothing written.  No context was created: the refusal comes with device 99, which no machine has -- a command that
    got as far as creating its context would fail in other words (and on a machine without a GPU, at once)"""
    _inputs(tmp_path)
    args = (["--list", "list.txt"] if form == "list" else ["a.yuv", "64", "64", "32", "--out", "a.dat"]) + ["--device", "99"] + opts
    _refused(tmp_path, lambda: _offline(tmp_path, args), text)


def test_thr_info_qp_parses_into_pairs_by_qp(pkg, tmp_path):
    offline = importlib.import_module("hevc-complexity-reduction_amd.resi_video_to_cu_depth_LDP")
    _inputs(tmp_path)
    (tmp_path / "t22.txt").write_text(THR[2])
    got = offline.gates_by_qp([["32", str(tmp_path / "t32.txt")], ["22", str(tmp_path / "t22.txt")]])
    assert {q: tuple(np.float32(x) for x in g) for q, g in got.items()} == {32: tuple(np.float32(x) for x in PAIRS[1]), 22: tuple(np.float32(x) for x in PAIRS[2])}
    assert offline.gates_by_qp(None) == {}
