"""CPU: what the pacer set (include/ethcnn.h "search budget, online: several sequences") settles without a GPU: the entries the header,
the library and the binding carry; the layout of a call -- which blocks of the two kernels and which records a frame owns -- against a
Python restatement; the stand-alone sanitizer program over that entry; and the start-up refusals of `resi_to_cu_depth_LDP.py --sessions
... --budget`, each in a process of its own: status 1, its message, nothing written.  The kernels are in tests/test_gpu_pacer_set.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
ENTRIES = ("create", "destroy", "slots", "launches", "reset", "frames_device", "frames", "last", "plan")
COMPANION_LDP = "0.25 0.75 0.25 0.75 0.25 0.75"
ERR_ARG = -1


def test_header_library_map_and_binding_carry_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "search budget, online: several sequences" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(?:int|void|int64_t) (ethcnn_pacer_set_\w+) ?\(", code))
    assert declared == {"ethcnn_pacer_set_" + n for n in ENTRIES}
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in declared:
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    # the version script exports the C ABI by its prefix, and nothing of the set beside it
    assert "ethcnn_*" in open(os.path.join(ROOT, "hevc-complexity-reduction_amd", "csrc", "ethcnn.map")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", pkg.ethcnn.LIB_PATH]).decode()
    assert {ln.split()[-1] for ln in dyn.splitlines() if "pacer_set" in ln} == declared
    for method in ("frames_device", "frames", "last", "reset", "close"):
        assert callable(getattr(pkg.PacerSet, method))
    assert callable(pkg.ethcnn.pacer_set_plan) and pkg.ethcnn.PACER_SET_MAX == 32
    # ethcnn_pacer_set_frame as the C compiler lays it out
    assert ctypes.sizeof(pkg.ethcnn.PacerSetFrame) == 40 and pkg.ethcnn.PacerSetFrame.result.offset == 32


def _plan_ref(nctus, K):
    """the definition: slices of at most 64 CTUs, balanced; a frame's count blocks = slices x ceil((K + 1) / 256), its bake blocks =
    ceil(n / 256); everything a running sum in call order"""
    rung_blocks = (K + 1 + 255) // 256
    out = {k: [] for k in ("count_first", "count_blocks", "slice_len", "bake_first", "rec0")}
    count = bake = rec = 0
    for n in nctus:
        most = (n + 63) // 64
        length = (n + most - 1) // most
        slices = (n + length - 1) // length
        out["count_first"].append(count), out["count_blocks"].append(slices * rung_blocks), out["slice_len"].append(length)
        out["bake_first"].append(bake), out["rec0"].append(rec)
        count, bake, rec = count + slices * rung_blocks, bake + (n + 255) // 256, rec + n
    out.update(count_grid=count, bake_grid=bake)
    return out


def _calls():
    rng = np.random.default_rng(9)
    mixed = [int(x) for x in rng.choice([1, 12, 63, 64, 65, 128, 129, 272, 510, 1200], size=32)]
    return [[1], [12], [64], [65], [272], [1, 12, 272], [272, 12, 1], mixed, [(1 << 24) - 1] * 32]


@pytest.mark.parametrize("rungs", [2, 256, 257, 514, 4097])
def test_plan_against_its_restatement(pkg, rungs):
    K = rungs - 1
    for nctus in _calls():
        got = pkg.ethcnn.pacer_set_plan(nctus, K)
        assert got == _plan_ref(nctus, K), (nctus[:4], K)
        # the properties themselves: block ranges disjoint, contiguous and in call order; records the running sum; slices cover the frame
        ends = [a + b for a, b in zip(got["count_first"], got["count_blocks"])]
        assert got["count_first"] == [0] + ends[:-1] and ends[-1] == got["count_grid"] < 2 ** 31
        bake_ends = got["bake_first"][1:] + [got["bake_grid"]]
        assert [e - f for f, e in zip(got["bake_first"], bake_ends)] == [(n + 255) // 256 for n in nctus]
        assert got["rec0"] == [sum(nctus[:j]) for j in range(len(nctus))]
        for n, length, blocks in zip(nctus, got["slice_len"], got["count_blocks"]):
            slices = blocks // ((rungs + 255) // 256)
            assert 1 <= length <= 64 and (slices - 1) * length < n <= slices * length and slices == (n + 63) // 64
    assert pkg.ethcnn.pacer_set_plan([272], 512)["slice_len"] == [55]   # 55, 55, 55, 55, 52
    assert pkg.ethcnn.pacer_set_plan([272], 512)["count_blocks"] == [15]
    assert pkg.ethcnn.pacer_set_plan([(1 << 24) - 1] * 32, 4096)["rec0"][31] * 64 > 2 ** 34   # (no 32-bit sum on the way)


def test_plan_refuses_bad_arguments(pkg):
    lib = pkg.load_library()
    for bad, K in (([1] * 33, 512), ([1 << 24], 512), ([12, 0], 512), ([-3], 512), ([], 512), ([12], 0), ([12], 4097)):
        with pytest.raises(pkg.EthCnnError) as err:
            pkg.ethcnn.pacer_set_plan(bad, K)
        assert err.value.code == ERR_ARG, (bad[:2], K)
    grid = np.full(2, 7, np.int64)
    one = np.array([1 << 24], np.int64)
    assert lib.ethcnn_pacer_set_plan(one.ctypes.data, 1, 512, None, None, None, None, None, grid.ctypes.data, grid.ctypes.data + 8) == ERR_ARG
    assert lib.ethcnn_pacer_set_plan(None, 1, 512, None, None, None, None, None, grid.ctypes.data, grid.ctypes.data + 8) == ERR_ARG
    assert grid.tolist() == [7, 7]   # a refusal writes nothing
    # NULL handles never reach a GPU
    assert lib.ethcnn_pacer_set_create(None, 4, None, 0, None, 5, 0, None) == ERR_ARG
    assert lib.ethcnn_pacer_set_reset(None, 0) == ERR_ARG and lib.ethcnn_pacer_set_last(None, 0, None) == ERR_ARG
    assert lib.ethcnn_pacer_set_frames(None, None, 1) == ERR_ARG and lib.ethcnn_pacer_set_frames_device(None, None, 1) == ERR_ARG
    assert lib.ethcnn_pacer_set_slots(None) < 0 and lib.ethcnn_pacer_set_launches(None) < 0
    lib.ethcnn_pacer_set_destroy(None)


def test_host_entry_under_the_sanitizers(tmp_path):
    """the stand-alone program over the host-only entry, built with -fsanitize=address,undefined and run on the CPU"""
    r = subprocess.run(["sh", os.path.join(ROOT, "scripts", "pacer_set_plan_asan.sh"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------------------------------------------------ start-up refusals ---
def _dirs(tmp_path, n, thr=None):
    out = []
    for k in range(n):
        d = tmp_path / ("hm%02d" % k)
        d.mkdir()
        (d / "Thr_info.txt").write_text((thr or {}).get(k, COMPANION_LDP) + "\n")
        out.append(str(d))
    return out


def _tree(tmp_path):
    return sorted((os.path.relpath(os.path.join(dp, f), str(tmp_path)), os.path.getsize(os.path.join(dp, f)))
                  for dp, _, fs in os.walk(str(tmp_path)) for f in fs + ["."])


def _server(tmp_path, args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update(ETHCNN_SYNTHETIC_SEED="21")
    return subprocess.run([sys.executable, LAUNCHER] + args + ["--max-frames", "0", "--idle-timeout", "0"], capture_output=True, text=True, env=e,
                          cwd=str(tmp_path), timeout=120)


def _refused(tmp_path, args, text, status=1):
    before = _tree(tmp_path)
    r = _server(tmp_path, args)
    assert r.returncode == status, (args, r.returncode, r.stderr[-800:])
    assert text in r.stderr and "Traceback" not in r.stderr, (args, r.stderr[-800:])
    assert _tree(tmp_path) == before, args
    return r


def test_the_server_refuses_bad_budget_options_before_a_gpu_is_touched(tmp_path):
    dirs = _dirs(tmp_path, 2)
    five = tmp_path / "five.txt"
    five.write_text("0.1 0.9 0.1 0.9 0.1\n")
    base = ["--sessions"] + dirs
    for opts, text in ((["--budget", "1.5"], "--budget='1.5' is not a share"), (["--budget", "nan"], "share"), (["--budget", "lots"], "share"),
                       (["--budget", "0.4", "--budget-mode", "both"], "--budget-mode='both' (allowed: frame, carry)"),
                       (["--budget", "0.4", "--budget-weights", "64 16 4"], "--budget-weights='64 16 4' is not four integers"),
                       (["--budget", "0.4", "--budget-weights", "64 16 4 x"], "four integers"),
                       (["--budget", "0.4", "--budget-weights", "64 16 4 4294967296"], "four integers"),
                       (["--budget", "0.4", "--budget-ladder", str(tmp_path / "none.txt")], "cannot be read"),
                       (["--budget", "0.4", "--budget-ladder", str(five)], "a rung is six values"),
                       (["--budget", "0.4", "--budget-ladder", "auto"], "one frame at a time")):
        r = _refused(tmp_path, base + opts, text)
        assert "resi_to_cu_depth_LDP: " in r.stderr


def test_a_directory_without_the_companion_line_is_refused(tmp_path):
    # the gates (tokens [1] and [3]) are the companion's, so the directory gets as far as the companion check
    for k, text in ((1, "0.3 0.75 0.25 0.75 0.25 0.75"), (0, "0.25 0.75 0.25 0.75 0.25 0.7"), (2, COMPANION_LDP + " 0.25")):
        sub = tmp_path / ("case%d" % k)
        sub.mkdir()
        dirs = _dirs(sub, 3, thr={k: text})
        r = _refused(sub, ["--sessions"] + dirs + ["--budget", "0.4"], "companion")
        assert COMPANION_LDP in r.stderr and os.path.join(dirs[k], "Thr_info.txt") in r.stderr and "--budget is set" in r.stderr


def test_the_budget_options_belong_to_sessions(tmp_path):
    (tmp_path / "Thr_info.txt").write_text(COMPANION_LDP + "\n")
    _refused(tmp_path, ["--python", "--budget", "0.4"], "usage:", status=2)
    _refused(tmp_path, ["--budget", "0.4", "--budget-mode", "carry"], "usage:", status=2)
    dirs = _dirs(tmp_path, 1)
    _refused(tmp_path, ["--sessions"] + dirs + ["--budget-mode", "carry"], "usage:", status=2)   # a mode without a budget
    _refused(tmp_path, ["--sessions"] + dirs + ["--budget", "0.4", "--budget", "0.5"], "usage:", status=2)


def test_the_environment_stays_refused_beside_the_options(tmp_path):
    dirs = _dirs(tmp_path, 2)
    before = _tree(tmp_path)
    e = dict({k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}, ETHCNN_SEARCH_BUDGET="0.4")
    r = subprocess.run([sys.executable, LAUNCHER, "--sessions"] + dirs + ["--budget", "0.4", "--max-frames", "0", "--idle-timeout", "0"], capture_output=True,
                       text=True, env=e, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1 and "ETHCNN_SEARCH_BUDGET is set" in r.stderr and "Traceback" not in r.stderr and _tree(tmp_path) == before


def test_a_good_budget_command_line_gets_past_the_checks(pkg, tmp_path):
    """whatever happens next is none of the refusals (on a machine without a GPU the context fails, with another message)"""
    dirs = _dirs(tmp_path, 3)
    pkg.ethcnn.sim_write_thr_info(os.path.join(dirs[1], "Thr_info.txt"), pkg.ethcnn.budget_companion_thr(), "ldp")   # as the library writes it
    ladder = tmp_path / "ladder.txt"
    ladder.write_text("0.0 1.0 0.0 1.0 0.0 1.0\n0.25 0.75 0.25 0.75 0.25 0.75\n\n0.5 0.5 0.5 0.5 0.5 0.5\n")
    r = _server(tmp_path, ["--sessions"] + dirs + ["--quiet", "--budget", "0.4", "--budget-mode", "carry", "--budget-weights", "8 4 2 1", "--budget-ladder",
                                                    str(ladder)])
    assert "companion" not in r.stderr and "budget" not in r.stderr and "usage" not in r.stderr, r.stderr[-600:]
    assert r.returncode != 2
    assert not [f for d in dirs for f in os.listdir(d) if f != "Thr_info.txt"]
