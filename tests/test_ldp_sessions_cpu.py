"""CPU: what the Low-Delay-P sessions (include/ethcnn.h "config #5 online, several live encoders") settle without a GPU: the layout of
a step -- which 16-CTU groups a picture owns, where the passes are cut -- against its numpy restatement, the byte formula, and the
four start-up refusals of `resi_to_cu_depth_LDP.py --sessions`, each in a process of its own: status 1, its message, nothing written."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
ERR_ARG = -1
COUNTS = [1, 4, 12, 16, 17, 28, 1200]
DEFAULT_CAP = 131072  # ethcnn_options.max_ctus_per_pass = 0


def _orders():
    rng = np.random.default_rng(5)
    out = [list(COUNTS), list(reversed(COUNTS)), [1200, 1, 1200, 17, 16, 4, 12, 28, 1200]]
    out += [[int(x) for x in rng.permutation(COUNTS)] for _ in range(4)]
    out += [[c] for c in COUNTS] + [list(p) for p in itertools.permutations((16, 17, 1), 3)]
    return out


def _plan_ref(nctus, cap):
    """numpy: first_group = running sum of ceil(n / 16); passes of floor(cap / 16) groups, the last one shorter"""
    g = (np.asarray(nctus, dtype=np.int64) + 15) // 16
    first = np.concatenate([[0], np.cumsum(g)[:-1]])
    total, per = int(g.sum()), (cap or DEFAULT_CAP) // 16
    passes = [min(per, total - p) for p in range(0, total, per)]
    return [int(x) for x in first], passes


@pytest.mark.parametrize("cap", [32, 0])
def test_plan_against_its_restatement(pkg, cap):
    for nctus in _orders():
        got = pkg.ethcnn.ldp_sessions_plan(nctus, cap)
        first, passes = _plan_ref(nctus, cap)
        assert got["first_group"] == first and got["pass_groups"] == passes, (nctus, cap, got)
        # the properties themselves, not only the restatement: group boundaries, the cap, nothing lost
        groups = [(n + 15) // 16 for n in nctus]
        assert got["first_group"] == [sum(groups[:j]) for j in range(len(nctus))]
        assert sum(got["pass_groups"]) == sum(groups)
        assert all(0 < p and p * 16 <= (cap or DEFAULT_CAP) for p in got["pass_groups"])
    if cap == 32:  # 1200 CTUs alone: 75 groups in passes of 2, the last one of 1
        assert pkg.ethcnn.ldp_sessions_plan([1200], 32)["pass_groups"] == [2] * 37 + [1]
    else:
        assert pkg.ethcnn.ldp_sessions_plan(COUNTS, 0)["pass_groups"] == [1 + 1 + 1 + 1 + 2 + 2 + 75]


def test_plan_refuses_bad_arguments(pkg):
    lib = pkg.load_library()
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    np_, first, passes = ctypes.c_int(0), (ctypes.c_int * 40)(), (ctypes.c_int * 40)()
    call = lambda nctus, n, cap, pg=passes, mp=40: lib.ethcnn_ldp_sessions_plan(arr(nctus), n, cap, first, ctypes.byref(np_), pg, mp)
    assert call([4, 12], 2, 32) == 0 and np_.value == 1 and passes[0] == 2
    assert call([4, 0], 2, 32) == ERR_ARG        # a picture without CTUs
    assert call([4, 12], 0, 32) == ERR_ARG       # no pictures
    assert call([1] * 33, 33, 32) == ERR_ARG     # more than 32
    assert call([4, 12], 2, 15) == ERR_ARG       # a pass that cannot hold one group
    assert call([4, 12], 2, -1) == ERR_ARG
    assert call([4, 12], 2, 32, None, 1) == ERR_ARG and call([4, 12], 2, 32, None, 0) == 0
    assert lib.ethcnn_ldp_sessions_plan(None, 2, 32, first, ctypes.byref(np_), passes, 40) == ERR_ARG
    # at most max_passes rows are written
    passes[1] = -7
    assert call([1200], 1, 32, passes, 1) == 0 and np_.value == 38 and passes[0] == 2 and passes[1] == -7


def test_bytes_against_the_formula(pkg):
    sizes = [(72, 72), (200, 136), (1040, 64), (416, 240), (1, 1), (2560, 1920)]
    want = 0
    for w, h in sizes:
        n = ((w + 63) // 64) * ((h + 63) // 64)
        want += (n + 15) // 16 * 16 * (448 * 4 + 2 * 448 * 4)  # vectors and the (c, h) state of whole 16-CTU groups
    ws, hs = [s[0] for s in sizes], [s[1] for s in sizes]
    assert pkg.ethcnn.ldp_sessions_bytes(ws, hs) == want
    assert pkg.ethcnn.ldp_sessions_bytes([64], [64]) == 16 * 5376
    assert pkg.ethcnn.ldp_sessions_bytes([64, 0], [64, 64]) == ERR_ARG
    assert pkg.ethcnn.ldp_sessions_bytes([64] * 33, [64] * 33) == ERR_ARG
    assert pkg.load_library().ethcnn_ldp_sessions_bytes(None, None, 1) == ERR_ARG


def test_the_front_end_switch_is_in_the_experiments_build_only(pkg):
    lib = os.path.join(ROOT, "hevc-complexity-reduction_amd", "%s", "libethcnn.so")
    assert b"ETHCNN_SESSIONS_FRONT\0" not in open(lib % "lib", "rb").read()
    assert b"ETHCNN_SESSIONS_FRONT\0" in open(lib % "lib_exp", "rb").read()


def test_host_entries_under_the_sanitizers(tmp_path):
    """the stand-alone program over the two host-only entries, built with -fsanitize=address,undefined and run on the CPU"""
    r = subprocess.run(["sh", os.path.join(ROOT, "scripts", "ldp_sessions_plan_asan.sh"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------------------------------------------------ start-up refusals ---
def _dirs(tmp_path, n, thr=None):
    out = []
    for k in range(n):
        d = tmp_path / ("hm%02d" % k)
        d.mkdir()
        (d / "Thr_info.txt").write_text((thr or {}).get(k, "0.4 0.6 0.3 0.7 0.2 0.8"))
        out.append(str(d))
    return out


def _tree(tmp_path):
    return sorted((os.path.relpath(os.path.join(dp, f), str(tmp_path)), os.path.getsize(os.path.join(dp, f)))
                  for dp, _, fs in os.walk(str(tmp_path)) for f in fs + ["."])


def _refused(tmp_path, dirs, text, env=None):
    before = _tree(tmp_path)
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    e.update(env or {}, ETHCNN_SYNTHETIC_SEED="21")
    r = subprocess.run([sys.executable, LAUNCHER, "--sessions"] + dirs + ["--max-frames", "1", "--idle-timeout", "1"], capture_output=True, text=True,
                       env=e, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr[-800:])
    assert text in r.stderr and "Traceback" not in r.stderr, r.stderr[-800:]
    assert _tree(tmp_path) == before, "a refused start-up wrote something"


def test_a_directory_listed_twice_is_refused(tmp_path):
    dirs = _dirs(tmp_path, 2)
    _refused(tmp_path, [dirs[0], dirs[1], os.path.join(dirs[0], "..", "hm00")], "listed twice")


def test_more_than_32_directories_are_refused(tmp_path):
    _refused(tmp_path, _dirs(tmp_path, 33), "33 directories")


def test_other_gate_thresholds_are_refused(tmp_path):
    # token [3] differs in directory 2; tokens [0], [2], [4], [5] may differ (the encoder reads those itself)
    dirs = _dirs(tmp_path, 3, thr={1: "0.1 0.6 0.9 0.7 0.3 0.9", 2: "0.4 0.6 0.3 0.75 0.2 0.8"})
    _refused(tmp_path, dirs, "gate thresholds of %s" % os.path.join(dirs[2], "Thr_info.txt"))
    _refused(tmp_path, [dirs[2], dirs[0]], "differ")  # whichever comes first sets the pair


@pytest.mark.parametrize("var,val", [("ETHCNN_SEARCH_BUDGET", "0.5"), ("ETHCNN_SEARCH_BUDGET_MODE", "carry"), ("ETHCNN_SEARCH_BUDGET_LADDER", "x.txt")])
def test_a_search_budget_is_refused(tmp_path, var, val):
    _refused(tmp_path, _dirs(tmp_path, 2), var, env={var: val})
