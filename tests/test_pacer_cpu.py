"""CPU: the host-only part of the online search budget (include/ethcnn.h "search budget, online") -- the entries the header declares, the
layout of ethcnn_pacer_result, the argument rules of ethcnn_pacer_check -- and the refusals of both Low-Delay-P daemons under
ETHCNN_SEARCH_BUDGET, which come before a GPU is touched.  The kernel and the end-to-end runs are in tests/test_gpu_pacer.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import budget_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_DAEMON = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
C_DAEMON = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "resi_to_cu_depth_ldp")
ENTRIES = ("check", "create", "destroy", "reset", "frame_device", "frame", "last")
COMPANION_LDP = "0.25 0.75 0.25 0.75 0.25 0.75"


def test_header_library_and_binding_carry_exactly_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    assert "search budget, online" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(?:int|void) (ethcnn_pacer_\w+)\(", code))
    assert declared == {"ethcnn_pacer_" + n for n in ENTRIES}
    assert set(re.findall(r"\b(ethcnn_pacer_\w+)\(", code)) == declared
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for name in declared:
        assert getattr(lib, name) and name in pkg.ethcnn.SIGNATURES
    for method in ("frame", "frame_device", "last", "reset", "close"):
        assert callable(getattr(pkg.Pacer, method))
    assert callable(pkg.ethcnn.pacer_check)


def test_result_layout_matches_the_documented_one(pkg, tmp_path):
    want = {"frame": (0, 8), "rung": (8, 4), "over": (12, 4), "cost": (16, 8), "full": (24, 8), "carry_lo": (32, 8), "carry_hi": (40, 8),
            "up_k": (48, 12), "down_k": (60, 12)}
    dt = pkg.ethcnn.PACER_RESULT
    assert dt.itemsize == 72 and {n: (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names} == want
    # ... and the C compiler agrees with the header's text
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ethcnn.h"\nint main(void) {\n  printf("%zu", sizeof(ethcnn_pacer_result));\n' +
                   "".join('  printf(" %%zu", offsetof(ethcnn_pacer_result, %s));\n' % n for n in dt.names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [72] + [want[n][0] for n in dt.names]


def test_check_agrees_with_the_argument_rules(pkg):
    e = pkg.ethcnn
    lib = pkg.load_library()
    lad = np.ascontiguousarray(bref.default_ladder()[:5])
    w = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
    p = lad.ctypes.data
    assert lib.ethcnn_pacer_check(p, 5, w, 400000, e.BUDGET_FRAME) == 0
    assert lib.ethcnn_pacer_check(p, 1, w, 0, e.BUDGET_CARRY) == 0 and lib.ethcnn_pacer_check(p, 5, w, 10 ** 6, e.BUDGET_CARRY) == 0
    assert lib.ethcnn_pacer_check(p, 5, None, 400000, e.BUDGET_FRAME) == 0        # NULL weight: the default
    assert lib.ethcnn_pacer_check(None, 0, None, 400000, e.BUDGET_FRAME) == 0     # NULL ladder: the default, K is not read
    big = np.ascontiguousarray(np.resize(bref.default_ladder(), 4097))
    assert lib.ethcnn_pacer_check(big.ctypes.data, 4096, w, 5, 0) == 0
    for k, ptr in ((0, p), (4097, big.ctypes.data), (-1, p)):
        assert lib.ethcnn_pacer_check(ptr, k, w, 400000, 0) == e.ERR_ARG, k
    for field, level, value in (("up_k", 2, 1025), ("up_k", 0, -1), ("down_k", 1, -2), ("down_k", 2, 1025)):
        bad = lad.copy()
        bad[field][3, level] = value
        assert lib.ethcnn_pacer_check(bad.ctypes.data, 5, w, 400000, 0) == e.ERR_ARG, (field, level, value)
        assert "candidate 3" in lib.ethcnn_last_error(None).decode()
    for d in range(4):
        wbig = (ctypes.c_uint64 * 4)(64, 16, 4, 1)
        wbig[d] = 2 ** 32
        assert lib.ethcnn_pacer_check(p, 5, wbig, 400000, 0) == e.ERR_ARG
        wbig[d] = 2 ** 32 - 1
        assert lib.ethcnn_pacer_check(p, 5, wbig, 400000, 0) == 0
    assert lib.ethcnn_pacer_check(p, 5, w, 10 ** 6 + 1, 0) == e.ERR_ARG
    for mode in (2, -1, 7):
        assert lib.ethcnn_pacer_check(p, 5, w, 400000, mode) == e.ERR_ARG
    # the binding's form
    e.pacer_check(400000)
    e.pacer_check(0, e.BUDGET_CARRY, lad, (1, 2, 3, 4))
    for args in ((10 ** 6 + 1,), (5, 2), (5, 0, lad, (1, 2, 3, 2 ** 32))):
        with pytest.raises(pkg.EthCnnError) as err:
            e.pacer_check(*args)
        assert err.value.code == e.ERR_ARG
    # NULL handles never reach a GPU
    assert lib.ethcnn_pacer_create(None, None, 0, None, 5, 0, None) == e.ERR_ARG
    assert lib.ethcnn_pacer_reset(None) == e.ERR_ARG and lib.ethcnn_pacer_last(None, None) == e.ERR_ARG
    assert lib.ethcnn_pacer_frame(None, None, 64, 64, None, None) == e.ERR_ARG
    assert lib.ethcnn_pacer_frame_device(None, None, 64, 64, None, None) == e.ERR_ARG
    lib.ethcnn_pacer_destroy(None)


def _daemon(which, cwd, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update({k: str(v) for k, v in env.items()})
    cmd = [sys.executable, PY_DAEMON, "--python"] if which == "python" else [C_DAEMON, "--quiet"]
    return subprocess.run(cmd + ["--max-frames", "0", "--idle-timeout", "0"], cwd=str(cwd), env=e, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("which", ["python", "native"])
def test_daemons_refuse_before_a_gpu_is_touched(pkg, tmp_path, which):
    """every refusal comes before the context is made: exit status 1, the message, no signal file and no cu_depth.dat (on a machine
    without a GPU the accepted case at the end fails at the context instead, with another message)"""
    name = "resi_to_cu_depth_LDP" if which == "python" else "resi_to_cu_depth_ldp"
    thr = tmp_path / "Thr_info.txt"
    thr.write_text(COMPANION_LDP + "\n")
    for env, word in (({"ETHCNN_SEARCH_BUDGET": "1.5"}, "ETHCNN_SEARCH_BUDGET='1.5'"), ({"ETHCNN_SEARCH_BUDGET": "-1"}, "share"),
                      ({"ETHCNN_SEARCH_BUDGET": "lots"}, "share"), ({"ETHCNN_SEARCH_BUDGET": "nan"}, "share"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_MODE": "both"}, "frame, carry"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4"}, "four integers"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4 x"}, "four integers"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4 4294967296"}, "four integers"),
                      ({"ETHCNN_SEARCH_BUDGET": "0.4", "ETHCNN_SEARCH_BUDGET_WEIGHTS": "64 16 4 1 1"}, "four integers")):
        r = _daemon(which, tmp_path, ETHCNN_SYNTHETIC_SEED=1, **env)
        assert r.returncode == 1 and (name + ": ") in r.stderr and word in r.stderr and "Traceback" not in r.stderr, (env, r.returncode, r.stderr[-300:])
    for text in ("0.5 0.5 0.5 0.5 0.5 0.5\n", "0.75 0.25 0.75 0.25 0.75 0.25\n", "0.25 0.75 0.25 0.75 0.25\n", COMPANION_LDP + " 0.25\n", "0.25 0.75 0.25 0.75 0.25 up\n",
                 None):
        if text is None:
            os.remove(str(thr))
        else:
            thr.write_text(text)
        r = _daemon(which, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4")
        assert r.returncode == 1 and COMPANION_LDP in r.stderr and "Thr_info.txt" in r.stderr and "Traceback" not in r.stderr, (text, r.stderr[-300:])
    assert sorted(os.listdir(str(tmp_path))) == []   # no pred_end.sig, no cu_depth.dat, no state file
    # the companion line as the library writes it is accepted: whatever happens next is not that refusal
    pkg.ethcnn.sim_write_thr_info(str(thr), pkg.ethcnn.budget_companion_thr(), "ldp")
    r = _daemon(which, tmp_path, ETHCNN_SYNTHETIC_SEED=1, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_MODE="carry", ETHCNN_SEARCH_BUDGET_WEIGHTS="8 4 2 1")
    assert "companion" not in r.stderr and "ETHCNN_SEARCH_BUDGET" not in r.stderr, r.stderr[-300:]
    assert "pred_end.sig" not in os.listdir(str(tmp_path)) and "cu_depth.dat" not in os.listdir(str(tmp_path))
