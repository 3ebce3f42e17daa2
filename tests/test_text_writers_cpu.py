"""No GPU: the three text-file writers of the threshold analysis -- ethcnn_risk_write (reliability table), ethcnn_ladder_write (ladder
file) and ethcnn_calib_write_thr_info (Thr_info.txt) -- through the same cases.  All three write through one helper (temporary file
beside the target, rename): a failure names the path and leaves no ".tmp." file, a refused argument leaves an existing target as it
was, and a successful write replaces the target and leaves nothing else in its directory."""
import ctypes
import os

import numpy as np
import pytest

import ladder_ref as lref
import risk_ref as rref

OLD = b"what the file held before\n"


def _writers(pkg):
    """name -> (call(path, good=True) -> return code, the text a good call writes)"""
    e = pkg.ethcnn
    lib = e.load_library()
    rel = np.random.default_rng(41).integers(0, e.RISK_ONE + 1, size=(3, 1025)).astype(np.uint32)
    over = rel.copy()
    over[1, 3] = e.RISK_ONE + 1                                          # a value above ETHCNN_RISK_ONE
    up, down = [(1024, 1000, 512), (700, 0, 1)], [(-1, 0, 512), (300, 0, 1)]
    thr = np.zeros(2, e.SIM_THR)
    thr["up_k"], thr["down_k"] = up, down
    bad_thr = thr.copy()
    bad_thr["up_k"][1, 2] = 1025                                         # a rung with up_k = 1025
    rep = e.CalibReport()
    for l in range(3):
        rep.level[l].up_k, rep.level[l].down_k = up[1][l], down[1][l]
    return {
        "risk": (lambda path, good=True: lib.ethcnn_risk_write(os.fsencode(path), (rel if good else over).ctypes.data), rref.table_text(rel)),
        "ladder": (lambda path, good=True: lib.ethcnn_ladder_write(os.fsencode(path), (thr if good else bad_thr).ctypes.data, 2, e.THR_ORDER_LDP),
                   lref.ladder_lines(up, down, "ldp")),
        # (an order that is neither ETHCNN_THR_ORDER_AI nor ETHCNN_THR_ORDER_LDP)
        "thr_info": (lambda path, good=True: lib.ethcnn_calib_write_thr_info(os.fsencode(path), ctypes.byref(rep), e.THR_ORDER_AI if good else 7),
                     lref.ladder_lines(up[1:], down[1:], "ai")),
    }


WRITERS = ("risk", "ladder", "thr_info")


@pytest.mark.parametrize("name", WRITERS)
def test_a_directory_that_does_not_exist_is_an_io_error_that_names_the_path(pkg, tmp_path, name):
    e = pkg.ethcnn
    call, _ = _writers(pkg)[name]
    path = str(tmp_path / "absent" / "out.txt")
    assert call(path) == e.ERR_IO
    assert path in e.load_library().ethcnn_last_error(None).decode()
    assert os.listdir(str(tmp_path)) == []                               # no directory made, no ".tmp." file anywhere


@pytest.mark.parametrize("name", WRITERS)
def test_a_refused_argument_leaves_the_existing_file_intact(pkg, tmp_path, name):
    e = pkg.ethcnn
    call, _ = _writers(pkg)[name]
    path = tmp_path / "out.txt"
    path.write_bytes(OLD)
    assert call(str(path), good=False) == e.ERR_ARG
    assert path.read_bytes() == OLD and os.listdir(str(tmp_path)) == ["out.txt"]


@pytest.mark.parametrize("name", WRITERS)
def test_a_write_replaces_the_existing_file_and_leaves_only_it(pkg, tmp_path, name):
    call, text = _writers(pkg)[name]
    path = tmp_path / "out.txt"
    path.write_bytes(OLD)
    assert call(str(path)) == 0
    assert path.read_bytes() == text.encode() and os.listdir(str(tmp_path)) == ["out.txt"]
