"""CPU: the host-only parts of the ETH-LSTM trainer group (include/ethcnn.h "ETH-LSTM training, several models at once"): the option
check, the driver's --qps parsing and the per-member keep lists."""
import importlib
import os
import sys

import numpy as np
import pytest

import train_data_lstm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drv(pkg):
    sys.path.insert(0, os.path.join(ROOT, "hevc-complexity-reduction_amd"))
    return importlib.import_module("train_LSTM_CTU64")


def _refused(pkg, opts):
    with pytest.raises(pkg.EthCnnError) as ei:
        pkg.ethcnn.lstm_train_group_check(opts)
    assert ei.value.code == -1  # ETHCNN_ERR_ARG
    return str(ei.value)


def test_check_accepts_members_that_differ_in_everything_but_the_batch(pkg):
    O = pkg.ethcnn.lstm_train_options
    pkg.ethcnn.lstm_train_group_check([O(batch=7)])
    pkg.ethcnn.lstm_train_group_check([O(batch=7, seed=1), O(batch=7, seed=2, lr=0.05, momentum=0.8, decay_rate=0.5, decay_steps=3,
                                                             dropout=False, qp_scale=0.18, clip_norm=0.0)] * 4)


def test_check_names_the_member_and_the_field(pkg):
    O = pkg.ethcnn.lstm_train_options
    assert "k = 0" in _refused(pkg, [])
    assert "k = 9" in _refused(pkg, [O(batch=7)] * 9)
    msg = _refused(pkg, [O(batch=7), O(batch=7), O(batch=8)])
    assert "member 2" in msg and "batch" in msg
    for field, kw in (("batch", dict(batch=0)), ("batch", dict(batch=4097)), ("decay_steps", dict(decay_steps=0)),
                      ("lr_init", dict(lr=float("nan"))), ("momentum", dict(momentum=float("inf"))),
                      ("decay_rate", dict(decay_rate=float("nan"))), ("qp_scale", dict(qp_scale=-1.0)),
                      ("qp_scale", dict(qp_scale=float("nan"))), ("clip_norm", dict(clip_norm=-0.5)),
                      ("clip_norm", dict(clip_norm=float("inf")))):
        bad = dict(batch=7)
        bad.update(kw)
        first = "batch" in kw  # a bad batch is met at member 0: the members of a group share it
        msg = _refused(pkg, [O(**bad), O(**bad)] if first else [O(batch=7), O(**bad)])
        assert ("member %d" % (0 if first else 1)) in msg and field in msg, (kw, msg)
    with pytest.raises(TypeError):
        pkg.ethcnn.lstm_train_group_check([pkg.ethcnn.train_options(batch=7)])


def test_qps_parsing(drv):
    base = ["--train", "a", "--valid", "b"]
    assert drv.parse_args(base + ["--qps", "22,27,32,37"]).qps == [22, 27, 32, 37]
    assert drv.parse_args(base + ["--qps", "5"]).qps == [5]
    assert drv.parse_args(base + ["--qp", "32"]).qps is None and drv.parse_args(base).qps is None
    for bad in (["--qps", "22,22"], ["--qps", ""], ["--qps", "1,2,3,4,5,6,7,8,9"], ["--qps", "22,x"], ["--qps", "52"],
                ["--qps", "22,27", "--qp", "32"], ["--qps", "22,27", "--model-type", "2"]):
        with pytest.raises(SystemExit):
            drv.parse_args(base + bad)


def test_keep_lists_equal_lstm_select_qp(pkg):
    E = pkg.ethcnn
    data = train_data_lstm.make_samples(60, seed=3)
    sizes = []
    for qps in ([22], [27, 32], [], [37, 22, 27, 32], [5]):
        got, want = E.lstm_group_keep_list(data, qps), E.lstm_select_qp(data, qps)
        assert got.dtype == np.int64 and np.array_equal(got, want), qps
        sizes.append(len(got))
    assert 0 < sizes[0] < sizes[1] < sizes[2] == sizes[3] == 60 and sizes[4] == 0
    with pytest.raises(pkg.EthCnnError) as ei:
        E.lstm_group_keep_list(data[:-1], [22])
    assert ei.value.code == -3  # ETHCNN_ERR_FORMAT
