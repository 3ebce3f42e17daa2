"""CPU: the trainer group's host-only side (include/ethcnn.h "training, several models at once"): the option check, the exported
names, and the driver's --model-types option."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hevc-complexity-reduction_amd"))

ERR_ARG = -1


def _opts(pkg, k, **kw):
    return [pkg.ethcnn.train_options(**kw) for _ in range(k)]


def _refused(pkg, opts):
    with pytest.raises(pkg.EthCnnError) as ei:
        pkg.ethcnn.train_group_check(opts)
    assert ei.value.code == ERR_ARG
    return str(ei.value)


def test_check_accepts_one_to_eight_members(pkg):
    pkg.ethcnn.train_group_check(_opts(pkg, 1))
    pkg.ethcnn.train_group_check(_opts(pkg, 8))
    pkg.ethcnn.train_group_check(_opts(pkg, 3, net="ldp", batch=7, tune=2))


def test_check_accepts_members_that_differ_in_seed_schedule_momentum_dropout(pkg):
    o = pkg.ethcnn.train_options
    pkg.ethcnn.train_group_check([o(seed=1), o(seed=2, lr=0.02, decay_rate=0.5, decay_steps=2), o(seed=3, momentum=0.8),
                                  o(seed=4, dropout=False)])


@pytest.mark.parametrize("k", [0, 9])
def test_check_refuses_the_member_count(pkg, k):
    assert "k = %d" % k in _refused(pkg, _opts(pkg, k))


@pytest.mark.parametrize("field,kw", [("net", {"net": "ldp"}), ("batch", {"batch": 32}), ("tune", {"tune": 1})])
def test_check_refuses_mixed_members_and_names_them(pkg, field, kw):
    opts = _opts(pkg, 3)
    opts[2] = pkg.ethcnn.train_options(**kw)
    msg = _refused(pkg, opts)
    assert "member 2" in msg and field in msg


@pytest.mark.parametrize("batch", [0, -4])
def test_check_refuses_a_batch_that_is_not_positive(pkg, batch):
    opts = _opts(pkg, 2)
    opts[1] = pkg.ethcnn.train_options(batch=batch)
    msg = _refused(pkg, opts)
    assert "member 1" in msg and "batch" in msg
    msg = _refused(pkg, _opts(pkg, 2, batch=batch))  # every member alike: the first one is named
    assert "member 0" in msg and "batch" in msg


def test_check_without_a_message_buffer(pkg):
    lib = pkg.load_library()
    arr = (pkg.ethcnn.TrainOptions * 2)(*_opts(pkg, 2))
    assert lib.ethcnn_train_group_check(arr, 2, None, 0) == 0
    assert lib.ethcnn_train_group_check(arr, 9, None, 0) == ERR_ARG


def test_every_group_name_of_the_header_is_exported(pkg):
    text = open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(ethcnn_train_group_[a-z0-9_]+)\s*\(", text)))
    want = {"check", "create", "destroy", "init_weights", "set_blob", "get_blob", "set_samples", "set_samples_from", "set_qps", "run",
            "last_stats", "step_indices", "evaluate", "debug_fetch", "last_error"}
    assert {n[len("ethcnn_train_group_"):] for n in names} == want
    lib = ctypes.CDLL(pkg.ethcnn.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "libethcnn.so lacks %s" % n


def test_driver_model_types_option():
    import train_CNN_CTU64 as drv
    a = drv.parse_args(["--train", "t", "--valid", "v", "--model-types", "1,3"])
    assert a.model_types == [1, 3]
    assert drv.group_members(a.model_types) == [drv.MODEL_TYPES[1], drv.MODEL_TYPES[3]] == [("qp22", [22]), ("qp32", [32])]
    a = drv.parse_args(["--model-types", "1,2,3,4"])
    assert [m[0] for m in drv.group_members(a.model_types)] == ["qp22", "qp27", "qp32", "qp37"]
    assert [m[1] for m in drv.group_members(a.model_types)] == [[22], [27], [32], [37]]
    assert drv.parse_args([]).model_types is None and drv.parse_args([]).model_type == 1  # without it: the solo driver
    for bad in (["--model-types", "1,3", "--model-type", "2"], ["--model-types", "1,3", "--qp", "30"], ["--model-types", "5"],
                ["--model-types", "1,1"], ["--model-types", "x"], ["--model-types", ""]):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
