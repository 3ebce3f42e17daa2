"""GPU: the trainer group (include/ethcnn.h "training, several models at once") against solo Trainers created in the same test with
the same options, weights and samples.  Every comparison is bit for bit.  Data: seeded synthetic records (tests/train_data.py,
tests/train_data_ldp.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_data
import train_data_ldp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREC, NVALID = 300, 400
DATA = train_data.make_records(NREC, seed=21)
VALID = train_data.make_records(NVALID, seed=22)
LDP_DATA = train_data_ldp.make_records(200, seed=23)
LDP_VALID = train_data_ldp.make_records(320, seed=24)
HEAD32 = ("h_fc1__32__w", "h_fc1__32__b", "h_fc2__32__w", "h_fc2__32__b", "y_conv_flat__32__w", "y_conv_flat__32__b")


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _group(pkg, ctx, members, qps, init, data=DATA, valid=None):
    """members: Trainer keyword dicts; qps: per member QP lists (None: keep the default); init: per member weight seeds"""
    g = pkg.TrainerGroup(ctx, [pkg.ethcnn.train_options(**kw) for kw in members])
    g.set_samples(0, data)
    if valid is not None:
        g.set_samples(1, valid)
    for m, q in enumerate(qps):
        if q is not None:
            g.set_qps(m, q)
    g.init_weights(init)
    return g


def _solo(pkg, ctx, kw, qps, init, data=DATA, valid=None):
    t = pkg.Trainer(ctx, **kw)
    t.set_samples(0, data)
    if valid is not None:
        t.set_samples(1, valid)
    if qps is not None:
        t.set_qps(qps)
    t.init_weights(init)
    return t


def _state(pkg, fetch, blob_accum, stats):
    e = pkg.ethcnn
    blob, accum = blob_accum
    out = {"blob": blob, "accum": accum, "loss": stats[0], "acc": stats[1]}
    for name, which in (("indices", e.TDBG_INDICES), ("mask_fc1", e.TDBG_MASK_FC1), ("mask_fc2", e.TDBG_MASK_FC2),
                        ("probs", e.TDBG_PROBS), ("grads", e.TDBG_GRADS), ("dbg_accum", e.TDBG_ACCUM)):
        out[name] = fetch(which)
    return out


def _member_state(pkg, g, m):
    l3, a3 = g.last_stats()
    return _state(pkg, lambda which: g.debug_fetch(m, which), g.get_blob(m, with_accum=True), (l3[m], a3[m]))


def _solo_state(pkg, t):
    return _state(pkg, t.debug_fetch, t.get_blob(with_accum=True), t.last_stats())


def _assert_same(got, want, what):
    for key in want:
        assert _bits(got[key], want[key]), "%s: %s differs from the solo trainer's" % (what, key)


def _run_against_solo(pkg, ctx, members, qps, init, nsteps, data=DATA):
    with _group(pkg, ctx, members, qps, init, data) as g:
        g.run(1, nsteps)
        got = [_member_state(pkg, g, m) for m in range(len(members))]
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, qps[m], init[m], data) as t:
            t.run(1, nsteps)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)
    return got


def test_three_members_batch_7(pkg, ctx):
    """smaller than a GEMM tile and odd; seeds, QP lists, dropout and the learning-rate schedule differ (decay inside the run)"""
    members = [dict(batch=7, seed=11), dict(batch=7, seed=12, dropout=False), dict(batch=7, seed=13, lr=0.02, decay_steps=2)]
    got = _run_against_solo(pkg, ctx, members, [[22], [27, 32], [37]], [1, 2, 3], 5)
    assert not _bits(got[0]["blob"], got[1]["blob"]) and set(got[1]["indices"][1::2]) <= {27.0, 32.0}
    assert got[1]["mask_fc1"].min() == 1.0 and got[0]["mask_fc1"].min() == 0.0


def test_two_members_batch_64(pkg, ctx):
    """the reference's batch: fills the 64-row tile exactly"""
    _run_against_solo(pkg, ctx, [dict(batch=64, seed=5), dict(batch=64, seed=6, momentum=0.8)], [[32], [22, 37]], [4, 4], 3)


def test_a_member_does_not_depend_on_k_or_on_its_position(pkg, ctx):
    me, other = dict(batch=7, seed=31), [dict(batch=7, seed=40 + i, lr=0.03) for i in range(3)]
    states = []
    for members, at in (([me], 0), ([me, other[0]], 0), (other + [me], 3)):
        qps = [[27]] * len(members)
        with _group(pkg, ctx, members, qps, [9 if kw is me else 50 for kw in members]) as g:
            g.run(1, 4)
            states.append(_member_state(pkg, g, at))
    _assert_same(states[1], states[0], "member 0 of K = 2 against K = 1")
    _assert_same(states[2], states[0], "member 3 of K = 4 against K = 1")


def test_split_run_and_resume(pkg, ctx):
    members, qps, init = [dict(batch=7, seed=3), dict(batch=7, seed=4, dropout=False)], [[22], [37]], [5, 6]
    with _group(pkg, ctx, members, qps, init) as g:
        g.run(1, 3)
        mid = [g.get_blob(m, with_accum=True) for m in range(2)]
        g.run(4, 3)
        whole = [_member_state(pkg, g, m) for m in range(2)]
    with _group(pkg, ctx, members, qps, init) as g:
        g.run(1, 2)
        g.run(3, 4)
        for m in range(2):
            _assert_same(_member_state(pkg, g, m), whole[m], "run(1, 2) + run(3, 4), member %d" % m)
    with _group(pkg, ctx, members, qps, [0, 0]) as g:  # a fresh group, resumed from the weights and accumulators after step 3
        for m in range(2):
            g.set_blob(m, mid[m][0], mid[m][1])
        g.run(4, 3)
        for m in range(2):
            _assert_same(_member_state(pkg, g, m), whole[m], "resumed at step 4, member %d" % m)


def test_step_indices_with_explicit_batches(pkg, ctx):
    members, init = [dict(batch=7, seed=8), dict(batch=7, seed=9), dict(batch=7, seed=10, dropout=False)], [1, 1, 2]
    rng = np.random.default_rng(5)
    idx = rng.integers(0, NREC, (3, 7)).astype(np.int32)
    idx[1, 4] = idx[1, 1] = idx[1, 0]  # a batch that repeats a sample
    qp = rng.choice([22, 27, 32, 37], (3, 7)).astype(np.int32)
    with _group(pkg, ctx, members, [[32]] * 3, init) as g:
        l3, a3 = g.step_indices(2, idx, qp)
        got = [_member_state(pkg, g, m) for m in range(3)]
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, [32], init[m]) as t:
            sl, sa = t.step_indices(2, idx[m], qp[m])
            assert _bits(l3[m], sl) and _bits(a3[m], sa)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)


def test_evaluate(pkg, ctx):
    """n = 300 is not a multiple of the evaluation piece; every member at its own QP; idx=None and an explicit index array"""
    members, qps, init = [dict(batch=7, seed=1), dict(batch=7, seed=2), dict(batch=7, seed=3)], [22, 32, 37], [7, 8, 9]
    idx = np.random.default_rng(3).integers(0, NVALID, 300)
    with _group(pkg, ctx, members, [[q] for q in qps], init, valid=VALID) as g:
        g.run(1, 2)
        got = [g.evaluate(1, qps, n=300, want_probs=True), g.evaluate(1, qps, idx=idx, want_probs=True)]
        assert got[0][2].shape == (3, 300, 21)
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, [qps[m]], init[m], valid=VALID) as t:
            t.run(1, 2)
            for (l3, a3, probs), want in zip(got, (t.evaluate(1, qps[m], n=300, want_probs=True),
                                                   t.evaluate(1, qps[m], idx=idx, want_probs=True))):
                assert _bits(l3[m], want[0]) and _bits(a3[m], want[1]) and _bits(probs[m], want[2])


def test_tune_2(pkg, ctx, oracle):
    members = [dict(batch=7, seed=21, tune=2), dict(batch=7, seed=22, tune=2)]
    with _group(pkg, ctx, members, [[27], [32]], [3, 4]) as g:
        start = [g.get_blob(m, with_accum=True) for m in range(2)]
    got = _run_against_solo(pkg, ctx, members, [[27], [32]], [3, 4], 3)
    tuned = np.zeros(start[0][0].size, bool)
    for name, shape, off in oracle.TENSORS:
        if name in HEAD32:
            tuned[off // 4: off // 4 + int(np.prod(shape))] = True
    assert tuned.sum() == 2688 * 128 + 128 + 129 * 96 + 96 + 97 * 4 + 4
    for m in range(2):
        assert _bits(got[m]["blob"][~tuned], start[m][0][~tuned]) and _bits(got[m]["accum"][~tuned], start[m][1][~tuned])
        assert not _bits(got[m]["blob"][tuned], start[m][0][tuned])


def test_ldp_members(pkg, ctx):
    """16516-byte records, the QP drawn among the four slots; evaluation at a slot QP and at -1"""
    members, init = [dict(batch=7, seed=14, net="ldp"), dict(batch=7, seed=15, net="ldp", dropout=False)], [2, 3]
    with _group(pkg, ctx, members, [None, None], init, LDP_DATA, LDP_VALID) as g:
        g.run(1, 3)
        got = [_member_state(pkg, g, m) for m in range(2)]
        ev = [g.evaluate(1, [27, -1], n=300, want_probs=True), g.evaluate(1, [-1, 37], n=300, want_probs=True)]
    assert len(set(got[0]["indices"][1::2])) > 1  # mixed slots in one batch
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, None, init[m], LDP_DATA, LDP_VALID) as t:
            t.run(1, 3)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)
            for (l3, a3, probs), qp in zip(ev, ([27, -1][m], [-1, 37][m])):
                want = t.evaluate(1, qp, n=300, want_probs=True)
                assert _bits(l3[m], want[0]) and _bits(a3[m], want[1]) and _bits(probs[m], want[2])


def test_a_sample_set_taken_in_hbm_serves_all_members(pkg, ctx, tmp_path):
    w, h, nframes = 192, 128, 4
    rng = np.random.default_rng(6)
    yuv = str(tmp_path / "seq.yuv")
    rng.integers(0, 256, nframes * w * h * 3 // 2, dtype=np.uint8).tofile(yuv)
    labels = [str(tmp_path / ("qp%d_CUDepth.dat" % q)) for q in (22, 37)]
    for path in labels:
        rng.integers(0, 4, nframes * (h // 16) * (w // 16), dtype=np.uint8).tofile(path)
    members, qps, init = [dict(batch=7, seed=1), dict(batch=7, seed=2)], [[22], [37]], [1, 2]

    def built():
        s = pkg.SampleSet(ctx, "ai", [22, 37])
        s.add_sequence(w, h, yuv, labels)
        return s.build()

    with built() as s:
        host = s.read()
        assert host.size == 24 * 4992
        g = pkg.TrainerGroup(ctx, [pkg.ethcnn.train_options(**kw) for kw in members])
        g.set_samples(0, s, take=True)
        assert len(s) == 0
    with g:
        for m in range(2):
            g.set_qps(m, qps[m])
        g.init_weights(init)
        g.run(1, 3)
        got = [_member_state(pkg, g, m) for m in range(2)]
    with _group(pkg, ctx, members, qps, init, host) as g:
        g.run(1, 3)
        for m in range(2):
            _assert_same(_member_state(pkg, g, m), got[m], "host bytes against the adopted set, member %d" % m)


def test_errors(pkg, ctx):
    E = pkg.EthCnnError
    opts = [pkg.ethcnn.train_options(batch=7, seed=s) for s in (1, 2)]

    def code(fn, *a, **kw):
        with pytest.raises(E) as ei:
            fn(*a, **kw)
        return ei.value.code

    with pkg.Trainer(ctx, batch=7, seed=1) as t, pkg.TrainerGroup(ctx, opts) as g:
        assert code(g.run, 1, 1) == code(t.run, 1, 1) == -1  # no samples
        g.set_samples(0, DATA)
        t.set_samples(0, DATA)
        assert code(g.run, 1, 1) == code(t.run, 1, 1) == -1  # no QP list
        g.set_qps(0, [32])
        assert code(g.run, 1, 1) == -1 and "member 1" in str(pytest.raises(E, g.run, 1, 1).value)
        for m in (-1, 2):
            assert code(g.set_qps, m, [32]) == -1
            assert code(g.get_blob, m) == -1
            assert code(g.set_blob, m, np.zeros(1288210, np.float32)) == -1
            assert code(g.debug_fetch, m, pkg.ethcnn.TDBG_PROBS) == -1
        assert code(g.evaluate, 0, [32, 60], n=10) == -1
        assert code(g.evaluate, 1, [32, 32], n=10) == -1  # no validation set
        g.set_qps(1, [22])
        t.set_qps([32])
        g.run(1, 1)  # without init_weights: the zero weights, as the solo trainer
        t.run(1, 1)
        assert _bits(g.get_blob(0), t.get_blob())
    with pytest.raises(E) as ei:
        pkg.TrainerGroup(ctx, opts + [pkg.ethcnn.train_options(batch=8)])
    assert ei.value.code == -1 and "member 2" in str(ei.value) and "batch" in str(ei.value)
    with pkg.TrainerGroup(ctx, [pkg.ethcnn.train_options(batch=7, net="ldp")] * 2) as g:
        assert code(g.set_qps, 1, [22]) == -1  # LDP: before the samples
        g.set_samples(0, LDP_DATA)
        assert code(g.set_qps, 1, [30]) == -1  # not a slot QP of the set
        assert code(g.evaluate, 0, [22, 30], n=10) == -1
        g.set_qps(1, [22, 37])


def test_driver_model_types(pkg, ctx, oracle, tmp_path):
    """--model-types 1,3: both members' files, equal to two solo driver runs; an exported file predicts like the oracle"""
    (tmp_path / "train.dat").write_bytes(DATA[: 200 * 4992])
    (tmp_path / "valid.dat").write_bytes(VALID[: 200 * 4992])
    drv = os.path.join(ROOT, "hevc-complexity-reduction_amd", "train_CNN_CTU64.py")
    base = [sys.executable, drv, "--train", "train.dat", "--valid", "valid.dat", "--iters", "20", "--batch", "7", "--seed", "4"]

    def run(extra):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    for d in ("grp", "solo1", "solo3"):
        (tmp_path / d).mkdir()
    out = run(["--model-types", "1,3", "--export-ai", "grp", "--models", "G"])
    assert "[qp22] " in out and "[qp32] " in out
    names = {1: ("qp22", pkg.ethcnn.model_name_for_qp(22)), 3: ("qp32", pkg.ethcnn.model_name_for_qp(32))}
    for mt, (name, model) in names.items():
        run(["--model-type", str(mt), "--export-ai", "solo%d" % mt, "--models", "S%d" % mt])
        lines = (tmp_path / "G" / name / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
        assert lines[0] == "20" and lines[-1] == "" and [len(ln.split("  ")) for ln in lines[1:-1]] == [19]
        assert lines == (tmp_path / ("S%d" % mt) / "loss_accuracy_list.dat").read_bytes().decode().split("\r\n")
        got = pkg.ethcnn.read_ckpt_blob(str(tmp_path / "grp" / model))
        assert _bits(got, pkg.ethcnn.read_ckpt_blob(str(tmp_path / ("solo%d" % mt) / model)))
        assert _bits(got, pkg.ethcnn.read_ckpt_blob(str(tmp_path / "G" / name / "model.dat")))
        assert any(f.startswith("model_") and f.endswith("_20_%s.dat.index" % name) for f in os.listdir(str(tmp_path / "G" / name)))
    ctx.load_checkpoint(str(tmp_path / "grp" / names[3][1]))
    ctx.set_thresholds(0.5, 0.5)
    luma = np.random.default_rng(8).integers(0, 256, size=(136, 200), dtype=np.uint8)
    got = ctx.predict_luma(luma, 200, 136, 1, 32)
    want = oracle.predict_frames(ctx.get_blob(), luma, 200, 136, 1, 32, 0.5, 0.5, mode=0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
