"""GPU: the ETH-LSTM trainer group (include/ethcnn.h "ETH-LSTM training, several models at once") against solo LstmTrainers created
in the same test with the same options and weights, their own set_qps and their own upload of the same bytes.  Every comparison is
bit for bit.  Data: seeded synthetic samples (tests/train_data_lstm.py) that carry four QPs, so members with different QP lists keep
different and unequal numbers of samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_data_ldp
import train_data_lstm
import train_ref_lstm as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = 37264
DATA = train_data_lstm.make_samples(300, seed=21)
VALID = train_data_lstm.make_samples(700, seed=22)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _group(pkg, ctx, members, qps, init, data=DATA, valid=None):
    """members: LstmTrainer keyword dicts; qps: per member QP lists ([]: keep all); init: per member weight seeds"""
    g = pkg.LstmTrainerGroup(ctx, [pkg.ethcnn.lstm_train_options(**kw) for kw in members])
    for m, q in enumerate(qps):
        g.set_qps(m, q)
    kept = g.set_samples(0, data)
    assert kept == [len(pkg.ethcnn.lstm_select_qp(data, q)) for q in qps] == [g.num_samples(m, 0) for m in range(len(members))]
    if valid is not None:
        g.set_samples(1, valid)
    g.init_weights(init)
    return g


def _solo(pkg, ctx, kw, qps, init, data=DATA, valid=None):
    t = pkg.LstmTrainer(ctx, **kw)
    t.set_qps(qps)
    t.set_samples(0, data)
    if valid is not None:
        t.set_samples(1, valid)
    t.init_weights(init)
    return t


def _state(pkg, fetch, blob_accum, stats):
    e = pkg.ethcnn
    blob, accum = blob_accum
    out = {"blob": blob, "accum": accum, "loss": stats[0], "acc": stats[1]}
    for name, which in (("indices", e.LDBG_INDICES), ("mask_h", e.LDBG_MASK_H), ("mask_fc2", e.LDBG_MASK_FC2), ("probs", e.LDBG_PROBS),
                        ("grads", e.LDBG_GRADS), ("norm", e.LDBG_NORM), ("state_c", e.LDBG_STATE_C), ("state_h", e.LDBG_STATE_H)):
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
    """one partial 16-sample slice, 140 rows (partial 64-row GEMM tiles); QP lists, seeds, dropout, qp_scale and the learning-rate
    schedule differ (a decay inside the run)"""
    members = [dict(batch=7, seed=11, qp_scale=0.18), dict(batch=7, seed=12, dropout=False), dict(batch=7, seed=13, lr=0.05, decay_steps=2)]
    qps = [[22], [27, 32], []]
    got = _run_against_solo(pkg, ctx, members, qps, [1, 2, 3], 5)
    keep = [pkg.ethcnn.lstm_select_qp(DATA, q) for q in qps]
    assert len(set(len(k) for k in keep)) == 3 and len(keep[2]) == 300
    for m in range(3):  # the indices are the member's own kept indices, drawn over its own count
        assert np.array_equal(got[m]["indices"], R.batch_of(members[m]["seed"], 5, 7, len(keep[m])))
    assert not _bits(got[0]["blob"], got[1]["blob"])
    assert got[1]["mask_h"].min() == 1.0 and got[0]["mask_h"].min() == 0.0


def test_two_members_batch_20(pkg, ctx):
    """two 16-sample slices, the second 4 wide"""
    _run_against_solo(pkg, ctx, [dict(batch=20, seed=5), dict(batch=20, seed=6, momentum=0.8)], [[37], [22, 27]], [4, 5], 3)


def test_two_members_batch_64(pkg, ctx):
    """the reference's batch"""
    _run_against_solo(pkg, ctx, [dict(batch=64, seed=5), dict(batch=64, seed=6, clip_norm=2.0)], [[32], [22, 37]], [4, 4], 3)


def test_a_member_does_not_depend_on_k_or_on_its_position(pkg, ctx):
    me, other = dict(batch=7, seed=31), [dict(batch=7, seed=40 + i, lr=0.03) for i in range(3)]
    states = []
    for members, at in (([me], 0), ([me, other[0]], 0), (other + [me], 3)):
        qps = [[27] if kw is me else [22, 32] for kw in members]
        with _group(pkg, ctx, members, qps, [9 if kw is me else 50 for kw in members]) as g:
            g.run(1, 4)
            states.append(_member_state(pkg, g, at))
    _assert_same(states[1], states[0], "member 0 of K = 2 against K = 1")
    _assert_same(states[2], states[0], "member 3 of K = 4 against K = 1")


def test_clipping_is_per_member(pkg, ctx):
    """test_gpu_train_lstm.py::test_clip_and_update's recipe (fc2 / fc3 matrices x 4 at batch 2: the restatement's global norm is
    6.6 .. 7.9 there, 0.7 .. 0.8 with the plain initialisation): member 0 is clipped, member 1 stays under the clip, member 2 has the
    scaled weights and clip_norm = 0"""
    members = [dict(batch=2, seed=1, lr=0.05), dict(batch=2, seed=2, lr=0.05), dict(batch=2, seed=1, lr=0.05, clip_norm=0.0)]
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 300, (3, 2)).astype(np.int32)
    idx[2] = idx[0]
    a0 = (rng.standard_normal(R.FLOATS) * 1e-3).astype(np.float32)
    with _group(pkg, ctx, members, [[]] * 3, [6, 6, 6]) as g:
        plain = g.get_blob(0)
        scaled = plain.copy()
        for n, (off, cnt) in R.OFFS.items():
            if "fc3/full_connect_w" in n or "fc2/full_connect_w" in n:
                scaled[off: off + cnt] *= np.float32(4.0)
        blobs = [scaled, plain, scaled]
        for m in range(3):
            g.set_blob(m, blobs[m], a0)
        l3, a3 = g.step_indices(3, idx)
        got = [_member_state(pkg, g, m) for m in range(3)]
    norms = [float(s["norm"][0]) for s in got]
    print("global norms", norms)
    assert norms[0] > 5.0 and norms[1] < 5.0 and _bits(got[2]["norm"], got[0]["norm"]) and _bits(got[2]["grads"], got[0]["grads"])
    assert not _bits(got[2]["accum"], got[0]["accum"])  # the same gradient, clipped in member 0 only
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, [], 6) as t:
            t.set_blob(blobs[m], a0)
            sl, sa = t.step_indices(3, idx[m])
            assert _bits(l3[m], sl) and _bits(a3[m], sa)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)


def test_split_run_and_resume(pkg, ctx):
    members, qps, init = [dict(batch=7, seed=3), dict(batch=7, seed=4, dropout=False)], [[22], [37, 27]], [5, 6]
    with _group(pkg, ctx, members, qps, init) as g:
        g.run(1, 2)
        mid = [g.get_blob(m, with_accum=True) for m in range(2)]
        g.run(3, 2)
        split = [_member_state(pkg, g, m) for m in range(2)]
    with _group(pkg, ctx, members, qps, init) as g:
        g.run(1, 4)
        for m in range(2):
            _assert_same(split[m], _member_state(pkg, g, m), "run(1, 2) + run(3, 2) against run(1, 4), member %d" % m)
    with _group(pkg, ctx, members, qps, [0, 0]) as g:  # a new group, resumed from the weights and accumulators after step 2
        for m in range(2):
            g.set_blob(m, mid[m][0], mid[m][1])
        g.run(3, 2)
        for m in range(2):
            _assert_same(_member_state(pkg, g, m), split[m], "resumed at step 3, member %d" % m)


def test_step_indices_with_explicit_batches(pkg, ctx):
    members, qps, init = [dict(batch=7, seed=8), dict(batch=7, seed=9), dict(batch=7, seed=10, dropout=False)], [[22], [], [32, 37]], [1, 1, 2]
    rng = np.random.default_rng(5)
    counts = [len(pkg.ethcnn.lstm_select_qp(DATA, q)) for q in qps]
    idx = np.stack([rng.integers(0, n, 7) for n in counts]).astype(np.int32)
    idx[1, 4] = idx[1, 1] = idx[1, 0]  # a batch that repeats a sample
    idx[0, 0], idx[0, 1] = 0, counts[0] - 1  # the member's first and last kept sample
    with _group(pkg, ctx, members, qps, init) as g:
        l3, a3 = g.step_indices(2, idx)
        got = [_member_state(pkg, g, m) for m in range(3)]
        bad = idx.copy()
        bad[0, 3] = counts[0]  # inside the set, outside member 0's kept range
        with pytest.raises(pkg.EthCnnError) as ei:
            g.step_indices(3, bad)
        assert ei.value.code == -1 and "member 0" in str(ei.value)
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, qps[m], init[m]) as t:
            sl, sa = t.step_indices(2, idx[m])
            assert _bits(l3[m], sl) and _bits(a3[m], sa)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)


def test_evaluate_on_the_validation_set(pkg, ctx):
    """n = 300: one full piece of 256 samples and one of 44; idx per member from its own kept range, with replacement; idx=None with
    n = the smallest kept count; the training state is untouched"""
    members, qps, init = [dict(batch=7, seed=1), dict(batch=7, seed=2, qp_scale=0.18), dict(batch=7, seed=3)], [[22], [27, 37], []], [7, 8, 9]
    counts = [len(pkg.ethcnn.lstm_select_qp(VALID, q)) for q in qps]
    assert min(counts) < 256 < 300 < max(counts) == 700
    rng = np.random.default_rng(3)
    idx = np.stack([rng.integers(0, n, 300) for n in counts]).astype(np.int32)
    with _group(pkg, ctx, members, qps, init, valid=VALID) as g:
        assert [g.num_samples(m, 1) for m in range(3)] == counts
        g.run(1, 2)
        before = [g.get_blob(m, with_accum=True) for m in range(3)]
        got = [g.evaluate(1, idx=idx, want_probs=True), g.evaluate(1, n=min(counts), want_probs=True)]
        assert got[0][2].shape == (3, 300 * 20, 21) and got[1][2].shape == (3, min(counts) * 20, 21)
        with pytest.raises(pkg.EthCnnError):
            g.evaluate(1, n=min(counts) + 1)
        for m in range(3):
            after = g.get_blob(m, with_accum=True)
            assert _bits(after[0], before[m][0]) and _bits(after[1], before[m][1])
        g.run(3, 1)
        trained = [g.get_blob(m) for m in range(3)]
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, qps[m], init[m], valid=VALID) as t:
            t.run(1, 2)
            for (l3, a3, probs), want in zip(got, (t.evaluate(1, idx=idx[m], want_probs=True),
                                                   t.evaluate(1, n=min(counts), want_probs=True))):
                assert _bits(l3[m], want[0]) and _bits(a3[m], want[1]) and _bits(probs[m], want[2])
            t.run(3, 1)
            assert _bits(trained[m], t.get_blob())


def test_upload_failures_leave_the_previous_set(pkg, ctx):
    """A label of 4 in a sample only member 1 keeps: ERR_FORMAT, "member 1: " + the message of that member's own solo upload (which
    names the sample).  The same bytes under QP lists that keep it nowhere are accepted.  An empty selection: the solo code, the
    member named.  After each failure the set uploaded before still trains, as if nothing had happened."""
    E = pkg.EthCnnError
    members, init = [dict(batch=7, seed=1), dict(batch=7, seed=2)], [3, 4]
    raw = np.frombuffer(DATA, np.uint8).reshape(-1, REC)[:40].copy()
    q0 = raw[:, 64:68].copy().view(np.float32)[:, 0]
    s = int(np.flatnonzero(q0 == 27.0)[2])
    bad = raw.copy()
    bad[:, 64:].view(np.float32).reshape(40, 20, 465)[s, 3, 6] = 4.0
    def solo_error(qps, data):  # what that member's own upload says
        with pkg.LstmTrainer(ctx, batch=7) as t:
            t.set_qps(qps)
            with pytest.raises(E) as solo:
                t.set_samples(0, data)
        return solo.value.code, str(solo.value).split(": ", 1)[1]

    with _group(pkg, ctx, members, [[22], [27]], init) as g:
        g.run(1, 1)
        code, msg = solo_error([27], bad)
        assert code == -3 and msg.startswith("sample %d:" % s)
        with pytest.raises(E) as ei:
            g.set_samples(0, bad)
        assert ei.value.code == -3 and str(ei.value).endswith(": member 1: " + msg)
        g.run(2, 1)
        g.set_qps(1, [5])
        code, msg = solo_error([5], raw)
        with pytest.raises(E) as ei:
            g.set_samples(0, raw)
        assert ei.value.code == code == -3 and str(ei.value).endswith(": member 1: " + msg)
        assert [g.num_samples(m, 0) for m in range(2)] == [len(pkg.ethcnn.lstm_select_qp(DATA, q)) for q in ([22], [27])]
        g.run(3, 1)
        got = [_member_state(pkg, g, m) for m in range(2)]
        g.set_qps(0, [22])
        g.set_qps(1, [32, 37])  # nobody keeps sample s now
        assert g.set_samples(0, bad) == [len(pkg.ethcnn.lstm_select_qp(bad, q)) for q in ([22], [32, 37])]
        g.run(4, 1)
        assert np.isfinite(g.last_stats()[0]).all()
    for m, kw in enumerate(members):
        with _solo(pkg, ctx, kw, [[22], [27]][m], init[m]) as t:
            t.run(1, 3)
            _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)


def test_an_adopted_sample_set_serves_both_members(pkg):
    """LDP records (tests/train_data_ldp.py, 192 x 128, 42 frames: 18 heads a slot) through a synthetic residual CNN
    (Trainer(net="ldp").init_weights(7)): a two-slot LstmSampleSet is taken by a K = 2 group; each member equals a solo trainer fed
    its one-slot set"""
    e = pkg.EthCnn(device=0)
    try:
        with pkg.Trainer(e, batch=8, net="ldp") as c:
            c.init_weights(7)
            e.load_blob(c.get_blob())
        per = 6
        rec = np.frombuffer(train_data_ldp.make_records(per * 42, seed=5, width=192, height=128), np.uint8).reshape(-1, 16516).copy()
        rec[:, 10:14] = (np.arange(per * 42) // per).astype("<u4").view(np.uint8).reshape(-1, 4)
        slot_qps = [int(rec[0, 64 + 4113 * s]) for s in range(4)]
        members, slots, init = [dict(batch=7, seed=1), dict(batch=7, seed=2)], [0, 2], [1, 2]
        g = pkg.LstmTrainerGroup(e, [pkg.ethcnn.lstm_train_options(**kw) for kw in members])
        with g:
            for m, s in enumerate(slots):
                g.set_qps(m, [slot_qps[s]])
            with pkg.LstmSampleSet(e, slots=slots) as ls:
                ls.build_from(rec)
                assert ls.count == 36
                assert g.set_samples(0, ls, take=True) == [18, 18]
                assert len(ls) == 0
            g.init_weights(init)
            g.run(1, 3)
            got = [_member_state(pkg, g, m) for m in range(2)]
        for m, kw in enumerate(members):
            with pkg.LstmTrainer(e, **kw) as t, pkg.LstmSampleSet(e, slots=[slots[m]]) as ls:
                t.set_qps([slot_qps[slots[m]]])
                assert t.set_samples(0, ls.build_from(rec), take=True) == 18
                t.init_weights(init[m])
                t.run(1, 3)
                _assert_same(got[m], _solo_state(pkg, t), "member %d" % m)
    finally:
        e.close()


def test_errors(pkg, ctx):
    E = pkg.EthCnnError
    opts = [pkg.ethcnn.lstm_train_options(batch=7, seed=s) for s in (1, 2)]

    def code(fn, *a, **kw):
        with pytest.raises(E) as ei:
            fn(*a, **kw)
        return ei.value.code

    with pkg.LstmTrainerGroup(ctx, opts) as g:
        assert code(g.run, 1, 1) == -1  # no samples
        for m in (-1, 2):
            assert code(g.set_qps, m, [32]) == -1
            assert code(g.get_blob, m) == -1
            assert code(g.set_blob, m, np.zeros(R.FLOATS, np.float32)) == -1
            assert code(g.debug_fetch, m, pkg.ethcnn.LDBG_NORM) == -1
            assert g.num_samples(m, 0) == -1
        assert code(g.set_samples, 0, DATA[:-1]) == -3
        assert code(g.evaluate, 1, n=4) == -1  # no validation set
    with pytest.raises(E) as ei:
        pkg.LstmTrainerGroup(ctx, opts + [pkg.ethcnn.lstm_train_options(batch=8)])
    assert ei.value.code == -1 and "member 2" in str(ei.value) and "batch" in str(ei.value)


def test_driver_qps(pkg, ctx, tmp_path):
    """--qps 22,32: both members' files, byte-identical to the files of the two --qp runs; the exported models load"""
    (tmp_path / "train.dat").write_bytes(DATA)
    (tmp_path / "valid.dat").write_bytes(VALID[: 300 * REC])
    drv = os.path.join(ROOT, "hevc-complexity-reduction_amd", "train_LSTM_CTU64.py")
    base = [sys.executable, drv, "--train", "train.dat", "--valid", "valid.dat", "--iters", "4", "--batch", "7", "--seed", "3"]

    def run(extra):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    def same_files(a, b):
        fa = sorted(f for f in os.listdir(os.path.dirname(a)) if f.startswith(os.path.basename(a)))
        fb = sorted(f for f in os.listdir(os.path.dirname(b)) if f.startswith(os.path.basename(b)))
        assert len(fa) >= 2 and [f[len(os.path.basename(a)):] for f in fa] == [f[len(os.path.basename(b)):] for f in fb]
        for x, y in zip(fa, fb):
            with open(os.path.join(os.path.dirname(a), x), "rb") as f1, open(os.path.join(os.path.dirname(b), y), "rb") as f2:
                assert f1.read() == f2.read(), (x, y)

    for d in ("grp", "solo22", "solo32"):
        (tmp_path / d).mkdir()
    out = run(["--qps", "22,32", "--export-lstm", "grp", "--models", "G"])
    assert "[qp22] " in out and "[qp32] " in out
    for qp in (22, 32):
        name, model = "qp%d" % qp, pkg.ethcnn.lstm_model_name_for_qp(qp)
        run(["--qp", str(qp), "--export-lstm", "solo%d" % qp, "--models", "S%d" % qp])
        same_files(str(tmp_path / "G" / name / "model.dat"), str(tmp_path / ("S%d" % qp) / "model.dat"))
        same_files(str(tmp_path / "grp" / model), str(tmp_path / ("solo%d" % qp) / model))
        with open(str(tmp_path / "G" / name / "loss_accuracy_list.dat"), "rb") as f1, \
                open(str(tmp_path / ("S%d" % qp) / "loss_accuracy_list.dat"), "rb") as f2:
            assert f1.read() == f2.read()
        ctx.load_lstm_checkpoint(str(tmp_path / "grp" / model))
        assert _bits(ctx.get_lstm_blob(), pkg.ethcnn.read_ckpt_lstm_blob(str(tmp_path / "G" / name / "model.dat")))
