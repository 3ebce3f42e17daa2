"""GPU: a solo trainer steps through the device-resident member table of its engine (K = 1).  What a solo call changes in that
table -- the QP list, the sample sets -- has to reach the next step, and an evaluation, which works on tables of its own, must leave
it alone.  Every comparison is bit for bit; batch 7; data: seeded synthetic records (tests/train_data*.py)."""
import functools

import numpy as np
import pytest

import train_data
import train_data_ldp
import train_data_lstm
import train_ref
import train_ref_lstm as R

pytestmark = pytest.mark.gpu

B = 7


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cnn_state(pkg, t):
    blob, accum = t.get_blob(with_accum=True)
    loss, acc = t.last_stats()
    return {"blob": blob, "accum": accum, "loss": loss, "acc": acc, "indices": t.debug_fetch(pkg.ethcnn.TDBG_INDICES),
            "grads": t.debug_fetch(pkg.ethcnn.TDBG_GRADS), "mask_fc1": t.debug_fetch(pkg.ethcnn.TDBG_MASK_FC1)}


def _lstm_state(pkg, t):
    blob, accum = t.get_blob(with_accum=True)
    loss, acc = t.last_stats()
    return {"blob": blob, "accum": accum, "loss": loss, "acc": acc, "indices": t.debug_fetch(pkg.ethcnn.LDBG_INDICES),
            "grads": t.debug_fetch(pkg.ethcnn.LDBG_GRADS), "mask_h": t.debug_fetch(pkg.ethcnn.LDBG_MASK_H)}


def _assert_same(got, want, what):
    for key in want:
        assert _bits(got[key], want[key]), "%s: %s differs" % (what, key)


@functools.lru_cache(None)
def _ai(n, seed):
    return train_data.make_records(n, seed=seed)


@functools.lru_cache(None)
def _lstm_kept(nkept, nother, seed, qp=27):
    """LSTM samples in file order of which exactly nkept have the slot-0 QP `qp`, spread among nother others"""
    pool = np.frombuffer(train_data_lstm.make_samples(8 * (nkept + nother), seed=seed), np.uint8).reshape(-1, train_data_lstm.REC)
    q0 = pool[:, 64:68].copy().view(np.float32)[:, 0]
    on, off = np.flatnonzero(q0 == qp)[:nkept], np.flatnonzero(q0 != qp)[:nother]
    assert on.size == nkept and off.size == nother
    return pool[np.sort(np.concatenate([on, off]))].tobytes()


def test_cnn_qp_list_changed_between_runs(pkg, ctx):
    """steps 1-3 at QP 22, set_qps([37]) with the steps still in flight, steps 4-6: the new list reaches step 4"""
    nrec, seed = 300, 17
    data = _ai(nrec, 31)

    def trainer(qps):
        t = pkg.Trainer(ctx, batch=B, dropout=True, seed=seed)
        t.set_samples(0, data)
        t.set_qps(qps)
        t.init_weights(3)
        return t

    with trainer([22]) as a:
        a.run(1, 3)
        a.set_qps([37])  # no synchronisation in between
        a.run(4, 3)
        got = _cnn_state(pkg, a)
    idx, qp = train_ref.batch_of(seed, 6, B, nrec, [37])
    assert np.array_equal(got["indices"][0::2], idx) and np.array_equal(got["indices"][1::2], qp) and set(qp) == {37}
    with trainer([22]) as r:  # the same three steps again (the trainer is deterministic): the state after step 3
        r.run(1, 3)
        mid = r.get_blob(with_accum=True)
    with trainer([37]) as b:  # [37] from the start, resumed from that state
        b.set_blob(*mid)
        b.run(4, 3)
        _assert_same(got, _cnn_state(pkg, b), "set_qps between two runs against [37] from the start")


def test_ldp_training_set_replaced(pkg, ctx):
    """a QP list of one slot QP, then a training set with other slot QPs: the list is the four new slots again"""
    seed, new_qps = 23, (20, 25, 30, 35)
    first = train_data_ldp.make_records(200, seed=41)
    second = train_data_ldp.make_records(150, seed=42, qps=new_qps)
    with pkg.Trainer(ctx, batch=B, dropout=True, seed=seed, net="ldp") as a:
        a.set_samples(0, first)
        a.set_qps([27])
        a.init_weights(5)
        a.run(1, 2)
        assert set(a.debug_fetch(pkg.ethcnn.TDBG_INDICES)[1::2]) == {27.0}
        mid = a.get_blob(with_accum=True)
        a.set_samples(0, second)
        a.run(3, 1)
        got = _cnn_state(pkg, a)
        with pytest.raises(pkg.EthCnnError):
            a.set_qps([27])  # no longer a slot QP
    idx, qp = train_ref.batch_of(seed, 3, B, 150, list(new_qps))
    assert np.array_equal(got["indices"][0::2], idx) and np.array_equal(got["indices"][1::2], qp)
    with pkg.Trainer(ctx, batch=B, dropout=True, seed=seed, net="ldp") as b:
        b.set_samples(0, second)
        b.set_blob(*mid)
        b.run(3, 1)
        _assert_same(got, _cnn_state(pkg, b), "a replaced training set against a fresh trainer on it")


def test_lstm_training_set_replaced_by_one_with_another_kept_count(pkg, ctx):
    """a QP list that keeps a subset: 40 kept samples, then 9 (not a multiple of the batch)"""
    seed = 29
    first, second = _lstm_kept(40, 25, 51), _lstm_kept(9, 14, 52)

    def trainer():
        t = pkg.LstmTrainer(ctx, batch=B, dropout=True, seed=seed)
        t.set_qps([27])
        return t

    with trainer() as a:
        assert a.set_samples(0, first) == 40
        a.init_weights(7)
        a.run(1, 2)
        assert np.array_equal(a.debug_fetch(pkg.ethcnn.LDBG_INDICES), R.batch_of(seed, 2, B, 40))
        assert a.set_samples(0, second) == 9 and a.num_samples(0) == 9
        a.run(3, 1)
        got = _lstm_state(pkg, a)
        assert np.array_equal(got["indices"], R.batch_of(seed, 3, B, 9))
        ev = a.evaluate(0, n=9, want_probs=True)
        with pytest.raises(pkg.EthCnnError):
            a.evaluate(0, n=10)
    with trainer() as b:
        assert b.set_samples(0, second) == 9
        b.set_blob(got["blob"])
        for x, y in zip(ev, b.evaluate(0, n=9, want_probs=True)):
            assert _bits(x, y)


@pytest.mark.parametrize("net", ["cnn", "lstm"])
def test_an_evaluation_between_two_runs_leaves_the_step_alone(pkg, ctx, net):
    """an evaluation over two pieces (CNN 1024 + 3, LSTM 256 + 3) with a shuffled index list, between step 2 and step 3"""
    if net == "cnn":
        n, state = 1027, _cnn_state
        data, valid = _ai(300, 31), _ai(n, 32)

        def trainer():
            t = pkg.Trainer(ctx, batch=B, dropout=True, seed=13)
            t.set_qps([22, 37])
            return t

        def evaluate(t, idx):
            return t.evaluate(1, 32, idx=idx, want_probs=True)
    else:
        n, state = 259, _lstm_state
        data, valid = train_data_lstm.make_samples(60, seed=61), train_data_lstm.make_samples(n, seed=62)

        def trainer():
            return pkg.LstmTrainer(ctx, batch=B, dropout=True, seed=13)

        def evaluate(t, idx):
            return t.evaluate(1, idx=idx, want_probs=True)
    idx = np.random.default_rng(9).permutation(n)
    states = []
    for with_eval in (True, False):
        with trainer() as t:
            t.set_samples(0, data)
            t.set_samples(1, valid)
            t.init_weights(11)
            t.run(1, 2)
            if with_eval:
                probs = evaluate(t, idx)[2]
                assert np.isfinite(probs).all() and probs.shape[0] == (n if net == "cnn" else 20 * n)
            t.run(3, 1)
            states.append(state(pkg, t))
    _assert_same(states[0], states[1], "step 3 after an evaluation against step 3 without it")
