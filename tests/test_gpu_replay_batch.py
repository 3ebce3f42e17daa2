"""-m gpu: several runs of an inter sample set through one LdpBatch (include/ethcnn.h "sample-set replay", the batch entries) against
the definition: per item the outputs equal Replay.run on a context with that item's bundle, word for word, and a consumer fed through
the batch ends in the state the per-run feeds leave.  The record set is made by hand: three runs of different geometry, length and first
frame number -- 64x64 (1 CTU) frames 3..4, 192x128 (6 CTUs) frames 1..5, 448x256 (28 CTUs) frames 2..4 --, four QP slots, records in
shuffled order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_ref
from replay_world import context as _context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL_TOOL = os.path.join(ROOT, "tools", "calibrate_thresholds.py")
ERR_ARG, ERR_NOWEIGHTS, ERR_NOMEM = -1, -5, -6
RUNS = ((0, 64, 64, 3, 2), (1, 192, 128, 1, 5), (2, 448, 256, 2, 3))  # seq, width, height, first frame number, frames
SLOT_QPS = (22, 27, 32, 37)
BUNDLES = [(41, 3.0), (42, 0.5)]  # LSTM seed, head gain
# (run, slot, bundle): every run, a run twice with different slots, both bundles
ITEMS = [(0, 0, 0), (1, 1, 1), (2, 2, 0), (1, 3, 0), (2, 0, 1), (0, 2, 1)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _records():
    rng = np.random.default_rng(93)
    recs = []
    for seq, w, h, f0, nf in RUNS:
        for f in range(f0, f0 + nf):
            for line in range(h // 64):
                for col in range(w // 64):
                    r = np.full(replay_ref.REC, 255, np.uint8)
                    r[2:6] = np.array([w, h], "<u2").view(np.uint8)
                    r[10:14] = np.array([f], "<u4").view(np.uint8)
                    r[14:20] = np.array([line, col, seq], "<u2").view(np.uint8)
                    for s, qp in enumerate(SLOT_QPS):
                        at = replay_ref.SLOT_BASE + replay_ref.SLOT_BYTES * s
                        r[at] = qp
                        r[at + 1:at + 17] = rng.integers(0, 4, 16)
                        r[at + 17:at + 17 + 4096] = rng.integers(0, 256, 4096) // (1 + 7 * ((f + col) % 2)) + 100 * ((f + col) % 2)
                    recs.append(r)
    rec = np.stack(recs)
    return rec[np.random.default_rng(94).permutation(len(rec))]


@pytest.fixture(scope="module")
def world(pkg):
    """the context (seeded CNN, open gates), the records and, per (run, slot, bundle) of ITEMS and of the feed tests, Replay.run on the
    context loaded with that bundle: computed once, never changed"""
    ctx = _context(pkg)
    rec = _records()
    plan = replay_ref.plan(rec)
    assert [(r["w"], r["h"], r["f0"], r["frames"], r["nctu"]) for r in plan] == [(64, 64, 3, 2, 1), (192, 128, 1, 5, 6), (448, 256, 2, 3, 28)]
    want = {}
    with pkg.Replay(ctx) as rp:
        rp.open(rec)
        for bi, (seed, gain) in enumerate(BUNDLES):
            ctx.load_lstm_synthetic(seed, gain)
            for run, slot, b in ITEMS + [(i, 2, 0) for i in range(3)]:
                if b == bi and (run, slot, b) not in want:
                    want[(run, slot, b)] = rp.run(run, slot)
                    assert np.array_equal(want[(run, slot, b)][1], replay_ref.planes(rec, plan[run], slot)[1])
    ctx.load_lstm_synthetic(*BUNDLES[0])
    yield ctx, rec, want
    ctx.close()


def _batch(pkg, ctx):
    b = pkg.LdpBatch(ctx, len(BUNDLES))
    for i, (seed, gain) in enumerate(BUNDLES):
        b.load_lstm_synthetic(i, seed, gain)
    return b


def test_a_batch_of_runs_equals_the_replay_of_each(pkg, world):
    ctx, rec, want = world
    with pkg.Replay(ctx) as rp, _batch(pkg, ctx) as b:
        rp.open(rec)
        for chunk in (0, 1, 2):
            rp.set_chunk_frames(chunk)
            got = rp.run_batch(ITEMS, b)
            for item, (probs, labels) in zip(ITEMS, got):
                assert probs.shape == want[item][0].shape and np.array_equal(_bits(probs), _bits(want[item][0])), (chunk, item)
                assert np.array_equal(labels, want[item][1]), (chunk, item)
        one = rp.run_batch(ITEMS[2:3], b)  # an item alone, at another sequence index than before
        assert np.array_equal(_bits(one[0][0]), _bits(want[ITEMS[2]][0]))
        # the memory sum: the records, per item the chunk's planes and the source table, one zero state for the largest run with f0 > 1
        runs = [it[0] for it in ITEMS]
        geo = {0: (1, 2), 1: (6, 5), 2: (28, 3)}  # run -> (CTUs, frames)
        for chunk in (0, 1, 2):
            rp.set_chunk_frames(chunk)
            fc = chunk if chunk else max(1, (256 << 20) // (sum(geo[r][0] for r in runs) * 4096))
            assert rp.run_batch_bytes(runs, b) == rec.nbytes + sum(min(geo[r][1], fc) * geo[r][0] * 4096 + geo[r][1] * geo[r][0] * 8 for r in runs) + 28 * 3584
        rp.set_chunk_frames(0)
        assert rp.run_batch_bytes([1], b) == rec.nbytes + 5 * 6 * 4096 + 5 * 6 * 8  # (run 1 starts at frame 1: no zero state)
        for bad, code in (([(3, 0, 0)], ERR_ARG), ([(0, 4, 0)], ERR_ARG), ([(0, 0, 2)], ERR_NOWEIGHTS), ([], ERR_ARG), ([(0, 0, 0)] * 33, ERR_ARG)):
            with pytest.raises(pkg.EthCnnError) as e:
                rp.run_batch(bad, b)
            assert e.value.code == code, bad
        rp.set_chunk_frames(0)
        again = rp.run_batch(ITEMS, b)  # usable behind the refusals
        assert all(np.array_equal(_bits(p), _bits(want[item][0])) for item, (p, _) in zip(ITEMS, again))
    small = pkg.Replay(ctx, max_bytes=rec.nbytes + 100000)
    try:
        small.open(rec)
        with _batch(pkg, ctx) as b:
            with pytest.raises(pkg.EthCnnError) as e:
                small.run_batch(ITEMS, b)
            assert e.value.code == ERR_NOMEM and "limit" in str(e.value)
    finally:
        small.close()


def test_feed_through_a_batch_leaves_the_consumers_as_the_per_run_feeds_do(pkg, world):
    ctx, rec, want = world
    e = pkg.ethcnn
    order = [2, 0, 1]
    with pkg.Replay(ctx) as rp, _batch(pkg, ctx) as b, pkg.Calibrator(ctx) as one, pkg.Calibrator(ctx) as many, pkg.PartitionSim(ctx) as sone, \
            pkg.PartitionSim(ctx) as smany:
        rp.open(rec)
        ctx.load_lstm_synthetic(*BUNDLES[0])
        rp.feed(one, runs=order, slot=2)
        rp.feed(sone, runs=order, qp=32)
        rp.feed(many, runs=order, slot=2, batch=b)
        rp.feed(smany, runs=order, qp=32, batch=b, bundle_of=lambda run, slot: 0)
        assert np.array_equal(one.histogram(), many.histogram()) and int(many.histogram()[0].sum()) == 2 * 1 + 5 * 6 + 3 * 28
        assert smany.info() == sone.info() and smany.info()["labelled_ctus"] == 116
        cands = e.sim_thr([[1024, 1024, 1024], [614, 717, 819]], [[-1, -1, -1], [410, 307, 205]])
        for gates in ("none", "ldp"):
            assert smany.eval(cands, gates).tobytes() == sone.eval(cands, gates).tobytes()
            a, c = smany.decide(cands[1:2], gates), sone.decide(cands[1:2], gates)
            for k in ("codes", "reach", "depth"):
                assert np.array_equal(a[k], c[k]), (gates, k)
        # the other bundle through bundle_of: what the context gives with that bundle loaded
        with pkg.Calibrator(ctx) as host, pkg.Calibrator(ctx) as fed:
            rp.feed(fed, runs=[1], slot=1, batch=b, bundle_of=lambda run, slot: 1)
            host.add_frames(want[(1, 1, 1)][0], want[(1, 1, 1)][1], 192, 128)
            assert np.array_equal(fed.histogram(), host.histogram())
    # packing: a limit that holds one run at a time still feeds them all, in order
    tight = pkg.Replay(ctx, max_bytes=rec.nbytes + 28 * 3 * (4096 + 8 + 100) + 28 * 3584 + 4096)
    try:
        tight.open(rec)
        with _batch(pkg, ctx) as b, pkg.PartitionSim(ctx) as packed, pkg.PartitionSim(ctx) as sone:
            assert [len(p) for p in tight._pack(order, b)] == [1, 2]
            tight.feed(packed, runs=order, slot=2, batch=b)
            tight.feed(sone, runs=order, slot=2)
            assert packed.info() == sone.info()
            assert packed.eval(cands, "ldp").tobytes() == sone.eval(cands, "ldp").tobytes()
    finally:
        tight.close()


def test_calibration_tool_with_batch_prints_and_writes_the_same(pkg, world, tmp_path):
    ctx, rec, want = world
    e = pkg.ethcnn
    models = tmp_path / "models"
    models.mkdir()
    ctx.load_lstm_synthetic(*BUNDLES[0])
    e.write_ckpt_blob(str(models / "model_LDP_2000000_qp22~37.dat"), ctx.get_blob())
    e.write_ckpt_lstm_blob(str(models / e.lstm_model_name_for_qp(32)), ctx.get_lstm_blob())
    path = str(tmp_path / "LDP_Valid_shuffled.dat")
    rec.tofile(path)
    outs = []
    for extra in ([], ["--batch"]):
        thr, hist = str(tmp_path / ("Thr_info%d.txt" % len(outs))), str(tmp_path / ("hist%d.bin" % len(outs)))
        r = subprocess.run([sys.executable, CAL_TOOL, "--json", "--eps-down", "100000", "100000", "100000", "--out", thr, "--order", "ldp", "--hist", hist,
                            "--samples", path, "--ldp", "--model-dir", str(models), "--qp", "32"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout.replace(thr, "THR").replace(hist, "HIST"), r.stderr.replace(thr, "THR").replace(hist, "HIST"),
                     open(thr, "rb").read(), open(hist, "rb").read()))
    assert outs[0] == outs[1]
    assert "sequence 2: 448x256 (7 x 4 whole CTUs), frames 2..4, 84 CTUs" in outs[1][1] and json.loads(outs[1][0])["levels"]
    with pkg.Calibrator(ctx) as cal:
        for i in range(3):
            cal.add_frames(want[(i, 2, 0)][0], want[(i, 2, 0)][1], RUNS[i][1], RUNS[i][2])
        assert json.loads(outs[1][0])["levels"] == json.loads(json.dumps(cal.choose([100000] * 3, [50000] * 3).as_dicts()))
