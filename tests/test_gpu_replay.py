"""GPU: the sample-set replay (include/ethcnn.h "sample-set replay").  An inter SampleSet cut from seeded residual YUVs and label
files is put back together and run through the deployed Low-Delay-P chain; everything is compared for equality -- the planes byte for
byte with the numpy crop of the files the set was cut from, the probabilities word for word with ctx.ldp_sequence on those files.
Two sequences: 200x136 (3 x 2 whole CTUs, ragged edges dropped) with frames 1..4 and 128x64 with frames 1..3; seeded CNN and LSTM."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extract_cases
import replay_ref
import replay_world
from replay_world import QPS, REC, SEQS
from replay_world import context as _context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL_TOOL = os.path.join(ROOT, "tools", "calibrate_thresholds.py")
SIM_TOOL = os.path.join(ROOT, "tools", "simulate_thresholds.py")
ERR_ARG, ERR_FORMAT, ERR_NOWEIGHTS, ERR_NOMEM = -1, -3, -5, -6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def W(pkg, tmp_path_factory):
    """the context, the files, the set cut from them, its records and the planes the records came from (tests/replay_world.py)"""
    w = replay_world.build(pkg, tmp_path_factory.mktemp("replay"))
    yield w
    w.close()


def crop(W, iseq, slot, first=1):
    """the whole-CTU crop of the planes sequence iseq was cut from, frames first..: (residual, labels)"""
    _, wd, ht, _ = SEQS[iseq]
    R, C = ht // 64, wd // 64
    return (np.ascontiguousarray(W.luma[iseq][slot][first:, :64 * R, :64 * C]), np.ascontiguousarray(W.labels[iseq][slot][first:, :4 * R, :4 * C]))


@pytest.fixture(scope="module")
def deployed(pkg, W):
    """[run][slot] -> (probs, labels) of Replay.run on the set, open gates: computed once, shared, never changed"""
    with pkg.Replay(W.ctx) as rp:
        rp.open(W.set)
        return [[rp.run(i, s) for s in range(4)] for i in range(len(rp))]


# ------------------------------------------------------------------------------------------------------------------ uncut alone ---
def _uncut(pkg, W, d_rec, nrec, run, slot):
    ctx = W.ctx
    n = run["frames"] * run["nctu"]
    d_src, d_resi, d_lab = ctx.alloc(n * 8), ctx.alloc(n * 4096), ctx.alloc(n * 16)
    try:
        d_src.upload(run["src"])
        pkg.ethcnn.replay_uncut_device(ctx, d_rec, nrec, d_src, run["frames"], run["rows"], run["cols"], slot, d_resi, d_lab)
        ctx.synchronize()
        return (d_resi.download(np.uint8, n * 4096).reshape(run["frames"], 64 * run["rows"], 64 * run["cols"]),
                d_lab.download(np.uint8, n * 16).reshape(run["frames"], 4 * run["rows"], 4 * run["cols"]))
    finally:
        for b in (d_src, d_resi, d_lab):
            b.free()


def test_uncut_gives_back_the_planes_at_every_source_offset(pkg, W):
    n = len(W.records)
    offsets = {(81 + 4113 * s + 16516 * i) % 16 for i in range(n) for s in range(4)}
    assert offsets == set(range(16)) and n >= 4
    assert [(r["seq"], r["frames"], r["nctu"]) for r in W.plan] == [(0, 4, 6), (1, 3, 2)]
    # the last record ends with its allocation: the word behind its slot-3 residual does not exist
    exact = W.ctx.alloc(n * REC)
    # the inter records' own alignment: 4 bytes
    shifted = W.ctx.alloc(n * REC + 16)
    try:
        exact.upload(W.records)
        shifted.upload(np.concatenate([np.zeros(4, np.uint8), W.records.reshape(-1)]))
        assert exact.ptr % 16 == 0 and shifted.ptr % 16 == 0
        for base in (exact.ptr, shifted.ptr + 4):
            for iseq, run in enumerate(W.plan):
                for slot in range(4):
                    got = _uncut(pkg, W, base, n, run, slot)
                    want = crop(W, iseq, slot)
                    assert np.array_equal(got[0], want[0]), (base % 16, iseq, slot)
                    assert np.array_equal(got[1], want[1]), (base % 16, iseq, slot)
                    ref = replay_ref.planes(W.records, run, slot)
                    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1])
    finally:
        exact.free()
        shifted.free()


def test_uncut_never_reads_outside_the_records(pkg, W):
    run = dict(W.plan[1])
    run["src"] = run["src"].copy()
    run["src"][0, 1], run["src"][2, 0] = len(W.records), -1  # what a caller's table could hold: zeros come back
    d = W.ctx.alloc(len(W.records) * REC)
    try:
        d.upload(W.records)
        got = _uncut(pkg, W, d, len(W.records), run, 2)
    finally:
        d.free()
    want = [x.copy() for x in crop(W, 1, 2)]
    want[0][0, :, 64:], want[1][0, :, 4:] = 0, 0
    want[0][2, :, :64], want[1][2, :, :4] = 0, 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for bad in (dict(slot=4), dict(rows=0), dict(cols=1024)):
        a = dict(slot=0, rows=1, cols=2)
        a.update(bad)
        with pytest.raises(pkg.EthCnnError) as e:
            pkg.ethcnn.replay_uncut_device(W.ctx, 16, 1, 16, 1, a["rows"], a["cols"], a["slot"], 16, 16)
        assert e.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ the replay ---
def test_order_independence(pkg, W, deployed):
    with pkg.Replay(W.ctx) as rp:
        for source in (W.set, W.set.read(), W.set.read(seed=3)):
            rp.open(source)
            runs = rp.runs()
            assert [(r["seq"], r["w"], r["h"], r["f0"], r["frames"], r["nctu"], r["qps"]) for r in runs] == \
                [(0, 200, 136, 1, 4, 6, QPS), (1, 128, 64, 1, 3, 2, QPS)]
            for i in range(len(runs)):
                for s in range(4):
                    probs, labels = rp.run(i, s)
                    assert np.array_equal(_bits(probs), _bits(deployed[i][s][0])), (i, s)
                    assert np.array_equal(labels, deployed[i][s][1]) and np.array_equal(labels, crop(W, i, s)[1]), (i, s)


def test_as_deployed(pkg, W, deployed):
    _, wd, ht, frames = SEQS[0]
    whole = [line * 4 + col for line in range(2) for col in range(3)]  # the 3 x 2 whole CTUs of the 4 x 3 of a 200x136 picture
    for s in range(4):
        full = W.ctx.ldp_sequence(np.ascontiguousarray(W.luma[0][s][1:]), wd, ht, frames - 1, QPS[s], i_frame_first=1)
        assert full.shape == (4, 12, 21)
        assert np.array_equal(_bits(deployed[0][s][0]), _bits(full[:, whole])), s
    assert len({deployed[0][s][0].tobytes() for s in range(4)}) == 4  # the slots are different pictures and QPs
    # closed gates: the cropped picture's result
    W.ctx.set_thresholds(0.4, 0.3)
    try:
        with pkg.Replay(W.ctx) as rp:
            rp.open(W.set)
            for i, (_, wd, ht, frames) in enumerate(SEQS):
                resi = crop(W, i, 2)[0]
                want = W.ctx.ldp_sequence(resi, resi.shape[2], resi.shape[1], frames - 1, QPS[2], i_frame_first=1)
                assert np.array_equal(_bits(rp.run(i, 2)[0]), _bits(want)), i
    finally:
        W.ctx.set_thresholds(0.0, 0.0)


def test_runs_are_independent_and_start_from_a_zero_state(pkg, W, deployed):
    fresh = _context(pkg)
    try:
        with pkg.Replay(fresh) as rp:
            got = rp.open(W.records).run(1, 1)  # run 1 first, on a context that has seen nothing
        assert np.array_equal(_bits(got[0]), _bits(deployed[1][1][0])) and np.array_equal(got[1], deployed[1][1][1])
    finally:
        fresh.close()
    # a file that starts at frame 3 of the first sequence: zeros in front of frame 3, whatever state the context holds
    late = W.records[12:]
    resi = crop(W, 0, 3, first=3)[0]
    assert resi.shape[0] == 2
    zeros = np.zeros((6, 2, 448), np.float32)
    want = W.ctx.ldp_sequence(resi, 192, 128, 2, QPS[3], i_frame_first=3, state_in=zeros)
    with pkg.Replay(W.ctx) as rp:
        rp.open(late)
        assert [(r["f0"], r["frames"]) for r in rp.runs()] == [(3, 2), (1, 3)]
        rp.run(1, 0)  # leaves a state of another CTU count resident
        a = rp.run(0, 3)[0]
        W.ctx.ldp_sequence(resi, 192, 128, 2, QPS[0], i_frame_first=1)  # leaves a state of the same CTU count resident
        b = rp.run(0, 3)[0]
    assert np.array_equal(_bits(a), _bits(want)) and np.array_equal(_bits(b), _bits(want))
    assert not np.array_equal(_bits(want), _bits(deployed[0][3][0][2:]))  # (the state does matter)


def test_chunking(pkg, W, deployed):
    with pkg.Replay(W.ctx) as rp:
        rp.open(W.set)
        for chunk in (2, 1, 3, 0):
            rp.set_chunk_frames(chunk)
            for i, s in ((0, 1), (1, 2)):
                probs, labels = rp.run(i, s)
                assert np.array_equal(_bits(probs), _bits(deployed[i][s][0])), (chunk, i, s)
                assert np.array_equal(labels, deployed[i][s][1]), (chunk, i, s)
        with pytest.raises(pkg.EthCnnError) as e:
            rp.set_chunk_frames(-1)
        assert e.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------- consumers ---
def test_feed_calibrator_and_simulator(pkg, W, deployed):
    e = pkg.ethcnn
    with pkg.Replay(W.ctx) as rp, pkg.Calibrator(W.ctx) as fed, pkg.Calibrator(W.ctx) as host, pkg.PartitionSim(W.ctx) as sfed, \
            pkg.PartitionSim(W.ctx) as shost:
        rp.open(W.set.read(seed=9))
        rp.feed(fed, slot=2)
        rp.feed(sfed, qp=32)
        rp.feed(fed, runs=[1], slot=0)
        for i, s in ((0, 2), (1, 2)):
            _, wd, ht, _ = SEQS[i]
            host.add_frames(deployed[i][s][0], deployed[i][s][1], wd // 64 * 64, ht // 64 * 64)
            shost.add_frames(deployed[i][s][0], deployed[i][s][1], wd // 64 * 64, ht // 64 * 64)
        host.add_frames(deployed[1][0][0], deployed[1][0][1], 128, 64)
        assert np.array_equal(fed.histogram(), host.histogram()) and int(fed.histogram()[0].sum()) == 24 + 6 + 6
        assert sfed.info() == shost.info() and sfed.info()["labelled_ctus"] == 30
        cands = e.sim_thr([[1024, 1024, 1024], [614, 717, 819]], [[-1, -1, -1], [410, 307, 205]])
        for gates in ("none", "ldp"):
            assert sfed.eval(cands, gates).tobytes() == shost.eval(cands, gates).tobytes()
        with pytest.raises(ValueError):
            rp.feed(fed, qp=30)
        with pytest.raises(TypeError):
            rp.feed(object(), slot=0)


@pytest.fixture(scope="module")
def files(pkg, W):
    """LDP_Valid.dat and its _shuffled form, a model directory with the context's weights, a Thr_info.txt in LDP order"""
    e = pkg.ethcnn
    models = W.dir / "models"
    models.mkdir()
    e.write_ckpt_blob(str(models / "model_LDP_2000000_qp22~37.dat"), W.ctx.get_blob())
    e.write_ckpt_lstm_blob(str(models / e.lstm_model_name_for_qp(32)), W.ctx.get_lstm_blob())
    plain, shuffled, thr = str(W.dir / "LDP_Valid.dat"), str(W.dir / "LDP_Valid_shuffled.dat"), str(W.dir / "Thr_info.txt")
    W.set.write(plain)
    W.set.write(shuffled, seed=5)
    assert np.fromfile(plain, np.uint8).tobytes() != np.fromfile(shuffled, np.uint8).tobytes()
    with open(thr, "w") as f:
        f.write("0.4 0.6 0.3 0.7 0.2 0.8\n")
    return plain, shuffled, str(models), thr


def _tool(argv):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


def test_calibration_tool_end_to_end(pkg, W, files, deployed):
    plain, shuffled, models, _ = files
    out = [_tool([CAL_TOOL, "--json", "--eps-down", "100000", "100000", "100000", "--samples", path, "--ldp", "--model-dir", models, "--qp", "32"])
           for path in (plain, shuffled)]
    assert out[0].stdout == out[1].stdout
    assert out[0].stderr == out[1].stderr and "sequence 0: 200x136 (3 x 2 whole CTUs), frames 1..4, 24 CTUs" in out[0].stderr
    assert "sequence 1: 128x64 (2 x 1 whole CTUs), frames 1..3, 6 CTUs" in out[0].stderr
    with pkg.Calibrator(W.ctx) as cal:
        for i in range(2):
            cal.add_frames(deployed[i][2][0], deployed[i][2][1], SEQS[i][1] // 64 * 64, SEQS[i][2] // 64 * 64)
        want = cal.choose([100000] * 3, [50000] * 3).as_dicts()
    assert json.loads(out[0].stdout)["levels"] == json.loads(json.dumps(want))


def test_simulation_tool_end_to_end(pkg, W, files, deployed):
    plain, shuffled, models, thr = files
    out = [_tool([SIM_TOOL, "--thr-info", thr, "--order", "ldp", "--json", "--samples", path, "--ldp", "--model-dir", models, "--qp", "32"])
           for path in (plain, shuffled)]
    assert out[0].stdout == out[1].stdout
    got = json.loads(out[0].stdout)
    e = pkg.ethcnn
    with pkg.PartitionSim(W.ctx) as sim:
        for i in range(2):
            sim.add_frames(deployed[i][2][0], deployed[i][2][1], SEQS[i][1] // 64 * 64, SEQS[i][2] // 64 * 64)
        want = sim.eval(e.sim_thr([614, 717, 819], [410, 307, 205]), "ldp")[0]
        assert got["info"] == json.loads(json.dumps(sim.info())) and got["info"]["ctus"] == 30
    assert got["checked"] == [int(x) for x in want["checked"]] and got["bad_ctus"] == int(want["bad_ctus"])


# ----------------------------------------------------------------------------------------------------------- errors and hygiene ---
def test_errors_leave_the_object_usable(pkg, W, deployed, tmp_path):
    before = W.set.read()
    bare = pkg.EthCnn(device=0)
    try:
        with pkg.Replay(bare) as rp:
            with pytest.raises(pkg.EthCnnError) as e:
                rp.run(0, 0)
            assert e.value.code == ERR_ARG and "nothing is open" in str(e.value)
            rp.open(W.records)
            for load in (lambda: None, lambda: bare.load_synthetic(31, 8.0)):  # no CNN; a CNN and no LSTM bundle
                load()
                with pytest.raises(pkg.EthCnnError) as e:
                    rp.run(0, 0)
                assert e.value.code == ERR_NOWEIGHTS
            bare.load_lstm_synthetic(32, 3.0)
            bare.set_thresholds(0.0, 0.0)
            assert np.array_equal(_bits(rp.run(0, 0)[0]), _bits(deployed[0][0][0]))
    finally:
        bare.close()
    with pkg.Replay(W.ctx) as rp:
        rp.open(W.set)
        for run, slot in ((2, 0), (-1, 0), (0, 4), (0, -1)):
            with pytest.raises(pkg.EthCnnError) as e:
                rp.run_device(run, slot)
            assert e.value.code == ERR_ARG
        # ERR_FORMAT: an All-Intra set, a set that is not built, bytes that are not whole records, an invalid run
        yuv, lab = str(tmp_path / "ai.yuv"), str(tmp_path / "ai_CUDepth.dat")
        with open(yuv, "wb") as f:
            f.write(extract_cases.synth_yuv(np.random.default_rng(1), 64, 64, 1))
        with open(lab, "wb") as f:
            f.write(bytes(16))
        with pkg.SampleSet(W.ctx, kind="ai", qps=[32]) as ai, pkg.SampleSet(W.ctx, kind="inter", qps=QPS) as unbuilt:
            ai.add_sequence(64, 64, yuv, [lab])
            ai.build()
            for bad in (ai, unbuilt, W.records.reshape(-1)[:-1], b"", np.delete(W.records, 10, axis=0)):
                with pytest.raises(pkg.EthCnnError) as e:
                    rp.open(bad)
                assert e.value.code == ERR_FORMAT, str(e.value)
                assert len(rp) == 0  # a failed open leaves nothing open ...
        assert "record 6 breaks rule 'missing'" in str(e.value)
        rp.open(W.set)                # ... and the object usable
        assert np.array_equal(_bits(rp.run(1, 3)[0]), _bits(deployed[1][3][0]))
    assert np.array_equal(W.set.read(), before)  # the source set is only read


def test_memory_limit(pkg, W, deployed):
    with pkg.Replay(W.ctx) as rp:
        rp.open(W.set)
        need = [rp.run_bytes(i, own_probs=True, own_labels=True) for i in range(2)]
        assert need[0] == 4 * 6 * (4096 + 8 + 84 + 16) and need[1] == 3 * 2 * (4096 + 8 + 84 + 16)
        assert rp.run_bytes(0) == 4 * 6 * (4096 + 8)
        rp.set_chunk_frames(1)
        assert rp.run_bytes(0) == 6 * 4096 + 4 * 6 * 8
    with pkg.Replay(W.ctx) as rp:  # host records: their copy counts; a run behind frame 1 holds a zero state
        rp.open(W.records[12:])
        assert rp.run_bytes(0) == 18 * REC + 2 * 6 * (4096 + 8) + 6 * 3584
    with pkg.Replay(W.ctx, max_bytes=need[0] - 1) as rp, pkg.Calibrator(W.ctx) as cal:
        rp.open(W.set)
        with pytest.raises(pkg.EthCnnError) as e:
            rp.feed(cal, runs=[0], slot=1)
        assert e.value.code == ERR_NOMEM and ("needs %d bytes" % need[0]) in str(e.value)
        assert int(cal.histogram().sum()) == 0
        rp.feed(cal, runs=[1], slot=1)  # the smaller run fits: the object is usable
        assert int(cal.histogram()[0].sum()) == 6
        assert np.array_equal(_bits(rp.run(0, 1)[0]), _bits(deployed[0][1][0]))  # with the caller's buffers the sum is smaller
    with pkg.Replay(W.ctx, max_bytes=need[0]) as rp, pkg.Calibrator(W.ctx) as cal:
        rp.open(W.set)
        rp.feed(cal, slot=1)
        assert int(cal.histogram()[0].sum()) == 30
    with pkg.Replay(W.ctx, max_bytes=len(W.records) * REC - 1) as rp:
        with pytest.raises(pkg.EthCnnError) as e:
            rp.open(W.records)
        assert e.value.code == ERR_NOMEM and str(len(W.records) * REC) in str(e.value)
