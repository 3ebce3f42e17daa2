"""CPU: the host plan of the sample-set replay (ethcnn_replay_plan; include/ethcnn.h "sample-set replay") against its numpy
restatement tests/replay_ref.py: runs, f0, F and the source table in any record order, and every rule of an invalid file with the
record it names.  Records are synthesised in numpy (tests/extract_cases.np_cut_inter)."""
import numpy as np
import pytest

import extract_cases
import replay_ref

REC = replay_ref.REC
QPS = [22, 27, 32, 37]
ERR_FORMAT = -3


def sequence(w, h, frames, seq, rng):
    """the records of one sequence, frame after frame, CTUs in raster order; frames: the frame numbers"""
    n = len(frames)
    lumas = [rng.integers(0, 256, (n, h, w), dtype=np.uint8) for _ in QPS]
    labels = [rng.integers(0, 4, (n, h // 16, w // 16), dtype=np.uint8) for _ in QPS]
    return extract_cases.np_cut_inter(lumas, labels, QPS, list(frames), seq)


@pytest.fixture(scope="module")
def rec():
    """200x136 (3 x 2 whole CTUs, ragged edges dropped) frames 1..4 as sequence 0, 128x64 frames 1..3 as sequence 1: 24 + 6 records"""
    rng = np.random.default_rng(5)
    out = np.concatenate([sequence(200, 136, range(1, 5), 0, rng), sequence(128, 64, range(1, 4), 1, rng)])
    assert out.shape == (30, REC)
    return out


def same_plan(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in ("seq", "w", "h", "rows", "cols", "f0", "frames", "nctu", "qps"):
            assert g[k] == w[k], k
        assert g["src"].dtype == np.int64 and np.array_equal(g["src"], w["src"])


def test_plain_order(pkg, rec):
    got = pkg.ethcnn.replay_plan(rec)
    same_plan(got, replay_ref.plan(rec))
    assert [(r["seq"], r["w"], r["h"], r["rows"], r["cols"], r["f0"], r["frames"]) for r in got] == [(0, 200, 136, 2, 3, 1, 4), (1, 128, 64, 1, 2, 1, 3)]
    assert np.array_equal(got[0]["src"].reshape(-1), np.arange(24)) and np.array_equal(got[1]["src"].reshape(-1), 24 + np.arange(6))
    assert got[0]["qps"] == QPS
    same_plan(pkg.ethcnn.replay_plan(rec.tobytes()), got)  # bytes as the source


def test_any_record_order_gives_the_same_planes(pkg, rec):
    plain = pkg.ethcnn.replay_plan(rec)
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(rec))
        shuffled = rec[order]
        got = pkg.ethcnn.replay_plan(shuffled)
        same_plan(got, replay_ref.plan(shuffled))
        for g, p in zip(got, plain):  # the same plan up to the source indices
            assert np.array_equal(order[g["src"]], p["src"])
            for slot in range(4):
                a, b = replay_ref.planes(shuffled, g, slot), replay_ref.planes(rec, p, slot)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_runs_are_ordered_by_seq_then_first_appearance(pkg, rec):
    swapped = np.concatenate([rec[24:], rec[:24]])  # sequence 1 comes first in the file, and still second in the plan
    got = pkg.ethcnn.replay_plan(swapped)
    same_plan(got, replay_ref.plan(swapped))
    assert [r["seq"] for r in got] == [0, 1] and got[0]["src"][0, 0] == 6
    twin = swapped.copy()
    twin[:6, 18] = 0  # the 128x64 records now carry seq 0 as well: another geometry is another run, first appearance decides
    got = pkg.ethcnn.replay_plan(twin)
    same_plan(got, replay_ref.plan(twin))
    assert [(r["seq"], r["w"]) for r in got] == [(0, 128), (0, 200)]


def test_a_file_that_starts_at_frame_3(pkg, rec):
    late = rec[12:]
    got = pkg.ethcnn.replay_plan(late)
    same_plan(got, replay_ref.plan(late))
    assert (got[0]["f0"], got[0]["frames"]) == (3, 2) and (got[1]["f0"], got[1]["frames"]) == (1, 3)


def refused(pkg, bad, record, rule):
    with pytest.raises(replay_ref.ReplayFormat) as ref:
        replay_ref.plan(bad)
    assert (ref.value.record, ref.value.rule) == (record, rule)
    with pytest.raises(pkg.EthCnnError) as e:
        pkg.ethcnn.replay_plan(bad)
    assert e.value.code == ERR_FORMAT
    assert ("record %d breaks rule '%s'" % (record, rule)) in str(e.value), str(e.value)


def test_one_record_removed(pkg, rec):
    # (frame 2, line 1, col 1) = record 10 is gone: shown by the lowest record of the run from frame 2 on, (2, 0, 0), still record 6
    refused(pkg, np.delete(rec, 10, axis=0), 6, "missing")
    # the very first place of a run: its lowest record is now (1, 0, 1)
    refused(pkg, rec[1:], 0, "missing")
    # the last place of a run: only the records of the last frame show it
    refused(pkg, np.delete(rec, 23, axis=0), 18, "missing")
    order = np.random.default_rng(3).permutation(len(rec) - 1)
    bad = np.delete(rec, 10, axis=0)[order]
    with pytest.raises(replay_ref.ReplayFormat) as ref:
        replay_ref.plan(bad)
    refused(pkg, bad, ref.value.record, "missing")


def test_one_record_duplicated(pkg, rec):
    refused(pkg, np.concatenate([rec, rec[7:8]]), 30, "duplicate")
    refused(pkg, np.concatenate([rec[:3], rec[25:26], rec[3:]]), 26, "duplicate")  # the higher record of the pair is named


def test_a_frame_gap(pkg, rec):
    # frame 3 of the 200x136 run is gone: shown by the lowest record of frame 4
    refused(pkg, np.concatenate([rec[:12], rec[18:]]), 12, "missing")


def test_a_position_outside_the_whole_ctus(pkg, rec):
    bad = rec.copy()
    bad[9, 16] = 3  # col 3 of a picture 3 CTUs wide (the ragged column that is never cut)
    refused(pkg, bad, 9, "outside")
    bad = rec.copy()
    bad[26, 14] = 1  # line 1 of a picture one CTU high
    refused(pkg, bad, 26, "outside")


def test_a_qp_byte_changed_in_one_record(pkg, rec):
    bad = rec.copy()
    bad[13, 64 + 4113 * 2] = 33
    refused(pkg, bad, 13, "QP differs")
    bad = rec.copy()
    bad[0, 64] = 23  # the run's lowest record is the reference: the next one differs from it
    refused(pkg, bad, 1, "QP differs")


def test_two_slots_with_equal_qps(pkg, rec):
    bad = rec.copy()
    bad[24:, 64 + 4113 * 3] = 22  # slots 0 and 3 of the second run
    refused(pkg, bad, 24, "QPs not distinct")


def test_geometry_and_byte_counts(pkg, rec):
    bad = rec.copy()
    bad[24:, 2] = 60  # 60 x 64: no whole CTU
    bad[24:, 3] = 0
    refused(pkg, bad, 24, "geometry")
    for raw in (b"", rec.tobytes()[:-1], rec.tobytes() + b"\0"):
        with pytest.raises(pkg.EthCnnError) as e:
            pkg.ethcnn.replay_plan(raw)
        assert e.value.code == ERR_FORMAT and "whole number" in str(e.value)


def test_rules_are_reported_in_their_order(pkg, rec):
    bad = np.concatenate([rec, rec[0:1]])  # a duplicate at record 30 ...
    bad[20, 16] = 5                        # ... and a position outside, which also leaves a hole: 'outside' comes first
    refused(pkg, bad, 20, "outside")


# ---- the tools' command line: --samples FILE --ldp --model-dir D --qp Q
def _tool(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tools_take_a_replayed_sample_file():
    cal, sim = _tool("calibrate_thresholds"), _tool("simulate_thresholds")
    argv = ["--samples", "LDP_Valid.dat", "--ldp", "--model-dir", "models", "--qp", "32"]
    want = {"kind": "samples", "file": "LDP_Valid.dat", "net": "ai", "ldp": True, "model_dir": "models", "qp": 32}
    assert cal.parse(argv)[1] == [want]
    assert sim.parse(["--sweep", "up0"] + argv)[1] == [want]
    # the trainer's evaluation keeps its form
    old = cal.parse(["--samples", "f.dat", "--model", "m", "--qp", "32", "--net", "ldp"])[1]
    assert old == [{"kind": "samples", "file": "f.dat", "net": "ldp", "ldp": False, "model": "m", "qp": 32}]
    for bad in (["--samples", "f", "--ldp", "--qp", "32"], ["--samples", "f", "--ldp", "--model-dir", "d"],
                ["--samples", "f", "--ldp", "--model", "m", "--model-dir", "d", "--qp", "32"], ["--samples", "f", "--model-dir", "d", "--model", "m", "--qp", "32"],
                ["--case", "l", "p", "64", "64", "--ldp"]):
        with pytest.raises(cal.Usage):
            cal.parse(bad)
