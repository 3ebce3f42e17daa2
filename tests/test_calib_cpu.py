"""CPU: the host side of the threshold calibrator (include/ethcnn.h "threshold calibration").  The numpy restatement of the histogram
(tests/calib_ref.py) is pinned to the existing scorer (tools/score_cu_depth.py); ethcnn_calib_choose is compared with the restatement
of the choice, on random and on hand-worked histograms, and its maximality is asserted directly; the Thr_info.txt writer is read back
by the library's own parser and by a C "%f" parse.  Counts and thresholds are integers and compared for equality; the report's four
quotients are compared to the rounding of their float64 division."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import calib_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("score_cu_depth", os.path.join(ROOT, "tools", "score_cu_depth.py"))
sc = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sc)

INT_FIELDS = ("n0", "n1", "down_k", "up_k", "miss", "fsplit", "uncertain", "empty_class", "crossed")
FLOAT_FIELDS = ("down", "up", "uncertain_share", "accuracy_512")


def _check_against_ref(pkg, hist, eps_down, eps_up):
    got = pkg.ethcnn.calib_choose(hist, eps_down, eps_up).as_dicts()
    want = ref.choose(hist, eps_down, eps_up)
    for l in range(3):
        for f in INT_FIELDS:
            assert got[l][f] == want[l][f], (l, f, got[l], want[l])
        for f in FLOAT_FIELDS:  # quotients of the same integers: the library rounds both to float64 and divides (three roundings of
            # 2^-53 relative; one where the counts are below 2^53), Python divides the integers exactly
            assert abs(got[l][f] - want[l][f]) <= 4 * 2.0 ** -53 * abs(want[l][f]), (l, f, got[l], want[l])
    return got


def _one_level(h0, h1):
    """the same (h0, h1) = ({bin: count}, {bin: count}) on all three levels"""
    hist = np.zeros((3, 2, ref.BINS), np.uint64)
    for t, h in enumerate((h0, h1)):
        for b, v in h.items():
            hist[:, t, b] = v
    return hist


def test_reference_histogram_is_the_scorers_count():
    rng = np.random.default_rng(5)
    n = 5000
    probs, depth = ref.edge_probs(rng, n), ref.random_depths(rng, n)
    assert (probs == 0).any() and (probs == 1).any() and (probs == np.nextafter(np.float32(0), np.float32(1))).any()
    assert (probs == np.nextafter(np.float32(0.5), np.float32(0))).any() and (probs == np.nextafter(np.float32(0.5), np.float32(1))).any()
    hist, rejected = ref.histogram(probs, depth)
    assert not rejected.any()
    assert all(hist[l, t].sum() > 0 for l in range(3) for t in (0, 1))
    for k in (0, 1, 511, 512, 513, 1023):
        assert sc.class_matrices(depth, probs, (k / 1024.0,) * 3) == ref.matrices_at(hist, k), k


def test_reference_frame_gather_is_the_scorers_on_whole_ctu_frames():
    rng = np.random.default_rng(6)
    w, h, frames = 128, 192, 3
    labels = rng.integers(0, 4, size=(frames + 1, h // 16, w // 16)).astype(np.uint8)
    probs = rng.random((frames, 6, 21), dtype=np.float32)
    p, d, skipped = ref.gather_frames(probs, labels, w, h, skip_label_frames=1)
    assert skipped == 0 and np.array_equal(d, sc.labels_per_ctu(labels[1:])) and np.array_equal(p, probs.reshape(-1, 21))
    p, d, skipped = ref.gather_frames(rng.random((2, 4 * 3, 21), dtype=np.float32), rng.integers(0, 4, size=(3, 9, 13)), 208, 144, 1)
    assert p.shape == (12, 21) and d.shape == (12, 16) and skipped == 12


def test_choose_matches_reference_on_random_histograms(pkg):
    rng = np.random.default_rng(7)
    for case in range(12):
        hist = np.zeros((3, 2, ref.BINS), np.uint64)
        for l in range(3):
            for t in (0, 1):
                if case % 3 == 0:    # two overlapping bumps
                    centre, width, m = (300, 150, 4000) if t == 0 else (700, 150, 3000)
                    b = np.clip(np.rint(rng.normal(centre + 40 * l, width, m)), 0, 1024).astype(np.int64)
                    hist[l, t] = np.bincount(b, minlength=ref.BINS)
                elif case % 3 == 1:  # sparse, huge counts: products above 2^64
                    hist[l, t, rng.integers(0, ref.BINS, 20)] = rng.integers(1, 2 ** 58, 20, dtype=np.uint64)
                else:                # dense uniform noise
                    hist[l, t] = rng.integers(0, 50, ref.BINS)
        eps_down = [int(x) for x in rng.choice([0, 1, 1000, 50000, 300000, 1000000], 3)]
        eps_up = [int(x) for x in rng.choice([0, 1, 1000, 50000, 300000, 1000000], 3)]
        got = _check_against_ref(pkg, hist, eps_down, eps_up)
        # budgets hold and the choice is maximal, asserted directly on the histogram
        for l in range(3):
            h0, h1 = [int(x) for x in hist[l, 0]], [int(x) for x in hist[l, 1]]
            n0, n1, dk, uk = sum(h0), sum(h1), got[l]["down_k"], got[l]["up_k"]
            miss, fsplit = (lambda k: sum(h1[:k + 1])), (lambda k: sum(h0[k + 1:]))
            assert miss(dk) * 10 ** 6 <= eps_down[l] * n1 and fsplit(uk) * 10 ** 6 <= eps_up[l] * n0
            assert got[l]["miss"] == miss(dk) and got[l]["fsplit"] == fsplit(uk)
            if not got[l]["crossed"]:
                assert dk <= uk
                assert dk == 1024 or miss(dk + 1) * 10 ** 6 > eps_down[l] * n1
                assert uk == 0 or fsplit(uk - 1) * 10 ** 6 > eps_up[l] * n0
            else:
                assert dk == uk


def test_choose_hand_worked(pkg):
    # N1 = N0 = 1000; a budget of 1000 ppm allows exactly one error: miss * 10^6 == eps * N1 is inside the budget
    hist = _one_level({5: 998, 990: 1, 1000: 1}, {10: 1, 20: 1, 900: 998})
    got = _check_against_ref(pkg, hist, [1000] * 3, [1000] * 3)
    assert [(g["down_k"], g["up_k"], g["miss"], g["fsplit"], g["crossed"]) for g in got] == [(19, 990, 1, 1, 0)] * 3
    assert got[0]["uncertain"] == 1 + 998 + 1 and got[0]["n0"] == got[0]["n1"] == 1000
    assert got[0]["down"] == 19 / 1024.0 and got[0]["up"] == 990 / 1024.0
    # one part per million less: that one error is over the budget
    got = _check_against_ref(pkg, hist, [999] * 3, [999] * 3)
    assert [(g["down_k"], g["up_k"], g["miss"], g["fsplit"]) for g in got] == [(9, 1000, 0, 0)] * 3
    # per-level budgets are per level
    got = _check_against_ref(pkg, hist, [1000, 999, 2000], [999, 1000, 2000])
    # (2000 ppm: two errors, down_k = 899 > up_k = 5: crossed; miss + fsplit is 2 on 5..9, 3 on 10..19, 4 on 20..899)
    assert [(g["down_k"], g["up_k"], g["crossed"]) for g in got] == [(19, 1000, 0), (9, 990, 0), (5, 5, 1)]


def test_choose_never_current_only(pkg):
    # truly split samples at p == 0 and no budget: even k = 0 misses them, so down_k = -1 ("p <= -1/1024" never holds)
    hist = _one_level({0: 10, 100: 10}, {0: 5, 800: 95})
    got = _check_against_ref(pkg, hist, [0] * 3, [0] * 3)
    assert [(g["down_k"], g["up_k"], g["miss"], g["fsplit"]) for g in got] == [(-1, 100, 0, 0)] * 3
    assert got[0]["down"] == -1 / 1024.0 and got[0]["uncertain"] == 10 + 10 + 5


def test_choose_crossing_with_a_tie(pkg):
    # budgets of 20 %: down_k = 699 (miss 10 of 100), up_k = 200 (fsplit 10 of 100): crossed.  miss + fsplit over [200, 699] is 10 on
    # 200..299, 20 on 300..599 and 10 on 600..699: the lowest k of the tie wins
    hist = _one_level({200: 90, 600: 10}, {300: 10, 700: 90})
    got = _check_against_ref(pkg, hist, [200000] * 3, [200000] * 3)
    assert [(g["down_k"], g["up_k"], g["crossed"], g["miss"], g["fsplit"], g["uncertain"]) for g in got] == [(200, 200, 1, 0, 10, 0)] * 3


def test_choose_empty_class_and_empty_level(pkg):
    hist = _one_level({100: 50, 400: 50}, {})
    hist[2] = 0
    got = _check_against_ref(pkg, hist, [50000] * 3, [50000] * 3)
    assert [g["empty_class"] for g in got] == [1, 1, 1] and got[0]["n1"] == 0 and got[2]["n0"] == 0
    assert 0 <= got[0]["up_k"] <= 1024 and -1 <= got[0]["down_k"] <= 1024
    assert got[2]["accuracy_512"] == 0.0 and got[2]["uncertain_share"] == 0.0


def test_choose_rejects_bad_arguments(pkg):
    hist = np.zeros((3, 2, ref.BINS), np.uint64)
    with pytest.raises(ValueError):
        pkg.ethcnn.calib_choose(hist, [1000001, 0, 0], [0, 0, 0])
    lib = pkg.load_library()
    eps = (ctypes.c_uint32 * 3)(0, 0, 2000000)
    rep = pkg.ethcnn.CalibReport()
    assert lib.ethcnn_calib_choose(hist.ctypes.data, eps, eps, ctypes.byref(rep)) == pkg.ethcnn.ERR_ARG
    assert b"parts per million" in lib.ethcnn_last_error(None)
    assert lib.ethcnn_calib_choose(None, eps, eps, ctypes.byref(rep)) == pkg.ethcnn.ERR_ARG
    assert lib.ethcnn_calib_write_thr_info(b"/nonexistent-dir/Thr_info.txt", ctypes.byref(rep), 0) == pkg.ethcnn.ERR_IO
    assert lib.ethcnn_calib_write_thr_info(b"x", ctypes.byref(rep), 2) == pkg.ethcnn.ERR_ARG


def _sscanf6(line):
    libc = ctypes.CDLL(None)
    v = [ctypes.c_float() for _ in range(6)]
    assert libc.sscanf(line, b"%f %f %f %f %f %f", *[ctypes.byref(x) for x in v]) == 6
    return [np.float32(x.value) for x in v]


@pytest.mark.parametrize("order", ["ai", "ldp"])
def test_thr_info_file_reads_back_exactly(pkg, tmp_path, order):
    rng = np.random.default_rng(9)
    cases = [[(-1, 0), (0, 1024), (1024, 1024)], [(1, 1023), (511, 513), (341, 683)]]
    cases += [[tuple(sorted(int(k) for k in rng.integers(0, 1025, 2))) for _ in range(3)] for _ in range(6)]
    for ks in cases:
        rep = pkg.ethcnn.CalibReport()
        for l, (dk, uk) in enumerate(ks):
            rep.level[l].down_k, rep.level[l].up_k = dk, uk
        path = str(tmp_path / "Thr_info.txt")
        pkg.ethcnn.write_thr_info(path, rep, order)
        line = open(path, "rb").read()
        assert line.decode() == ref.thr_info_line([{"down_k": d, "up_k": u} for d, u in ks], order)
        assert os.listdir(str(tmp_path)) == ["Thr_info.txt"]  # the temp file was renamed
        want = []
        for dk, uk in ks:
            want += [uk, dk] if order == "ai" else [dk, uk]
        want = [np.float32(k / 1024.0) for k in want]
        assert _sscanf6(line) == want                                     # what both encoders' fscanf("%f ...") reads
        assert [np.float32(float(t)) for t in line.decode().split(" ")] == want   # what net_CNN.get_thresholds' float() reads
        t1, t3 = pkg.ethcnn.parse_thresholds(path)                        # tokens [1] and [3]
        assert (np.float32(t1), np.float32(t3)) == (want[1], want[3])
        assert all(len(t.strip().split(".")[1]) == 10 for t in line.decode().split(" "))
