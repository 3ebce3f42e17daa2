"""GPU box (ONE MI355X visible): the launch contract of bench.py.

  * `python bench.py --gpus 2` on a 1-GPU box must exit non-zero with a clear message -- never a line whose n_gpus is not what ran;
  * the N > 1 control flow (self-launch through torch.distributed.run, barriers, max-over-ranks, sharded host scopes, rank-0 JSON
    with `roofline` + `cpu_baseline` under --full) is exercised by two ranks sharing GPU 0 over gloo through the command itself, not torchrun (test hooks
    BENCH_FORCE_DEVICE / BENCH_DIST_BACKEND; RCCL refuses two ranks on one device).  The numbers of that run mean nothing;
  * a plain run (no --full) prints the headline line only, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_more_gpus_than_visible_is_refused():
    import torch
    n = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1)], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert r.returncode != 0
    assert "only %d GPU(s) visible" % n in r.stderr
    assert not any(l.startswith("{") for l in r.stdout.splitlines())


def test_world_size_mismatch_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE (1) != --gpus (2)" in r.stderr


def test_two_ranks_through_the_plain_command():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c2", "--steps", "3", "--warmup", "1",
                        "--ramp-ms", "20", "--cpu-seconds", "2", "--full"], capture_output=True, text=True,
                       env=_env(BENCH_FORCE_DEVICE="0", BENCH_DIST_BACKEND="gloo"), timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"
    assert d["roofline"]["frac"] > 0 and d["roofline"]["bound"] == "mfma"
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1
    hs = d["host_scopes"]
    assert hs["ranks"] == 2 and hs["s2_host_to_host_ctus_per_s"] > 0 and hs["s3_file_to_file_ctus_per_s"] > 0
    # the two ranks shared the node's host budget
    import importlib
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    assert hs["fill_threads_per_rank"] == pkg.ethcnn.host_thread_budget(2)
    assert d["parity_first_frame_bit_exact"] is True


def test_box_calibration_is_a_plausible_mfma_rate(pkg):
    """ethcnn_measure_mfma_rate: pure exact-fp32 MFMAs for 20 ms -- between the rate every kernel of the path already reaches and
    the data-sheet peak (157.3 TFLOP/s); bad arguments are refused"""
    c = pkg.EthCnn(device=0)
    try:
        tf = c.measure_mfma_rate(0.02)
        assert 120.0 < tf < 160.0, tf
        with pytest.raises(Exception):
            c.measure_mfma_rate(0.0)
        with pytest.raises(Exception):
            c.measure_mfma_rate(60.0)
    finally:
        c.close()


def test_one_gpu_line_states_the_north_star_ratio_and_the_fast_plans():
    """The --full (N = 1) line on a short C2 run: contract keys, `roofline` + `cpu_baseline`, the north star's ratio
    (`vs_baseline` = S3 GPU / S3 oracle port, `vs_tf_cpu_proxy`, `north_star_10x`, each naming scope / cores / kind "port"),
    and the two opt-in plans reported BESIDE the exact headline (`fast_plan_fp16x2`, `fast_plan_fp16x2_trunk`) -- the headline
    itself stays dtype f32 and bit-exact."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", "4", "--warmup", "1", "--ramp-ms", "20",
                        "--cpu-seconds", "3", "--full"], capture_output=True, text=True, env=_env(), timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["dtype"] == "f32" and d["parity_first_frame_bit_exact"] is True
    assert d["vs_baseline"] is not None and d["vs_baseline"] > 1.0
    det = d["vs_baseline_detail"]
    assert det["kind"] == "port" and det["cores"] >= 1 and "S3" in det["scope"]
    assert d["vs_tf_cpu_proxy"] > 1.0 and d["vs_tf_cpu_proxy_detail"]["kind"] == "port"
    assert isinstance(d["north_star_10x"], bool)
    hs = d["host_scopes"]
    assert abs(d["vs_baseline"] - hs["s3_file_to_file_ctus_per_s"] / next(
        b["value"] for b in d["cpu_baselines"] if b["name"].startswith("B1 oracle") and "file scope" in b["name"])) < 1e-9
    assert "fast_plan" not in d  # (round 4's bf16 x 3 plan is gone)
    # roofline.traffic IS the FC1 rows of hbm.per_kernel_bytes (one stamped file, one workload, per kernel AND grid
    # size) -- or absent when the committed PMC passes were taken at other kernel sources; never an average over other configs' launches
    for obj in (d, d["fast_plan_fp16x2"], d["fast_plan_fp16x2_trunk"]):
        rl, hbm = obj["roofline"], obj["hbm"]
        if rl.get("traffic") is not None:
            fc1_rows = {k: v for k, v in hbm["per_kernel_bytes"].items() if k.startswith("k_fc1")}
            assert fc1_rows and rl["traffic"] == sum(fc1_rows.values()) == sum(rl["traffic_rows"].values()), (rl["traffic"], fc1_rows)
            assert all("@" in k for k in hbm["per_kernel_bytes"])          # every row names its grid size
            assert 1.0 <= rl["traffic_over_algorithmic"] < 3.0
        else:
            assert hbm["bytes_per_step"] is None                            # the same stamp rules both
    cs = hs["cold_start_ms"]   # the command's wall time on the reference's own C1 case, both launchers
    assert "error" not in cs and 30.0 < cs["native_tool"] < 5000.0 and 60.0 < cs["python_launcher"] < 10000.0, cs
    cl = d["ctu_load_stage"]["counter_bytes_per_ctu"]
    assert cl["fetched"] is None or (3500 < cl["fetched"] < 12000 and 6000 < cl["written"] < 8000), cl
    for key, dtype_word in (("fast_plan_fp16x2", "fp16x2"), ("fast_plan_fp16x2_trunk", "fp16x2")):
        fp = d[key]
        assert dtype_word in fp["dtype"] and fp["value"] > 0 and fp["roofline"]["peak"] == 2500.0
        assert fp["gate_pattern_equal"] is False or fp["max_abs_vs_exact"] <= 1e-4  # north star's tolerance
        assert fp["flips_vs_exact"] <= 2
    # every other single-GPU BASELINE config is driver-timed by the same run (short regions, parity-checked)
    oc = d["other_configs"]
    assert set(oc) == {"c3", "c4", "c5"}, oc.keys()
    for k in ("c3", "c4"):
        assert oc[k]["value"] > 1e6 and 0.5 < oc[k]["fc1_frac"] < 1.0 and oc[k]["parity_first_frame_bit_exact"] is True, oc[k]
    assert 10.0 < oc["c5"]["us_per_frame"] < 500.0 and oc["c5"]["parity_first_frames_bit_exact"] is True, oc["c5"]
    # side measurement: one picture host -> host (the path the in-process hook and every caller with the picture in its own memory takes)
    h2h = d["single_picture_latency"]["host_to_host"]
    for name in ("1920x1080", "3840x2160"):
        assert 20.0 < h2h[name]["page_locked"] < 2000.0 and 20.0 < h2h[name]["pageable"] < 4000.0, h2h


def _plain(tmp_path, tag, *args):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--ramp-ms", "20", "--dump-outputs", str(out)] + list(args),
                       capture_output=True, text=True, env=_env(), timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path, oracle):
    """No --full: the contract keys and nothing measured beside them; --steps sets the timed steps; the dumped probabilities
    are the whole last step (every CTU of the 50 frames), and its first frame is bit-exact vs the oracle"""
    d, out = _plain(tmp_path, "c2", "--workload", "c2", "--steps", "3", "--warmup", "1")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "config"):
        assert k in d, k
    assert d["steps"] == 3 and d["dtype"] == "f32" and d["higher_is_better"] is True and d["unit"] == "CTU/s"
    assert abs(d["value"] - d["config"]["ctus_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "host_scopes", "other_configs", "fast_plan_fp16x2", "stages_ms_per_step"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["probabilities.npy"]
    import numpy as np
    import bench
    got = np.load(out / "probabilities.npy")
    w, h = 1920, 1080
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    assert got.dtype == np.float32 and got.shape == (nctu * 50, 21)
    luma = bench.synth_luma(w, h, 1, seed=0xE7C00000 + 2)
    want = oracle.predict_frames(oracle.synth_blob(1, 8.0), luma, w, h, 1, 32, 0.5, 0.5, mode=0)
    assert np.array_equal(got[:nctu].view(np.uint32), want.view(np.uint32))


def test_dumped_ldp_step_repeats_run_to_run(tmp_path):
    """The LDP step (recurrent state in HBM) walks the same frames in every run: two runs with the same arguments dump the
    same probabilities and the same state"""
    import numpy as np
    runs = [_plain(tmp_path, "run%d" % i, "--workload", "c5", "--steps", "20", "--warmup", "5")[1] for i in range(2)]
    for name, shape in (("probabilities", (510, 21)), ("lstm_state", (510, 896))):
        a, b = (np.load(r / (name + ".npy")) for r in runs)
        assert a.shape == shape and a.dtype == np.float32
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
