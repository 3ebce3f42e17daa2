"""Training-step rate of the GPU trainer (include/ethcnn.h "training") and the float64 torch-CPU restatement as a baseline.

    python scripts/train_rate.py [--steps 2000] [--cpu-steps 5] [--out profiles/train_rate.json]
    python scripts/train_rate.py --net ldp --tune 0,1 [--cpu-steps 0] [--out profiles/train_rate_ldp.json]

Per batch size: `--warmup` steps, then `--steps` device-drawn steps enqueued back to back inside one synchronised host-clock window
(no read-back inside it) -> us per step and samples/s.  The CPU baseline runs tests/train_ref.py (float64 autograd, torch's own CPU
kernels) on the same batch size; its thread count is torch's default unless --cpu-threads is given.  Data: seeded synthetic records.
--net ldp: the Low-Delay-P residual net on 16516-byte records (every step over the four slots); --tune: PARTLY_TUNING_MODE values,
one timing row set each (1..3 skip the trunk backward: 7 launches).
--net lstm: the ETH-LSTM trainer (LstmTrainer, 10 launches a step, csrc/ethcnn_lstm_train.h) on synthetic 37264-byte samples; the CPU
baseline is tests/train_ref_lstm.py at batch 64; also one 10000-sample one-batch evaluation, which the reference's schedule runs
twice every 1000 steps.

    python scripts/train_rate.py --net lstm [--steps 500] [--out profiles/train_rate_lstm.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_data  # noqa: E402
import train_data_ldp  # noqa: E402

LAUNCHES_PER_STEP = 8  # csrc/ethcnn_train.h
FC1_FLOP_PER_SAMPLE = 2 * 2688 * 448 * 3  # forward + the two backward GEMMs of FC1


def gpu_rate(pkg, ctx, batch, data, warmup, steps, net="ai", tune=0):
    t = pkg.Trainer(ctx, batch=batch, seed=1, net=net, tune=tune)
    t.set_samples(0, data)
    if net == "ai":
        t.set_qps([32])  # LDP: the four slot QPs
    t.init_weights(1)
    t.run(1, warmup)
    t.last_stats()
    t0 = time.perf_counter()
    t.run(warmup + 1, steps)
    t.last_stats()
    dt = time.perf_counter() - t0
    t.close()
    return dt / steps * 1e6


def cpu_rate(batch, data, steps, threads):
    import torch
    import train_ref
    if threads:
        torch.set_num_threads(threads)
    blob = np.random.default_rng(0).standard_normal(1288210) * 0.05
    idx = np.arange(batch) % (len(data) // 4992)
    luma, lab = train_ref.parse_records(data, idx, 32)
    train_ref.loss_and_grad(blob, luma, lab, 32)
    t0 = time.perf_counter()
    for _ in range(steps):
        train_ref.loss_and_grad(blob, luma, lab, 32)
    return (time.perf_counter() - t0) / steps * 1e6, torch.get_num_threads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--net", choices=("ai", "ldp", "lstm"), default="ai")
    ap.add_argument("--tune", default="0", help="comma-separated tuning modes (each a row set)")
    a = ap.parse_args()
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    if a.net == "ldp":
        return main_ldp(a, pkg)
    if a.net == "lstm":
        return main_lstm(a, pkg)
    data = train_data.make_records(4096, seed=1)
    ctx = pkg.EthCnn(device=0)
    res = {"launches_per_step": LAUNCHES_PER_STEP, "device": ctx.device_name, "gpu": {}}
    for b in [int(x) for x in a.batches.split(",")]:
        us = gpu_rate(pkg, ctx, b, data, a.warmup, a.steps)
        res["gpu"][str(b)] = {"us_per_step": round(us, 2), "samples_per_s": round(b / us * 1e6),
                              "fc1_tflops": round(FC1_FLOP_PER_SAMPLE * b / us * 1e-6, 3)}
        print("batch %5d: %9.1f us/step  %10.0f samples/s" % (b, us, b / us * 1e6), flush=True)
    ctx.close()
    us64 = res["gpu"].get("64", {}).get("us_per_step")
    if us64:
        res["projected_1M_iterations_h"] = round(us64 * 1e6 / 3.6e9, 3)  # the reference's schedule: 1 M steps at batch 64
    if a.cpu_steps:
        cus, thr = cpu_rate(64, data, a.cpu_steps, a.cpu_threads)
        res["cpu_torch_float64"] = {"batch": 64, "us_per_step": round(cus), "threads": thr}
        print("cpu torch float64 batch 64: %.0f us/step (%d threads)" % (cus, thr))
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main_ldp(a, pkg):
    data = train_data_ldp.make_records(4096, seed=1)
    ctx = pkg.EthCnn(device=0)
    res = {"net": "ldp", "device": ctx.device_name, "gpu": {}}
    for tune in [int(x) for x in a.tune.split(",")]:
        rows = res["gpu"]["tune%d" % tune] = {"launches_per_step": LAUNCHES_PER_STEP - (1 if tune else 0)}
        for b in [int(x) for x in a.batches.split(",")]:
            us = gpu_rate(pkg, ctx, b, data, a.warmup, a.steps, "ldp", tune)
            rows[str(b)] = {"us_per_step": round(us, 2), "samples_per_s": round(b / us * 1e6)}
            print("ldp tune %d batch %5d: %9.1f us/step  %10.0f samples/s" % (tune, b, us, b / us * 1e6), flush=True)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


LSTM_LAUNCHES_PER_STEP = 10  # csrc/ethcnn_lstm_train.h


def main_lstm(a, pkg):
    import train_data_lstm
    data = train_data_lstm.make_samples(2500, seed=1, qps=(32,))
    ctx = pkg.EthCnn(device=0)
    res = {"net": "lstm", "launches_per_step": LSTM_LAUNCHES_PER_STEP, "device": ctx.device_name, "gpu": {}}
    for b in [int(x) for x in a.batches.split(",")]:
        t = pkg.LstmTrainer(ctx, batch=b, seed=1)
        t.set_samples(0, data)
        t.init_weights(1)
        t.run(1, a.warmup)
        t.last_stats()
        t0 = time.perf_counter()
        t.run(a.warmup + 1, a.steps)
        t.last_stats()
        us = (time.perf_counter() - t0) / a.steps * 1e6
        res["gpu"][str(b)] = {"us_per_step": round(us, 2), "samples_per_s": round(b / us * 1e6)}
        print("lstm batch %5d: %9.1f us/step  %10.0f samples/s" % (b, us, b / us * 1e6), flush=True)
        if b == 64:  # NUM_TRAIN_PART = 10000 samples as ONE batch (drawn with replacement from the 2500)
            idx = np.random.default_rng(0).integers(0, 2500, 10000)
            t.evaluate(0, idx=idx)
            t0 = time.perf_counter()
            t.evaluate(0, idx=idx)
            res["eval_10000_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t.close()
    ctx.close()
    us64 = res["gpu"].get("64", {}).get("us_per_step")
    if us64:  # the reference's schedule: 200000 steps at batch 64 + 2 x 200 evaluations of 10000 samples
        res["projected_200000_iterations_min"] = round((us64 * 200000 * 1e-6 + res.get("eval_10000_ms", 0) * 400 * 1e-3) / 60, 2)
    if a.cpu_steps:
        import torch
        import train_ref_lstm as R
        if a.cpu_threads:
            torch.set_num_threads(a.cpu_threads)
        blob = (np.random.default_rng(0).standard_normal(R.FLOATS) * 0.05)
        vec, lab, qps, gop = R.parse_samples(data, np.arange(64))
        R.loss_and_grad(blob, vec, lab, qps, gop)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            R.loss_and_grad(blob, vec, lab, qps, gop)
        cus = (time.perf_counter() - t0) / a.cpu_steps * 1e6
        res["cpu_torch_float64"] = {"batch": 64, "us_per_step": round(cus), "threads": torch.get_num_threads()}
        print("cpu torch float64 batch 64: %.0f us/step (%d threads)" % (cus, torch.get_num_threads()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
