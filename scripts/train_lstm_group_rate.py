"""Step rate of an ETH-LSTM trainer group (include/ethcnn.h "ETH-LSTM training, several models at once") against the same members
trained one after another, by the method of scripts/train_rate.py --net lstm: `--warmup` steps, then `--steps` device-drawn steps
enqueued back to back inside one synchronised host-clock window (no read-back inside it), the best of `--repeats` windows.

    python scripts/train_lstm_group_rate.py [--steps 2000] [--parent-root DIR] [--out profiles/train_lstm_group_rate.json]

Per batch size (64, 256): the solo LstmTrainer's us per step, then the group's us per group step at K = 1, 2, 4 and
ratio = group step / (K x solo step) -- below 1 the group beats its members in sequence.  At batch 64 also one 10000-sample one-batch
evaluation (drawn with replacement), solo and for a K = 4 group.  The samples carry four QPs; the solo trainer keeps QP 32, member m
of a group keeps QP (22, 27, 32, 37)[m % 4].  --parent-root: a checkout of the parent commit with its library built; its
scripts/train_rate.py --net lstm runs there three times (a process each) for the solo step time of the parent's library and its
run-to-run spread, against which any change of the solo path shows.
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
import train_data_lstm  # noqa: E402

KS = (1, 2, 4)
QPS = (22, 27, 32, 37)
NUM_EVAL = 10000


def window(obj, warmup, steps, repeats):
    """us per step: the best of `repeats` windows of `steps` steps"""
    obj.run(1, warmup)
    obj.last_stats()
    best, first = None, warmup + 1
    for _ in range(repeats):
        t0 = time.perf_counter()
        obj.run(first, steps)
        obj.last_stats()
        dt = time.perf_counter() - t0
        first += steps
        best = dt if best is None else min(best, dt)
    return best / steps * 1e6


def solo(pkg, ctx, batch, data):
    t = pkg.LstmTrainer(ctx, batch=batch, seed=1)
    t.set_qps([32])
    t.set_samples(0, data)
    t.init_weights(1)
    return t


def group(pkg, ctx, k, batch, data):
    g = pkg.LstmTrainerGroup(ctx, [pkg.ethcnn.lstm_train_options(batch=batch, seed=1 + m) for m in range(k)])
    for m in range(k):
        g.set_qps(m, [QPS[m % 4]])
    g.set_samples(0, data)
    g.init_weights(list(range(1, k + 1)))
    return g


def eval_ms(fn):
    fn()
    t0 = time.perf_counter()
    fn()
    return round((time.perf_counter() - t0) * 1e3, 2)


def parent_solo(root, batches, warmup, steps, runs=3):
    """us per solo step of the library under `root`, one process per run: {batch: [us, ...]}"""
    out = {str(b): [] for b in batches}
    for _ in range(runs):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "train_rate.py"), "--net", "lstm", "--batches",
                            ",".join(str(b) for b in batches), "--steps", str(steps), "--warmup", str(warmup), "--cpu-steps", "0"],
                           capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise SystemExit("parent run failed:\n" + r.stderr)
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for b in batches:
            out[str(b)].append(res["gpu"][str(b)]["us_per_step"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    res = {"net": "lstm", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "batch": {}}
    if a.parent_root:  # first, and in processes of their own: this process has not opened the GPU yet
        res["parent_solo_us_per_step"] = parent_solo(a.parent_root, batches, a.warmup, a.steps)
        print("parent solo:", res["parent_solo_us_per_step"], flush=True)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    data = train_data_lstm.make_samples(2500, seed=1)
    ctx = pkg.EthCnn(device=0)
    res["device"] = ctx.device_name
    for b in batches:
        row = res["batch"][str(b)] = {"group": {}}
        with solo(pkg, ctx, b, data) as t:
            base = window(t, a.warmup, a.steps, a.repeats)
            if b == 64:
                idx = np.random.default_rng(0).integers(0, t.num_samples(0), NUM_EVAL)
                row["solo_eval_10000_ms"] = eval_ms(lambda: t.evaluate(0, idx=idx))
        row["solo_us_per_step"] = round(base, 2)
        print("batch %4d solo: %9.1f us/step" % (b, base), flush=True)
        for k in KS:
            with group(pkg, ctx, k, b, data) as g:
                us = window(g, a.warmup, a.steps, a.repeats)
                if b == 64 and k == 4:
                    gidx = np.stack([np.random.default_rng(m).integers(0, g.num_samples(m, 0), NUM_EVAL) for m in range(k)])
                    row["group_4_eval_10000_ms"] = eval_ms(lambda: g.evaluate(0, idx=gidx))
            row["group"][str(k)] = {"us_per_group_step": round(us, 2), "ratio_to_k_solo_steps": round(us / (k * base), 3)}
            print("batch %4d K = %d: %9.1f us/group step, %.3f of K solo steps" % (b, k, us, us / (k * base)), flush=True)
    ctx.close()
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
