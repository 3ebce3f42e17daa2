"""Step rate of a trainer group (include/ethcnn.h "training, several models at once") against the same members trained one after
another, by the method of scripts/train_rate.py: `--warmup` steps, then `--steps` device-drawn steps enqueued back to back inside
one synchronised host-clock window (no read-back inside it).

    python scripts/train_group_rate.py [--steps 1000] [--parent-root DIR] [--out profiles/train_group_rate.json]

All-Intra net, per batch size (64, 256): the solo trainer's us per step, then the group's us per group step at K = 1, 2, 4, 8 and
ratio = group step / (K x solo step) -- below 1 the group beats its members in sequence.  --parent-root: a checkout of the parent
commit with its library built; its scripts/train_rate.py runs there three times (a process each) for the solo step time of the
parent's library and its run-to-run spread, against which any change of the solo path shows.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_data  # noqa: E402

KS = (1, 2, 4, 8)


def solo_rate(pkg, ctx, batch, data, warmup, steps):
    t = pkg.Trainer(ctx, batch=batch, seed=1)
    t.set_samples(0, data)
    t.set_qps([32])
    t.init_weights(1)
    t.run(1, warmup)
    t.last_stats()
    t0 = time.perf_counter()
    t.run(warmup + 1, steps)
    t.last_stats()
    dt = time.perf_counter() - t0
    t.close()
    return dt / steps * 1e6


def group_rate(pkg, ctx, k, batch, data, warmup, steps):
    g = pkg.TrainerGroup(ctx, [pkg.ethcnn.train_options(batch=batch, seed=1 + m) for m in range(k)])
    g.set_samples(0, data)
    for m in range(k):
        g.set_qps(m, [(22, 27, 32, 37)[m % 4]])
    g.init_weights(list(range(1, k + 1)))
    g.run(1, warmup)
    g.last_stats()
    t0 = time.perf_counter()
    g.run(warmup + 1, steps)
    g.last_stats()
    dt = time.perf_counter() - t0
    g.close()
    return dt / steps * 1e6


def parent_solo(root, batches, warmup, steps, runs=3):
    """us per solo step of the library under `root`, one process per run: {batch: [us, ...]}"""
    out = {str(b): [] for b in batches}
    for _ in range(runs):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "train_rate.py"), "--batches", ",".join(str(b) for b in batches),
                            "--steps", str(steps), "--warmup", str(warmup), "--cpu-steps", "0"], capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise SystemExit("parent run failed:\n" + r.stderr)
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for b in batches:
            out[str(b)].append(res["gpu"][str(b)]["us_per_step"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    res = {"steps": a.steps, "warmup": a.warmup, "batch": {}}
    if a.parent_root:  # first, and in processes of their own: this process has not opened the GPU yet
        res["parent_solo_us_per_step"] = parent_solo(a.parent_root, batches, a.warmup, a.steps)
        print("parent solo:", res["parent_solo_us_per_step"], flush=True)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    data = train_data.make_records(4096, seed=1)
    ctx = pkg.EthCnn(device=0)
    res["device"] = ctx.device_name
    for b in batches:
        solo = [solo_rate(pkg, ctx, b, data, a.warmup, a.steps) for _ in range(3)]
        row = res["batch"][str(b)] = {"solo_us_per_step": [round(x, 2) for x in solo], "group": {}}
        base = sorted(solo)[1]
        print("batch %4d solo: %s us/step" % (b, row["solo_us_per_step"]), flush=True)
        for k in KS:
            us = group_rate(pkg, ctx, k, b, data, a.warmup, a.steps)
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
