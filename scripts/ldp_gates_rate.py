#!/usr/bin/env python
"""What the per-row gate thresholds cost: time of ONE step of N live Low-Delay-P encoders of one picture size (frames and outputs in
HBM, LdpSessions.step_device), three ways:
  parent   the library of the commit before the per-row table (one threshold pair per gate launch, 512 bytes of kernel arguments).
           Built from a `git worktree` of that commit into a scratch directory; its process imports that tree's own binding
  inherit  this library, every session inheriting the context's pair
  own      this library, every session with a pair of its own (the context's values, so that all three forms give the same words)
Each form runs in a child process of its own, the way scripts/ldp_sessions_rate.py runs lib_exp in a child, so that the three are
timed under the same conditions; this process only tells them when.  The method of scripts/ldp_sessions_rate.py -- a warm-up, then 50
steps in one synchronised host-clock window, best of three windows with the spread -- but the three forms ALTERNATE window by window,
and the round starts with another form each time (parent inherit own, inherit own parent, own parent inherit).  A child stays alive
for a job and times one window when it is told to; while one form runs the two others wait.  N = 1, 4, 16 at 416x240 and at
1920x1080.  No ratio is fixed in advance: read a difference only where it exceeds the spreads of its job.
    python scripts/ldp_gates_rate.py [--steps 50] [--base HEAD^] [--parent bench_out/ldp_gates_parent] [--out profiles/ldp_gates_rate.json]
--base: the commit the parent form is built from when --parent does not hold a built tree yet (needs git; a tree that was built
before, on another machine for instance, is used as it is)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hevc-complexity-reduction_amd"
SIZES = ((416, 240), (1920, 1080))
COUNTS = (1, 4, 16)
QP = 32
THR = (0.5, 0.5)
WINDOWS = 3


def stats(ts):
    return {"best": min(ts), "spread": max(ts) - min(ts), "windows": ts}


def pictures(w, h, n):
    return np.random.default_rng(100 + n).integers(0, 256, size=(n, h, w), dtype=np.uint8)


class Job(object):
    """N sessions of w x h on a context, warmed up; window() times `steps` steps, end() gives the words of frame 1 from zeros"""

    def __init__(self, e, ctx, w, h, n, own):
        self.e, self.ctx, self.n = e, ctx, n
        nctu = self.nctu = e.ctus_per_frame(w, h)
        lum = pictures(w, h, n)
        self.d_l, self.d_p = ctx.alloc(lum.size), ctx.alloc(n * nctu * 21 * 4)
        self.d_l.upload(lum.reshape(-1))
        self.s = e.LdpSessions(ctx, 1)
        self.s.load_lstm_synthetic(0, 22, 3.0)
        ids = [self.s.open(w, h) for _ in range(n)]
        if own:
            for i in ids:
                self.s.set_thresholds(i, *THR)
        self.frames = lambda i: [{"session": ids[j], "d_luma": self.d_l.ptr + j * w * h, "qp": QP, "i_frame": i, "bundle": 0,
                                  "d_probs": self.d_p.ptr + j * nctu * 84} for j in range(n)]
        self.s.step_device(self.frames(1))  # warm-up: allocations, first launches
        self.s.step_device(self.frames(2))
        ctx.synchronize()

    def window(self, steps):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            self.s.step_device(self.frames(2 + k))
        self.ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    def end(self):
        self.s.step_device(self.frames(1))
        self.ctx.synchronize()
        words = self.d_p.download(np.uint32, self.n * self.nctu * 21)
        self.s.close()
        self.d_l.free()
        self.d_p.free()
        return words


def make_ctx(e):
    ctx = e.EthCnn(device=0)
    ctx.load_synthetic(21, 1.0)
    ctx.set_thresholds(*THR)
    return ctx


def child(steps):
    """one form: serves `job W H N`, `window`, `end` lines on stdin, one answer line each"""
    sys.path.insert(0, os.environ["ETHCNN_GATES_TREE"])
    form = os.environ["ETHCNN_GATES_FORM"]
    e = importlib.import_module(PKG + ".ethcnn")
    assert hasattr(e.LdpSessions, "set_thresholds") == (form != "parent"), "the parent tree already has the per-row table"
    ctx = make_ctx(e)
    job = None
    print("ready %s" % ctx.device_name, flush=True)
    for line in sys.stdin:
        words = line.split()
        if words[0] == "job":
            job = Job(e, ctx, int(words[1]), int(words[2]), int(words[3]), form == "own")
            print("ok", flush=True)
        elif words[0] == "window":
            print(repr(job.window(steps)), flush=True)
        elif words[0] == "end":
            w = job.end()
            print(json.dumps([int(x) for x in w]), flush=True)
    ctx.close()
    return 0


def build_parent(parent, base):
    lib = os.path.join(parent, PKG, "lib", "libethcnn.so")
    if os.path.exists(lib):
        return
    if not os.path.isdir(os.path.join(parent, PKG, "csrc")):
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", os.path.abspath(parent), base])
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-s", "-j16", "-C", os.path.join(parent, PKG, "csrc"), "../lib/libethcnn.so"], env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--base", default="HEAD^")
    ap.add_argument("--parent", default=os.path.join(ROOT, "bench_out", "ldp_gates_parent"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldp_gates_rate.json"))
    ap.add_argument("--build-only", action="store_true", help="build the parent form's tree and stop")
    ap.add_argument("--child", action="store_true", help="internal: one form, told which by its environment")
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    build_parent(a.parent, a.base)
    if a.build_only:
        return 0
    forms = ["parent", "inherit", "own"]
    procs = {}

    def ask(name, line=None):
        proc = procs[name]
        if line is not None:
            proc.stdin.write(line + "\n")
            proc.stdin.flush()
        got = proc.stdout.readline()
        if not got:
            raise RuntimeError("ldp_gates_rate: the process of form %s ended (status %r)" % (name, proc.poll()))
        return got.strip()

    ok = True
    try:
        for name in forms:
            tree = os.path.abspath(a.parent) if name == "parent" else ROOT
            env = dict(os.environ, ETHCNN_GATES_TREE=tree, ETHCNN_GATES_FORM=name)
            env.pop("ETHCNN_LIB", None)
            procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)], env=env, stdin=subprocess.PIPE,
                                           stdout=subprocess.PIPE, text=True, cwd=tree)
        devices = [ask(name).split(" ", 1) for name in forms]  # (this process opens no GPU itself)
        assert all(d[0] == "ready" for d in devices), devices
        res = {"device": devices[0][1], "steps": a.steps, "qp": QP, "windows": WINDOWS,
               "order": [forms[r:] + forms[:r] for r in range(WINDOWS)], "sizes": {}}
        for w, h in SIZES:
            for n in COUNTS:
                for name in forms:
                    assert ask(name, "job %d %d %d" % (w, h, n)) == "ok"
                ts = {name: [] for name in forms}
                for r in range(WINDOWS):
                    for name in forms[r % 3:] + forms[:r % 3]:
                        ts[name].append(float(ask(name, "window")))
                words = {name: np.array(json.loads(ask(name, "end")), dtype=np.uint32) for name in forms}
                row = {name: {"us_per_step": stats(ts[name]), "crc": int(words[name].astype(np.uint64).sum())} for name in ts}
                row["identical"] = {name: bool(np.array_equal(words[name], words["parent"])) for name in ("inherit", "own")}
                best = {name: row[name]["us_per_step"]["best"] for name in ts}
                row["ratio_to_parent"] = {name: best[name] / best["parent"] for name in ("inherit", "own")}
                row["largest_spread"] = max(row[name]["us_per_step"]["spread"] for name in ts)
                row["beyond_the_spreads"] = {name: bool(abs(best[name] - best["parent"]) > row["largest_spread"]) for name in ("inherit", "own")}
                ok = ok and all(row["identical"].values())
                res["sizes"].setdefault("%dx%d" % (w, h), {})[str(n)] = row
    finally:
        for proc in procs.values():
            proc.stdin.close()
        for proc in procs.values():
            proc.wait(timeout=60)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not ok:
        sys.stderr.write("ldp_gates_rate: the forms differ\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
