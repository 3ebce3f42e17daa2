#!/usr/bin/env python
"""What a policy per slot costs the pacer set, by the method of scripts/pacer_set_rate.py: a warm-up, then `steps` rounds in one
synchronised host-clock window, the forms ALTERNATED window by window inside one job so that they meet the same neighbours on the
machine, best of the windows.  Everything goes through the C ABI with argument arrays built once.

  lookup   the cost of the policy record: one ethcnn_pacer_set_frames_device call over N frames under the default ladder and ONE policy,
           through this tree's library (ethcnn_pacer_set_create, which is now a set of one policy) and through the library of the
           PARENT commit (--parent-lib, a libethcnn.so built from the commit before this feature), interleaved.  The margin is the
           parent's own noise: the max / min of its five windows.  `inside_band` says whether this tree's best lies within
           parent's best x that ratio.  A set of one policy takes the record from the kernel argument (the form the old entry runs);
           `table` is the other form of the kernel, which reads the record from the policy table in HBM, on the same frames: a set
           of two equal policies with every slot bound to the first.  Without --parent-lib this part is written as "not measured".
  mixed    N frames spread over four policies with ladders of 64, 256, 513 (the default) and 4096 rungs, so that one launch mixes
           segments of 1, 2, 3 and 17 rung blocks, against N solo pacers of the same policies (2 N launches).  Reported, no threshold.
           The baked words and the results of the two forms are compared.
N = 1, 4, 16 at 416x240 and at 1920x1080, budget 0.4, carry mode.
    python scripts/pacer_policies_rate.py [--parent-lib PATH] [--steps 500] [--windows 5] [--out profiles/pacer_policies_rate.json]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((416, 240), (1920, 1080))
COUNTS = (1, 4, 16)
SHARE, MODE = 0.4, "carry"
PARENT_ENTRIES = ("ethcnn_create", "ethcnn_destroy", "ethcnn_last_error", "ethcnn_synchronize", "ethcnn_pacer_set_create", "ethcnn_pacer_set_destroy",
                  "ethcnn_pacer_set_frames_device")


def stats(ts):
    return {"best": min(ts), "spread": max(ts) - min(ts), "max_over_min": max(ts) / min(ts), "windows": ts}


def window(sync, steps, fn):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e6 / steps


def alternate(forms, steps, windows):
    """forms: {name: (round function, its synchronise)} -> {name: [us per round of each window]}; the order inside a group of windows
    rotates, so that no form always runs first"""
    names = list(forms)
    ts = {k: [] for k in names}
    for k in range(windows):
        for name in names[k % len(names):] + names[:k % len(names)]:
            ts[name].append(window(forms[name][1], steps, forms[name][0]))
    return ts


class Parent(object):
    """the parent commit's library beside this tree's, with a context of its own; only the entries the measurement calls are typed"""

    def __init__(self, e, path):
        self.lib = ctypes.CDLL(path)
        for name in PARENT_ENTRIES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = e.SIGNATURES[name]
        self.h = ctypes.c_void_p()
        opt = e.Options(device=0, max_ctus_per_pass=0, host_threads=0)
        if self.lib.ethcnn_create(ctypes.byref(self.h), ctypes.byref(opt)):
            raise RuntimeError(self.lib.ethcnn_last_error(None).decode())

    def chk(self, rc):
        if rc:
            raise RuntimeError(self.lib.ethcnn_last_error(self.h).decode())

    def synchronize(self):
        self.chk(self.lib.ethcnn_synchronize(self.h))

    def pacer_set(self, nslots, ppm, mode):
        s = ctypes.c_void_p()
        self.chk(self.lib.ethcnn_pacer_set_create(self.h, nslots, None, 0, None, ppm, mode, ctypes.byref(s)))
        return s

    def close(self):
        self.lib.ethcnn_destroy(self.h)


def lookup(e, ctx, parent, steps, windows, res):
    lib = ctx.lib
    size = e.PACER_RESULT.itemsize
    for w, h in SIZES:
        nctu = e.ctus_per_frame(w, h)
        for n in COUNTS:
            rng = np.random.default_rng(1000 + n + w)
            probs = (rng.integers(0, 1025, size=(n, nctu, 21)) / 1024.0).astype(np.float32)
            d_in, d_new, d_old, d_tab, d_res = [ctx.alloc(probs.nbytes) for _ in range(4)] + [ctx.alloc(3 * n * size)]
            d_in.upload(probs)
            ctx.synchronize()
            at = lambda b, j: b.ptr + j * nctu * 84
            frames = lambda out, r0: (e.PacerSetFrame * n)(*[e.PacerSetFrame(j, at(d_in, j), w, h, at(out, j), d_res.ptr + (r0 + j) * size) for j in range(n)])
            pset = e.PacerSet(ctx, n, SHARE, MODE)
            old = parent.pacer_set(n, int(round(SHARE * 1e6)), e.BUDGET_CARRY)
            ptab = e.PacerSet(ctx, n, policies=[{"budget": SHARE, "mode": MODE}] * 2)
            arr_new, arr_old, arr_tab = frames(d_new, 0), frames(d_old, n), frames(d_tab, 2 * n)

            def new_round():
                if lib.ethcnn_pacer_set_frames_device(pset.h, arr_new, n):
                    raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            def old_round():
                parent.chk(parent.lib.ethcnn_pacer_set_frames_device(old, arr_old, n))

            def tab_round():
                if lib.ethcnn_pacer_set_frames_device(ptab.h, arr_tab, n):
                    raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            for _ in range(20):
                new_round()
                old_round()
                tab_round()
            ts = alternate({"parent": (old_round, parent.synchronize), "tree": (new_round, ctx.synchronize), "table": (tab_round, ctx.synchronize)}, steps, windows)
            ctx.synchronize()
            parent.synchronize()
            same = bool(np.array_equal(d_new.download(np.uint32, probs.size), d_old.download(np.uint32, probs.size)))
            same = same and bool(np.array_equal(d_tab.download(np.uint32, probs.size), d_old.download(np.uint32, probs.size)))
            records = d_res.download(np.uint8, 3 * n * size)
            same = same and records[:n * size].tobytes() == records[n * size:2 * n * size].tobytes() == records[2 * n * size:].tobytes()
            pset.close()
            ptab.close()
            parent.lib.ethcnn_pacer_set_destroy(old)
            for b in (d_in, d_new, d_old, d_tab, d_res):
                b.free()
            row = {"ctus_per_frame": nctu, "parent": {"us_per_call": stats(ts["parent"])}, "tree": {"us_per_call": stats(ts["tree"])},
                   "table": {"us_per_call": stats(ts["table"])}, "identical": same}
            row["table_over_parent"] = row["table"]["us_per_call"]["best"] / row["parent"]["us_per_call"]["best"]
            row["noise_band"] = row["parent"]["us_per_call"]["max_over_min"]
            row["tree_over_parent"] = row["tree"]["us_per_call"]["best"] / row["parent"]["us_per_call"]["best"]
            row["inside_band"] = bool(row["tree_over_parent"] <= row["noise_band"])
            res.setdefault("%dx%d" % (w, h), {})[str(n)] = row
    return all(r["identical"] for s in res.values() for r in s.values())


def mixed_policies(e):
    full = e.budget_default_ladder()
    j = np.arange(4096)
    deep = e.sim_thr(np.repeat((1024 - j // 4)[:, None], 3, axis=1), np.repeat((j // 4 - 1)[:, None], 3, axis=1))
    return [{"budget": SHARE, "mode": MODE, "ladder": lad, "weights": None} for lad in (full[0::8][:64].copy(), full[0::2][:256].copy(), None, deep)]


def mixed(e, ctx, steps, windows, res):
    lib = ctx.lib
    size = e.PACER_RESULT.itemsize
    policies = mixed_policies(e)
    for w, h in SIZES:
        nctu = e.ctus_per_frame(w, h)
        for n in COUNTS:
            rng = np.random.default_rng(2000 + n + w)
            probs = (rng.integers(0, 1025, size=(n, nctu, 21)) / 1024.0).astype(np.float32)
            d_in, d_set, d_solo, d_res = ctx.alloc(probs.nbytes), ctx.alloc(probs.nbytes), ctx.alloc(probs.nbytes), ctx.alloc(2 * n * size)
            d_in.upload(probs)
            at = lambda b, j: b.ptr + j * nctu * 84
            of = [(j + 2) % 4 for j in range(n)]   # (one frame alone stands under the default ladder)
            pset = e.PacerSet(ctx, n, policies=policies, slot_policy=of)
            solos = [e.Pacer(ctx, SHARE, MODE, ladder=policies[of[j]]["ladder"]) for j in range(n)]
            arr = (e.PacerSetFrame * n)(*[e.PacerSetFrame(j, at(d_in, j), w, h, at(d_set, j), d_res.ptr + j * size) for j in range(n)])
            solo_args = [(solos[j].h, at(d_in, j), w, h, at(d_solo, j), d_res.ptr + (n + j) * size) for j in range(n)]

            def set_round():
                if lib.ethcnn_pacer_set_frames_device(pset.h, arr, n):
                    raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            def solo_round():
                for a in solo_args:
                    if lib.ethcnn_pacer_frame_device(*a):
                        raise RuntimeError(lib.ethcnn_last_error(ctx.h).decode())

            for _ in range(20):
                set_round()
                solo_round()
            ts = alternate({"set": (set_round, ctx.synchronize), "solo": (solo_round, ctx.synchronize)}, steps, windows)
            ctx.synchronize()
            same = bool(np.array_equal(d_set.download(np.uint32, probs.size), d_solo.download(np.uint32, probs.size)))
            records = d_res.download(np.uint8, 2 * n * size)
            same = same and records[:n * size].tobytes() == records[n * size:].tobytes()
            launches = pset.launches
            blocks = e.pacer_set_plan([nctu] * n, [(64, 256, 513, 4096)[p] for p in of])["count_grid"]
            pset.close()
            for p in solos:
                p.close()
            for b in (d_in, d_set, d_solo, d_res):
                b.free()
            row = {"ctus_per_frame": nctu, "rungs_of_frame": [(65, 257, 514, 4097)[p] for p in of], "count_blocks": blocks,
                   "set": {"us_per_round": stats(ts["set"])}, "solo": {"us_per_round": stats(ts["solo"])}, "identical": same,
                   "set_launches_per_round": launches / float(20 + windows * steps)}
            row["solo_over_set"] = row["solo"]["us_per_round"]["best"] / row["set"]["us_per_round"]["best"]
            res.setdefault("%dx%d" % (w, h), {})[str(n)] = row
    return all(r["identical"] for s in res.values() for r in s.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libethcnn.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pacer_policies_rate.json"))
    a = ap.parse_args()
    e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    ctx = e.EthCnn(device=0)
    res = {"device": ctx.device_name, "steps": a.steps, "windows": a.windows, "budget": SHARE, "mode": MODE, "lookup": "not measured", "mixed": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    if a.parent_lib:
        parent = Parent(e, a.parent_lib)
        res["lookup"] = {}
        ok = lookup(e, ctx, parent, a.steps, a.windows, res["lookup"])
        parent.close()
        rows = [r for s in res["lookup"].values() for r in s.values()]
        res["lookup_summary"] = {"worst_tree_over_parent": max(r["tree_over_parent"] for r in rows), "widest_noise_band": max(r["noise_band"] for r in rows),
                                 "narrowest_noise_band": min(r["noise_band"] for r in rows), "worst_table_over_parent": max(r["table_over_parent"] for r in rows),
                                 "all_inside_band": all(r["inside_band"] for r in rows)}
        with open(a.out, "w") as f:   # (kept even if the second part fails)
            json.dump(res, f, indent=1)
    ok = mixed(e, ctx, a.steps, a.windows, res["mixed"]) and ok
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not ok:
        sys.stderr.write("pacer_policies_rate: two forms differ\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
