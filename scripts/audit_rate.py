"""Rate of the comparison of two predictions on one MI355X -> profiles/audit_rate.json.  A record, not a gate.

  gpu    EthCnn.compare_frames_device over the C4 job's geometry -- 4928x3264 (77 x 51 CTUs a frame), 425 frames = 1,668,975 CTUs -- with
         both sides (140 MB each) resident in HBM, with and without a candidate: after a warm-up call, one call per synchronised window
         (the call is synchronous: the launch, the 176-byte state back to the host), best of three.  168 bytes are read per CTU; the
         fraction of the HBM rate is that against the data-sheet 8 TB/s.  A call over one tile of 256 CTUs is timed the same way: what a
         call costs whatever its size.
  numpy  the restatement of the tests (tests/audit_ref.py: compare, in pieces of 25 frames that are combined by the split rule) over the
         same arrays on the same box, once per form; the results are compared for equality
  audit  one audit_plan (plan 3) of 5 frames of 3840x2160 beside the two predictions it contains (plan 0 and plan 3 through
         predict_luma_device, one synchronised window each), best of three

    python scripts/audit_rate.py [--out profiles/audit_rate.json] [--quick]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, FRAMES = 4928, 3264, 425
HBM_BYTES_PER_S = 8.0e12  # MI355X data sheet
PIECE = 25                # frames per piece of the numpy restatement


def best_of_three(ctx, fn):
    fn()  # warm-up: code object, first launch
    ctx.synchronize()
    times = []
    for _ in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_rate.json"))
    ap.add_argument("--quick", action="store_true", help="25 frames (a functional check, not a measurement)")
    a = ap.parse_args(argv)
    import audit_ref
    import calib_ref
    import sim_ref
    import bench
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    frames = 25 if a.quick else FRAMES
    nctu = ((W + 63) // 64) * ((H + 63) // 64)
    n = frames * nctu
    rng = np.random.default_rng(1)
    pa = calib_ref.edge_probs(rng, n)
    pb = audit_ref.perturbed(rng, pa, 0.01, 0.001, 1e-3)
    thr = sim_ref.thr((600, 700, 800), (400, 300, 200))
    tol = 1e-4
    res = {"width": W, "height": H, "frames": frames, "ctus": n, "bytes_read": 168 * n, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        da, db = ctx.alloc(pa.nbytes), ctx.alloc(pb.nbytes)
        da.upload(pa)
        db.upload(pb)
        got = {}
        for form, t in (("thr", thr), ("no_thr", None)):
            got[form], times = best_of_three(ctx, lambda: ctx.compare_frames_device(da, db, W, H, frames, tol, t))
            best = min(times)
            res["gpu_" + form] = dict(seconds=best, all_seconds=times, ctus_per_s=n / best, bytes_per_s=168 * n / best,
                                      fraction_of_hbm_rate=168 * n / best / HBM_BYTES_PER_S,
                                      window="one synchronous compare_frames_device call between two synchronisations, best of three")
        # what a call costs whatever its size: one tile (zeroing the state, the launch, the state back, the synchronisation)
        _, times = best_of_three(ctx, lambda: ctx.compare_probs_device(da, db, 256, tol, thr))
        res["gpu_one_tile_seconds"] = min(times)
        da.free()
        db.free()
        # the audit beside the two predictions it contains
        aw, ah, af, qp = 3840, 2160, 5, 32
        luma = bench.synth_luma(aw, ah, af, seed=4032)
        actus = af * ((aw + 63) // 64) * ((ah + 63) // 64)
        ctx.load_synthetic(11, 8.0)
        ctx.set_thresholds(-1.0, -1.0)
        dl, dp = ctx.alloc(luma.nbytes), ctx.alloc(actus * 84)
        dl.upload(luma)
        audit = {"width": aw, "height": ah, "frames": af, "ctus": actus, "plan": 3}
        for plan in (0, 3):
            ctx.set_fc1_plan(plan)
            _, times = best_of_three(ctx, lambda: ctx.predict_luma_device(dl, aw, ah, af, qp, dp))
            audit["predict_plan%d_seconds" % plan] = min(times)
        ctx.set_fc1_plan(0)
        r, times = best_of_three(ctx, lambda: ctx.audit_plan(dl, aw, ah, af, qp, 3, tol, thr))
        audit.update(audit_seconds=min(times), all_audit_seconds=times, fast_passes=r["fast_passes"], passes=r["passes"], max_abs=r["max_abs"],
                     over_tol=r["over_tol"], search_diff_ctus=r["search_diff_ctus"])
        res["audit"] = audit
        dl.free()
        dp.free()
    same = True
    for form, t in (("thr", thr), ("no_thr", None)):
        t0 = time.perf_counter()
        want = None
        for f0 in range(0, frames, PIECE):
            lo, hi = f0 * nctu, min(frames, f0 + PIECE) * nctu
            part = audit_ref.compare(pa[lo:hi], pb[lo:hi], tol, t, W, H)
            want = part if want is None else audit_ref.combine(want, part)
        dt = time.perf_counter() - t0
        res["numpy_" + form] = dict(seconds=dt, ctus_per_s=n / dt, runs=1)
        res["identical_" + form] = bool(audit_ref.stats_equal(got[form], want))
        res["stats_" + form] = {k: got[form][k] for k in audit_ref.FIELDS}
        same = same and res["identical_" + form]
    res["not_measured"] = ["the host entries (they add a pageable upload)", "arrays that are not 16-byte aligned (the dword loads)", "other GPUs of the pool"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the GPU comparison and the numpy restatement disagree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
