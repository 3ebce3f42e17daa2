#!/usr/bin/env python
"""bench.py -- CTUs/sec of ETH-CNN inference (BASELINE.json metric) on N MI355X GPUs.

A "step" = one pass of the whole hot path (k0 tile -> k1 trunk -> FC1 -> FC2 -> head ->
gates) over one batch of synthetic luma frames ALREADY RESIDENT IN HBM, producing the
cu_depth.dat payload in HBM.  Default workload = BASELINE.json configs[2] at QP32
("All-Intra 3840x2160 QP32, 50 frames": the largest single-GPU configuration and the one
north_star sets its target on); --workload picks another config (c2 = configs[1], ...).
N > 1: frames shard across ranks with no data-path collective (weak scaling: every rank
runs the same per-GPU workload on its own frames); torch.distributed is used only for the
timing barrier and the max-over-ranks reduction.  `python bench.py --gpus N` launches its own
N ranks (one per GPU, torch.distributed.run on 127.0.0.1) when it is not already running under
torchrun, and REFUSES (non-zero exit) when fewer than N GPUs are visible: the printed `n_gpus`
is always the number of GPUs that were measured.  With --full, N > 1 lines carry the same `roofline`
and `cpu_baseline` objects plus the SHARDED host scopes (all ranks reading one 4:2:0 file / their own
host memory at the same time: where host DRAM and PCIe contention decide).

Prints ONE JSON line on rank 0: the headline (`metric`, `value`, `unit`, `ms_per_step`, `dtype` ...)
and `config`.  A plain run does only that: set-up, warm-up, the --steps timed steps, the line.
--dump-outputs DIR also writes what the last timed step computed as DIR/<name>.npy.  --full adds
every side measurement and check (stage breakdown, opt-in plans, host scopes, other configs,
latency, parity vs the oracle) and, among others, these two objects:
  roofline      dominant kernel = FC1 (77.6 % of the MACs): algorithmic FLOP / HIP-event
                kernel time vs the fp32-MFMA peak of MI355X_MICROARCH.md (157.3 TFLOP/s)
  cpu_baseline  the CPU oracle (a port of the reference's TF-CPU path; TensorFlow itself
                cannot run here) timed on all host cores on a bounded sample; `cpu_baselines`
                lists it again beside the same oracle on 1 thread, the oracle at the reference's
                own timed scope (file -> cu_depth.dat) and the structure-faithful TF-CPU proxy
                (oracle/tf_cpu_proxy.py: per-CTU Python tiling loop, 1024-CTU feeds, torch-CPU ops)
"""
import argparse
import importlib
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {  # BASELINE.json configs
    "c1": dict(width=768, height=512, frames=1, qp=32, name="All-Intra 768x512 QP32, 1 frame"),
    "c2": dict(width=1920, height=1080, frames=50, qp=32, name="All-Intra 1920x1080 QP32, 50 frames synthetic YUV"),
    "c3": dict(width=3840, height=2160, frames=50, qp=32, name="All-Intra 3840x2160 QP32, 50 frames synthetic YUV"),
    "c4": dict(width=4928, height=3264, frames=54, qp=27, name="All-Intra 4928x3264 QP27, 54 frames (one GPU's 1/8 share of 425)"),
    # config #5 (LDP): one frame per call, lock-step with the encoder -> a step is ONE frame through
    # resi_cnn + one ETH-LSTM step + heads + gates with the recurrent state resident in HBM
    "c5": dict(width=1920, height=1080, frames=8, qp=32, ldp=True,
               name="Low-Delay-P 1920x1080 QP32, one residual frame per step (ETH-CNN + ETH-LSTM one step)"),
}
MAC_PER_CTU = 1552149          # conv 279,552 + FC1 1,204,224 + FC2 64,848 + FC3 3,525
FC1_FLOP_PER_CTU = 2 * 1204224
ALG_BYTES_PER_CTU = 4096 + 84  # u8 luma in + 21 fp32 out
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2_f32
PEAK_HBM_GBPS = 8000.0
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (the 5 PF headline includes 2:1 sparsity)


def synth_luma(width, height, frames, seed):
    """Seeded synthetic 8-bit luma: 256x256 macro-tiles cycling smooth gradient / blurred
    noise / flat blocks / full-range noise, so CTUs span easy -> hard."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = np.empty((frames, height, width), dtype=np.uint8)
    yy, xx = np.ogrid[0:height, 0:width]
    kind = ((yy // 256) + (xx // 256)) % 4
    is_grad, is_blur, is_flat = kind == 0, kind == 1, kind == 2
    grad = (((yy * 3 + xx * 2) // 8) % 256).astype(np.uint8)
    flat = (((yy // 16) * 31 + (xx // 16) * 17) % 200 + 20).astype(np.uint8)
    for f in range(frames):
        noise = rng.integers(0, 256, size=(height, width), dtype=np.uint8)
        blur = noise.astype(np.uint16)
        blur = (blur + np.roll(blur, 1, 0) + np.roll(blur, 1, 1) + np.roll(np.roll(blur, 1, 0), 1, 1)) // 4
        # the four macro-tile kinds written in place, in 8 bits (uint8 addition wraps: (grad + f) % 256)
        frame = out[f]
        frame[...] = noise
        np.copyto(frame, flat, where=is_flat)
        np.copyto(frame, blur, where=is_blur, casting="unsafe")
        np.add(grad, np.uint8(f % 256), out=frame, where=is_grad)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ramp-ms", type=float, default=250.0, help="untimed load before the warm-up steps (GPU clock ramp)")
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=24.0, help="target CPU time of ALL baseline samples together")
    ap.add_argument("--no-host-scopes", action="store_true", help="skip the PCIe / file-inclusive side measurements")
    ap.add_argument("--no-fast-plan", action="store_true", help="skip the further timed regions (opt-in FC1 / trunk plans on the 16-bit matrix pipe), reported as `fast_plan*`")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short driver-timed regions of the other BASELINE configs (`other_configs`)")
    ap.add_argument("--fast-plans", default="2,3", help="which opt-in plans get a timed region (profiling runs: --fast-plans 3)")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and check (stage breakdown, roofline, box calibration, opt-in plans, host scopes, "
                         "CPU baselines, other configs, latency, parity vs the oracle); the --no-* options above prune it.  Without it "
                         "the run is set-up, warm-up, the timed steps and the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32; rank 0's frames when --gpus > 1)")
    args = ap.parse_args()

    import numpy as np
    import torch  # first: both torch and libethcnn bind libamdhip64.so.7 -> one HIP runtime in the process
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (libethcnn has no CPU fallback)")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return self_launch(args.gpus, torch.cuda.device_count())
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:  # never print an n_gpus that is not what ran
        raise SystemExit("bench.py: WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus))
    # test hooks for exercising the multi-rank control flow on a ONE-GPU box (scripts/gpu_dist_smoke.sh):
    # BENCH_FORCE_DEVICE puts every rank on that device, BENCH_DIST_BACKEND=gloo replaces RCCL (which
    # refuses two ranks on one GPU).  Never set by the driver.
    if os.environ.get("BENCH_FORCE_DEVICE") is not None:
        local_rank = int(os.environ["BENCH_FORCE_DEVICE"])
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d has no GPU (%d visible): one rank per GPU" % (local_rank, torch.cuda.device_count()))
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)

    def barrier():
        if dist is not None:
            if backend == "nccl":
                dist.barrier(device_ids=[local_rank])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    wl = WORKLOADS[args.workload]
    W, H, NF, QP = wl["width"], wl["height"], wl["frames"], wl["qp"]
    nctu = pkg.ethcnn.ctus_per_frame(W, H)
    ctus_per_step = nctu * NF

    ctx = pkg.EthCnn(device=local_rank)
    numa = pin_to_gpu_numa_node(ctx.device_name)  # before any input buffer is first touched
    ctx.load_synthetic(seed=1, head_gain=8.0)
    ctx.set_thresholds(0.5, 0.5)  # shipped Thr_info.txt
    luma = synth_luma(W, H, NF, seed=0xE7C00000 + 2 + 1000 * rank)
    d_in = ctx.alloc(luma.nbytes)
    d_out = ctx.alloc(ctus_per_step * 21 * 4)
    d_in.upload(luma)

    ldp = bool(wl.get("ldp"))
    if ldp:
        ctus_per_step = nctu
        ctx.load_lstm_synthetic(seed=2, head_gain=3.0)
        d_vec = ctx.alloc(nctu * 448 * 4)
        d_state = [ctx.alloc(nctu * 896 * 4), ctx.alloc(nctu * 896 * 4)]
        ldp_frame = [0]

    def step():
        if not ldp:
            ctx.predict_luma_device(d_in, W, H, NF, QP, d_out)
            return
        i = ldp_frame[0]
        ldp_frame[0] = i + 1
        ctx._chk(ctx.lib.ethcnn_resi_vectors_device(ctx.h, d_in.ptr + (i % NF) * W * H, W, H, W, d_vec.ptr))
        ctx._chk(ctx.lib.ethcnn_lstm_step_device(ctx.h, d_vec.ptr, d_state[i & 1].ptr if i > 0 else None, nctu, QP,
                                                 i + 1, d_state[(i + 1) & 1].ptr, d_out.ptr))

    # clock ramp: the GPU reaches its sustained clocks only after ~100 ms of load (measured: a 20-step timed
    # region right after 5 warm-up steps runs 6 % slower than the same region after 40); bring it there
    # first, untimed, then do the W warm-up steps the contract asks for
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < args.ramp_ms * 1e-3:
        for _ in range(8):
            step()
        ctx.synchronize()
    if ldp:
        ldp_frame[0] = 0  # the warm-up and timed steps walk the same frames and recurrent states in every run
    for _ in range(args.warmup):
        step()
    ctx.synchronize()
    ctx.set_profiling(1)  # HIP events around the dominant kernel (FC1) on every 3rd pass, on the library's stream
    ctx.reset_stage_times()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.synchronize()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    st = ctx.stage_times()
    ctx.set_profiling(0)
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the gated probabilities of every CTU of the step
        # (21 per CTU; c4, the largest, is 17.8 MB) and, for the LDP step, the recurrent state it hands to the next frame
        dump = {"probabilities": d_out.download(np.float32, ctus_per_step * 21).reshape(ctus_per_step, 21)}
        if ldp:
            dump["lstm_state"] = d_state[ldp_frame[0] & 1].download(np.float32, nctu * 896).reshape(nctu, 896)
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)
    if args.full:
        # per-stage breakdown: a short extra run OUTSIDE the timed region (an event pair per launch costs stream time, so it
        # is kept out of `value`), with the pass pipeline OFF: with it on the CTU-load stage of step i+1 runs beside FC1 of step i
        # (throttled to one block per CU on purpose) and the stage intervals overlap
        ctx.set_pass_pipeline(False)
        ctx.set_profiling(2)
        ctx.reset_stage_times()
        for _ in range(3):
            step()
        st_all = ctx.stage_times()
        ctx.set_profiling(0)
        ctx.set_pass_pipeline(True)  # (the library's default; it reads no environment switch for it -- ADVICE r04)
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # collective side measurements (every rank takes part; never `value`): the sharded host scopes at N > 1
    sharded = None
    if args.full and dist is not None and not ldp and not args.no_host_scopes:
        sharded = host_scopes_sharded(ctx, luma, W, H, NF, QP, rank, world, dist, backend, barrier)

    # FC1 plans 1 / 2 ("fast": split operands on the 16-bit matrix pipe, ethcnn_set_fc1_plan) -- further timed regions of the same K
    # steps under the same barriers, reported beside the headline as `fast_plan` (bf16 x 3) and `fast_plan_fp16x2`, never as
    # `value`: their results agree with the exact plan to ~1e-6 but are not bit-identical to the oracle
    fast = {}
    if args.full and not ldp and not args.no_fast_plan:
        exact_out = d_out.download(np.float32, ctus_per_step * 21).reshape(-1, 21) if rank == 0 else None
        for plan in [int(p) for p in args.fast_plans.split(",") if p]:
            ctx.set_profiling(0)
            ctx.set_fc1_plan(plan)
            t_ramp = time.perf_counter()
            while time.perf_counter() - t_ramp < 0.1:  # the clock settles at this plan's level (power management, ~ms)
                for _ in range(8):
                    step()
                ctx.synchronize()
            for _ in range(args.warmup):
                step()
            ctx.synchronize()
            ctx.set_profiling(1)
            ctx.reset_stage_times()
            barrier()
            tf0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            ctx.synchronize()
            barrier()
            f_elapsed = time.perf_counter() - tf0
            f_st = ctx.stage_times()
            ctx.set_pass_pipeline(False)
            ctx.set_profiling(2)
            ctx.reset_stage_times()
            for _ in range(3):
                step()
            f_all = ctx.stage_times()
            ctx.set_profiling(0)
            ctx.set_pass_pipeline(True)  # (the library's default; it reads no environment switch for it -- ADVICE r04)
            if dist is not None:
                tt = torch.tensor([f_elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                f_elapsed = float(tt.item())
            if rank == 0:
                fast_out = d_out.download(np.float32, ctus_per_step * 21).reshape(-1, 21)
                f_ms = f_st["ms"]["fc1"] / max(1, f_st["timed"]["fc1"])
                f_alg = FC1_FLOP_PER_CTU * f_st["timed_ctus"]["fc1"] / (f_st["ms"]["fc1"] * 1e-3) / 1e12 if f_st["ms"]["fc1"] > 0 else 0.0
                same_zero = bool(np.array_equal(fast_out == 0.0, exact_out == 0.0))
                nprod = 3
                fc1_plan = 2
                fast[plan] = {
                    "value": ctus_per_step * args.steps * world / f_elapsed, "unit": "CTU/s", "ms_per_step": f_elapsed / args.steps * 1e3,
                    "dtype": "fp16x2 split (power-of-two scaled), f32 accumulate" +
                             (" (FC1 only; trunk, heads and gates exact f32 as in `value`)" if plan < 3 else
                              " (trunk convolutions, FC1 and the heads' FC2 / FC3; CTU-load stage folded into the trunk; gates exact as in `value`)"),
                    "plan": "ethcnn_set_fc1_plan(ctx, %d): " % plan +
                            "every scaled fp32 feature / weight as two fp16 pieces (2^-24 relative), three products on "
                            "v_mfma_f32_32x32x16_f16; opt-in, never the default",
                    "roofline": {"kernel": "k_fc1_fast<%d, 7, nine> (ethcnn_fc1_fast.hip; FC1 [N,2688]x[2688,448] as %d 16-bit products per fp32 product)" % (fc1_plan, nprod),
                                 "bound": "mfma", "achieved": nprod * f_alg, "peak": PEAK_BF16_MFMA_TFLOPS,
                                 "unit": "TFLOP/s (16-bit products issued)", "frac": nprod * f_alg / PEAK_BF16_MFMA_TFLOPS,
                                 "algorithmic_f32_tflops": f_alg, "avg_launch_ms": f_ms, "launches_timed": f_st["timed"]["fc1"],
                                 "flop_per_ctu_issued": nprod * FC1_FLOP_PER_CTU, **pmc_traffic("%s_plan%d" % (args.workload, fc1_plan)),
                                 "note": "the chip lowers its shader clock under dense 16-bit MFMA streams (profiles/r04_power_probe.txt): "
                                         "the data-sheet peak assumes 2.4 GHz"},
                    "stages_ms_per_step": {k: v / 3.0 for k, v in f_all["ms"].items()},
                    "hbm": step_hbm("%s_plan%d" % (args.workload, plan), f_elapsed / args.steps * 1e3),
                    "max_abs_vs_exact": float(np.abs(fast_out - exact_out).max()) if same_zero else None,
                    "flips_vs_exact": int(((fast_out > 0.5) != (exact_out > 0.5)).sum()),
                    "gate_pattern_equal": same_zero,
                    "outputs_compared": int(fast_out.size),
                    "note": "same K steps, same barriers, same frames as `value`; compared: the gated probabilities of the whole step "
                            "(shipped thresholds 0.5 / 0.5) of this plan and of the exact plan; tests/test_gpu_fast_plan.py holds the <= 1e-4 bar",
                }
        ctx.set_fc1_plan(0)
        step()  # d_out holds the exact plan's output again (first_frame_parity below reads it)
        ctx.synchronize()

    result = None
    if rank == 0:
        total_ctus = ctus_per_step * args.steps * world
        value = total_ctus / elapsed
        result = {
            "metric": "CTUs/sec (ETH-CNN inference)", "value": value, "unit": "CTU/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic (seeded luma frames resident in HBM; seeded synthetic weights -- trained blobs absent from the reference)",
            "config": {"workload": wl["name"], "width": W, "height": H, "frames_per_gpu": NF, "qp": QP,
                       "ctus_per_step_per_gpu": ctus_per_step, "sharding": "frame ranges, no collective",
                       "ranks": world, "devices_visible": torch.cuda.device_count(), "rank0_device": local_rank,
                       "one_rank_per_device": os.environ.get("BENCH_FORCE_DEVICE") is None,  # False only under the one-GPU test hook
                       "rendezvous_backend": backend if world > 1 else None,
                       "device": ctx.device_name, "host_affinity": numa, "host_fill_threads_per_rank": ctx.host_threads},
        }
    if rank == 0 and args.full:
        # level 1 times the FC1 stage of every 3rd pass of the timed region; the rate uses the CTUs of exactly those passes
        fc1_ms = st["ms"]["fc1"] / max(1, st["timed"]["fc1"])
        ctus_per_launch = st["timed_ctus"]["fc1"] / max(1, st["timed"]["fc1"])
        fc1_tflops = FC1_FLOP_PER_CTU * st["timed_ctus"]["fc1"] / (st["ms"]["fc1"] * 1e-3) / 1e12 if st["ms"]["fc1"] > 0 else 0.0
        tile_ms = st_all["ms"]["tile"] / max(1, st_all["timed"]["tile"])
        tile_gbps = 4096.0 * st_all["timed_ctus"]["tile"] / (st_all["ms"]["tile"] * 1e-3) / 1e9 if st_all["ms"]["tile"] > 0 else 0.0
        kernel_ms = sum(st_all["ms"].values()) / 3.0
        result.update({
            "roofline": {"kernel": FC1_KERNEL_NOTE,
                         "bound": "mfma", "achieved": fc1_tflops, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": fc1_tflops / PEAK_F32_MFMA_TFLOPS, **pmc_traffic(args.workload),
                         "avg_launch_ms": fc1_ms, "launches_timed": st["timed"]["fc1"], "ctus_per_launch": ctus_per_launch,
                         "flop_per_ctu": FC1_FLOP_PER_CTU,
                         "profile": "profiles/r06_kernel_stats_by_grid_%s.csv: row k_fc1_* of this workload's grid size (rocprofv3 kernel trace of this "
                                    "command with --no-other-configs --no-fast-plan)" % args.workload,
                         "note": "rank 0's launches, timed inside the measured region, i.e. with the next step's CTU-load stage "
                                 "running beside them; alone on the GPU the same launch takes stages_ms_per_step.fc1"},
            "stages_ms_per_step": {k: v / 3.0 for k, v in st_all["ms"].items()},
            "stages_note": ("each stage alone on one stream (ethcnn_set_pass_pipeline off), 3 untimed steps; in the timed region the "
                            "tile stage of step i+1 runs beside FC1 of step i, so ms_per_step < the sum of these"),
            "stages_frac_of_f32_mfma_peak": stage_fracs({k: v / 3.0 for k, v in st_all["ms"].items()}, ctus_per_step),
            "kernel_ms_per_step": kernel_ms,
            "hbm": step_hbm(args.workload, elapsed / args.steps * 1e3),
            "whole_path_tflops": 2.0 * MAC_PER_CTU * total_ctus / elapsed / 1e12,
            "whole_path_frac_of_f32_mfma_peak": 2.0 * MAC_PER_CTU * total_ctus / elapsed / 1e12 / PEAK_F32_MFMA_TFLOPS / world,
            "ctu_load_stage": {"kernel": "k0_tile", "bound": "hbm", "achieved": tile_gbps, "peak": PEAK_HBM_GBPS,
                               "unit": "GB/s", "frac": tile_gbps / PEAK_HBM_GBPS, "avg_launch_ms": tile_ms,
                               "algorithmic_bytes_per_ctu": 4096,
                               "counter_bytes_per_ctu": ctu_load_counters(args.workload, ctus_per_step),
                               "form": "k0_tile_slab on a side stream beside FC1 of the previous step; the form folded into the trunk "
                                       "(no slab records, no side stream) was measured 3.5 % slower per step (profiles/r04_tile_fold.txt)"},
        })
        # box calibration, right behind the timed region (same clocks, same temperature): what THIS GPU sustains in pure
        # exact-fp32 MFMAs.  Boxes of one pool differ by several per cent (round 3 saw 39.4 - 42.0 M CTU/s from the same code);
        # frac_of_box_mfma_rate is the fraction that does not move with the box
        try:
            box = ctx.measure_mfma_rate(0.05)
            result["roofline"]["box_mfma_tflops"] = box
            result["roofline"]["frac_of_box_mfma_rate"] = fc1_tflops / box if box > 0 else None
            result["roofline"]["box_note"] = ("pure v_mfma_f32_16x16x4_f32 for 50 ms on this GPU right after the timed region "
                                              "(ethcnn_measure_mfma_rate); 'peak' stays the data-sheet 157.3")
        except Exception as exc:  # noqa: BLE001  (calibration only: never fail the bench line)
            result["roofline"]["box_mfma_tflops"] = None
            result["roofline"]["box_note"] = "calibration failed: %s" % exc
        # N > 1: the CPU baseline is the same single-box measurement, on a shorter sample (the other ranks wait at the
        # final barrier meanwhile); the per-GPU side measurements that need the GPU to themselves are N = 1 only
        cpu_seconds = args.cpu_seconds if world == 1 else min(args.cpu_seconds, 8.0)
        if ldp:
            result.pop("whole_path_tflops", None)  # MAC_PER_CTU is the All-Intra path's
            result.pop("whole_path_frac_of_f32_mfma_peak", None)
            result.pop("stages_frac_of_f32_mfma_peak", None)
            result["roofline"]["note"] = ("latency-bound call (one frame, %d CTUs): the serial K chain of FC1 sets the "
                                          "launch time, not the MFMA rate; stage 'heads' = k_lstm_cell + k_lstm_heads" % nctu)
            result["config"]["sharding"] = "none (lock-step with the encoder): replicas only"
            if not args.no_cpu_baseline:
                result["cpu_baseline"] = cpu_baseline_ldp(luma, W, H, QP, cpu_seconds)
            result["parity_first_frames_bit_exact"] = ldp_parity(ctx, luma, W, H, QP)
        if 2 in fast:
            result["fast_plan_fp16x2"] = fast[2]
        if 3 in fast:
            result["fast_plan_fp16x2_trunk"] = fast[3]
        if sharded is not None:
            result["host_scopes"] = sharded
        if not ldp and not (args.no_host_scopes and args.no_cpu_baseline):
            with YuvFile(luma, W, H) as yuv:
                if not args.no_host_scopes and world == 1:
                    result["host_scopes"] = host_scopes(ctx, luma, W, H, NF, QP, yuv)
                if not args.no_cpu_baseline:
                    result["cpu_baselines"] = cpu_baselines(luma, W, H, QP, cpu_seconds, yuv, full=(world == 1))
                    result["cpu_baseline"] = dict(result["cpu_baselines"][0])
        # the north star's ratio, stated in the line: the reference's own timed scope (4:2:0 file -> cu_depth.dat, 'Predicting Time',
        # video_to_cu_depth.py:142-145) on the GPU vs on this box's host cores.  BASELINE.md holds no published number, so the
        # denominator is measured here -- by PORTS (TensorFlow cannot run in this image): the C oracle on all usable cores, and the
        # structure-faithful TF-CPU proxy.  `vs_baseline` = S3 GPU / S3 oracle port.
        hs, cbs = result.get("host_scopes"), result.get("cpu_baselines")
        if not ldp and world == 1 and hs and cbs and hs.get("s3_file_to_file_ctus_per_s"):
            s3 = hs["s3_file_to_file_ctus_per_s"]
            b1 = next((b for b in cbs if b.get("name", "").startswith("B1 oracle") and "file scope" in b.get("name", "") and b.get("value")), None)
            b2 = next((b for b in cbs if b.get("name", "").startswith("B2 TF-CPU proxy") and b.get("value")), None)
            if b1:
                result["vs_baseline"] = s3 / b1["value"]
                result["vs_baseline_detail"] = {
                    "numerator": "S3 on 1 x MI355X: 4:2:0 file -> cu_depth.dat through ethcnn_predict_yuv_file (PCIe + file I/O inside), %.0f CTU/s" % s3,
                    "denominator": "%s: %.0f CTU/s on %s cores (kind: port -- the C restatement oracle/ethcnn_oracle.c, not TensorFlow)" % (b1["name"], b1["value"], b1["cores"]),
                    "scope": b1.get("scope"), "kind": "port", "cores": b1["cores"]}
            if b2:
                result["vs_tf_cpu_proxy"] = s3 / b2["value"]
                result["vs_tf_cpu_proxy_detail"] = {
                    "denominator": "%s: %.0f CTU/s on %s threads (kind: port -- per-frame Python tiling + torch-CPU ops in the reference's feed structure)" % (b2["name"], b2["value"], b2["cores"]),
                    "scope": b2.get("scope"), "kind": "port", "cores": b2["cores"]}
            ratios = [result.get("vs_baseline"), result.get("vs_tf_cpu_proxy")]
            result["north_star_10x"] = bool(ratios[0] is not None and ratios[0] >= 10.0 and (ratios[1] is None or ratios[1] >= 10.0))
            result["north_star_note"] = ("target: >= 10x the reference CPU path's CTUs/sec on 3840x2160 QP32 at 1 GPU (BASELINE.json); both "
                                         "denominators are ports timed on this box (TensorFlow is not installable here), same scope on both sides")
        if not ldp and world == 1 and not args.no_host_scopes:
            result["single_picture_latency"] = single_picture_latency(ctx, QP)
        # every other single-GPU BASELINE config, timed by THIS run too (short regions, never `value`): VERDICT r04 item 4
        if not ldp and world == 1 and not args.no_other_configs:
            result["other_configs"] = other_configs(ctx, args.workload)
        # sanity: the benchmark output is the real thing (first frame vs oracle), outside the timed region
        if not ldp:
            result["parity_first_frame_bit_exact"] = first_frame_parity(ctx, d_out, luma, W, H, QP, nctu)
            if world == 1 and not args.no_cpu_baseline:
                result["decision_stability"] = decision_stability(ctx, luma, W, H, QP)
    if rank == 0:
        print(json.dumps(result))
        sys.stdout.flush()
    d_in.free()
    d_out.free()
    ctx.close()
    if dist is not None:
        if backend == "nccl":
            dist.barrier(device_ids=[local_rank])
        else:
            dist.barrier()
        dist.destroy_process_group()
    return 0


FC1_KERNEL_NOTE = "FC1 stage = k_fc1_bulk / k_fc1_p3 (FC1 [N,2688]x[2688,448], v_mfma_f32_16x16x4_f32)"


def self_launch(ngpus, visible):
    """`python bench.py --gpus N` outside torchrun: start the N ranks ourselves (one per GPU), or refuse.  The line rank 0
    prints goes to our stdout unchanged; our exit status is the launcher's."""
    import socket
    import subprocess
    if visible < ngpus and os.environ.get("BENCH_FORCE_DEVICE") is None:
        sys.stderr.write("bench.py: --gpus %d but only %d GPU(s) visible on this node: refusing to print a line for GPUs that "
                         "were not measured (run under torchrun with one rank per GPU, or lower --gpus)\n" % (ngpus, visible))
        return 2
    with socket.socket() as sk:  # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ngpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between the ranks needs it on these hosts
    env.setdefault("OMP_NUM_THREADS", "1")             # torchrun's own default, said explicitly (no warning banner)
    return subprocess.call(cmd, env=env)


def host_scopes_sharded(ctx, luma, W, H, NF, QP, rank, world, dist, backend, barrier):
    """N > 1 side measurements (never `value`), all ranks at once -- what a node really does with the reference's job:
      S2 sharded: every rank pushes its own pageable host frames through its GPU at the same time (host DRAM + PCIe shared);
      S3 sharded: ONE 4:2:0 file holding every rank's frames -> ONE cu_depth.dat, each rank preads its frame range and
                  pwrites its slice (ethcnn_predict_yuv_shard) -- the multi-GPU form of 'Predicting Time'.
    Rates are whole-job (sum over ranks / slowest rank's time), best of 3."""
    import numpy as np
    import shutil
    import tempfile
    import torch
    nctu = ((W + 63) // 64) * ((H + 63) // 64)

    def slowest(dt):
        t = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    out = {"ranks": world, "fill_threads_per_rank": ctx.host_threads}
    ctx.predict_luma(luma, W, H, NF, QP)  # warm the staging ring
    best = 1e30
    for _ in range(3):
        barrier()
        t0 = time.perf_counter()
        ctx.predict_luma(luma, W, H, NF, QP)
        best = min(best, slowest(time.perf_counter() - t0))
    out["s2_host_to_host_ctus_per_s"] = world * NF * nctu / best
    out["s2_h2d_gbps_total"] = world * NF * W * H / best / 1e9

    # one shared file: rank 0 picks the directory (tmpfs when it has room), every rank writes its own frames into it
    frame_bytes = W * H * 3 // 2
    need = world * NF * frame_bytes + world * NF * nctu * 84 + (64 << 20)
    box = [None]
    if rank == 0:
        for d in ("/dev/shm", tempfile.gettempdir()):
            try:
                sv = os.statvfs(d)
                if sv.f_bavail * sv.f_frsize > need:
                    box[0] = tempfile.mkdtemp(prefix="ethcnn_bench_", dir=d)
                    break
            except OSError:
                pass
    dist.broadcast_object_list(box, src=0)
    if box[0] is None:
        out["s3_note"] = "no file system with %.1f GB free for the shared YUV file: file scope skipped" % (need / 1e9)
        return out
    yuv, dat = os.path.join(box[0], "seq.yuv"), os.path.join(box[0], "cu_depth.dat")
    try:
        if rank == 0:
            with open(yuv, "wb") as f:
                f.truncate(world * NF * frame_bytes)
            with open(dat, "wb") as f:
                f.truncate(world * NF * nctu * 84)
        barrier()
        chroma = np.full(W * H // 2, 128, dtype=np.uint8).tobytes()
        with open(yuv, "r+b") as f:
            f.seek(rank * NF * frame_bytes)
            for k in range(NF):
                f.write(luma[k].tobytes())
                f.write(chroma)
        barrier()
        f0, f1 = rank * NF, (rank + 1) * NF
        ctx.predict_yuv_shard(yuv, W, H, QP, dat, f0, f1)
        best = 1e30
        for _ in range(3):
            barrier()
            t0 = time.perf_counter()
            ctx.predict_yuv_shard(yuv, W, H, QP, dat, f0, f1)
            best = min(best, slowest(time.perf_counter() - t0))
        out["s3_file_to_file_ctus_per_s"] = world * NF * nctu / best
        out["s3_luma_gbps_total"] = world * NF * W * H / best / 1e9
        out["s3_file"] = "%d frames of %dx%d 4:2:0 (%.2f GB) in %s, one frame range per rank" % (world * NF, W, H, world * NF * frame_bytes / 1e9, os.path.dirname(box[0]))
        barrier()
        # ... and what the encoder would see: the drop-in COMMAND over all the job's GPUs -- one process, a worker thread
        # per GPU (tools/video_to_cu_depth.c -> ethcnn_predict_yuv_file_sharded) -- on the same file, wall time incl. process start, N
        # contexts and the exit; rank 0 runs it while the other ranks wait at the barrier (their contexts stay allocated, idle)
        if rank == 0:
            out["sharded_command"] = sharded_command(box[0], yuv, W, H, QP, world, nctu * NF * world)
        barrier()
    finally:
        barrier()
        if rank == 0:
            shutil.rmtree(box[0], ignore_errors=True)
    out["note"] = "best of 3, whole job: sum over ranks / slowest rank; every rank runs at the same time"
    return out


def sharded_command(workdir, yuv, W, H, QP, world, total_ctus):
    """wall time of `ETHCNN_DEVICES=<the ranks' GPUs> video_to_cu_depth <yuv> <w> <h> <qp>` (native tool), median of 3 behind a warm-up run;
    a side measurement: any failure is reported, never raised"""
    import subprocess
    tool = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "video_to_cu_depth")
    try:
        forced = os.environ.get("BENCH_FORCE_DEVICE")
        devices = [int(forced)] * world if forced is not None else list(range(world))
        cwd = os.path.join(workdir, "cmd")
        os.makedirs(cwd, exist_ok=True)
        open(os.path.join(cwd, "Thr_info.txt"), "w").write("0.5 0.5 0.5 0.5 0.5 0.5\n")
        env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="1", ETHCNN_DEVICES=",".join(str(d) for d in devices))
        for k in ("ETHCNN_LOCAL_WORKERS", "LOCAL_WORLD_SIZE", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)  # (the command is ONE process with its own worker threads: the node budget is divided inside it)
        walls = []
        for rep in range(4):
            t0 = time.perf_counter()
            r = subprocess.run([tool, yuv, str(W), str(H), str(QP)], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                return {"error": r.stderr[-300:]}
            if rep:
                walls.append(time.perf_counter() - t0)
        w = sorted(walls)[len(walls) // 2]
        return {"wall_ms": w * 1e3, "ctus_per_s": total_ctus / w, "workers": world, "devices": devices,
                "what": "native tool, one process, a worker thread per GPU, whole command incl. process start / N contexts / exit; median of 3"}
    except Exception as exc:  # noqa: BLE001
        return {"error": str(exc)}


def pin_to_gpu_numa_node(device_name):
    """Run this process on the CPUs of the GPU's host NUMA node (the library reports it in its device string), as one
    would deploy it: on the two-socket boxes the host scopes (S2 / S3) lose a third of their rate when the caller's luma or
    the page cache of the YUV file sits on the other socket.  The HBM-resident `value` does not depend on it."""
    import re
    m = re.search(r"host NUMA node (\d+)", device_name or "")
    if not m or not hasattr(os, "sched_setaffinity"):
        return "not pinned"
    try:
        cpus = set()
        for part in open("/sys/devices/system/node/node%s/cpulist" % m.group(1)).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if cpus:
            os.sched_setaffinity(0, cpus)
            return "NUMA node %s (%d CPUs)" % (m.group(1), len(cpus))
    except Exception:
        pass
    return "not pinned"


def first_frame_parity(ctx, d_out, luma, W, H, QP, nctu):
    try:
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import ethcnn_np as oracle
        got = d_out.download(np.float32, nctu * 21).reshape(nctu, 21)
        want = oracle.predict_frames(ctx.get_blob(), luma[0], W, H, 1, QP, 0.5, 0.5, mode=0)
        return bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    except Exception as exc:  # the oracle is a checker only; never fatal for the measurement
        return "unchecked: %s" % exc


def other_configs(ctx, skip):
    """Short timed regions (5 steps; LDP: 40 frames) of the BASELINE configs the headline does not run, on the same context and
    weights, inputs resident in HBM, exact plan, first frame(s) checked bit for bit against the oracle.  Frames beyond the first few
    are repeats (generating 54 distinct 4928x3264 frames costs more than the measurement); throughput does not depend on content."""
    import numpy as np
    out = {}
    for key in ("c2", "c3", "c4", "c5"):
        if key == skip:
            continue
        wl = WORKLOADS[key]
        W, H, NF, QP = wl["width"], wl["height"], wl["frames"], wl["qp"]
        nctu = ((W + 63) // 64) * ((H + 63) // 64)
        t_all = time.perf_counter()
        try:
            if wl.get("ldp"):
                ctx.load_lstm_synthetic(seed=2, head_gain=3.0)
                luma = synth_luma(W, H, NF, seed=0xE7C00000 + 5)
                d_in, d_out, d_vec = ctx.alloc(luma.nbytes), ctx.alloc(nctu * 21 * 4), ctx.alloc(nctu * 448 * 4)
                d_state = [ctx.alloc(nctu * 896 * 4), ctx.alloc(nctu * 896 * 4)]
                d_in.upload(luma)

                def frame(i):
                    ctx._chk(ctx.lib.ethcnn_resi_vectors_device(ctx.h, d_in.ptr + (i % NF) * W * H, W, H, W, d_vec.ptr))
                    ctx._chk(ctx.lib.ethcnn_lstm_step_device(ctx.h, d_vec.ptr, d_state[i & 1].ptr if i > 0 else None, nctu, QP,
                                                             i + 1, d_state[(i + 1) & 1].ptr, d_out.ptr))
                for i in range(20):
                    frame(i)
                ctx.synchronize()
                n = 40
                t0 = time.perf_counter()
                for i in range(n):
                    frame(20 + i)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                out[key] = {"workload": wl["name"], "us_per_frame": dt / n * 1e6, "value": nctu * n / dt, "unit": "CTU/s", "frames_timed": n,
                            "parity_first_frames_bit_exact": ldp_parity(ctx, luma, W, H, QP),
                            "note": "device-resident calls back to back (resi_cnn + one ETH-LSTM step + heads + gates per frame, state in HBM); "
                                    "latency-bound: one frame per call, lock-step with the encoder"}
                for b in [d_in, d_out, d_vec] + d_state:
                    b.free()
            else:
                distinct = min(NF, 3 if W * H > 8000000 else 5)
                base = synth_luma(W, H, distinct, seed=0xE7C00000 + int(key[1]))
                luma = np.concatenate([base] * (NF // distinct) + ([base[:NF % distinct]] if NF % distinct else []))
                d_in, d_out = ctx.alloc(luma.nbytes), ctx.alloc(nctu * NF * 21 * 4)
                d_in.upload(luma)
                t_ramp = time.perf_counter()
                while time.perf_counter() - t_ramp < 0.1:
                    ctx.predict_luma_device(d_in, W, H, NF, QP, d_out)
                    ctx.synchronize()
                ctx.set_profiling(1)
                ctx.reset_stage_times()
                steps = 5
                t0 = time.perf_counter()
                for _ in range(steps):
                    ctx.predict_luma_device(d_in, W, H, NF, QP, d_out)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                st = ctx.stage_times()
                ctx.set_profiling(0)
                fc1_tf = FC1_FLOP_PER_CTU * st["timed_ctus"]["fc1"] / (st["ms"]["fc1"] * 1e-3) / 1e12 if st["ms"]["fc1"] > 0 else 0.0
                out[key] = {"workload": wl["name"], "value": nctu * NF * steps / dt, "unit": "CTU/s", "steps": steps,
                            "ms_per_step": dt / steps * 1e3, "ctus_per_step": nctu * NF, "fc1_frac": fc1_tf / PEAK_F32_MFMA_TFLOPS,
                            "whole_path_frac_of_f32_mfma_peak": 2.0 * MAC_PER_CTU * nctu * NF * steps / dt / 1e12 / PEAK_F32_MFMA_TFLOPS,
                            "parity_first_frame_bit_exact": first_frame_parity(ctx, d_out, luma, W, H, QP, nctu),
                            "distinct_frames": distinct}
                d_in.free()
                d_out.free()
            out[key]["wall_s"] = time.perf_counter() - t_all
        except Exception as exc:  # noqa: BLE001  (a side measurement never fails the bench line)
            out[key] = {"workload": wl["name"], "error": "%s: %s" % (type(exc).__name__, exc)}
    return out


def single_picture_latency(ctx, QP):
    """Side measurement (never `value`): one picture per call, luma resident in HBM, call + synchronise -- what the in-process
    encoder hook and the LDP daemon pay per picture.  Single-launch pass (csrc/ethcnn_small.hip) vs the five-launch path."""
    out = {"unit": "us per call (device-resident luma -> probabilities, incl. launch + synchronise)",
           "note": "one launch = CTU gather + trunk -> FC1 -> heads -> gates as a dataflow inside one grid (default); five launches = "
                   "tile / trunk / FC1 / heads / gate (ethcnn_set_small_pass_launch off)"}
    try:
        for name, w, h in (("768x512", 768, 512), ("1920x1080", 1920, 1080)):
            luma = synth_luma(w, h, 1, 3)
            nctu = ((w + 63) // 64) * ((h + 63) // 64)
            d_in, d_out = ctx.alloc(luma.nbytes), ctx.alloc(nctu * 84)
            d_in.upload(luma)
            row = {}
            for label, on in (("one_launch", True), ("five_launches", False)):
                ctx.set_small_pass_launch(on)
                for _ in range(30):
                    ctx.predict_luma_device(d_in, w, h, 1, QP, d_out)
                    ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(200):
                    ctx.predict_luma_device(d_in, w, h, 1, QP, d_out)
                    ctx.synchronize()
                row[label] = (time.perf_counter() - t0) / 200 * 1e6
            ctx.set_small_pass_launch(True)
            d_in.free()
            d_out.free()
            out[name] = row
        # host memory -> host memory through ethcnn_predict_luma: what a caller with the picture in its own memory pays (round 4: the
        # single-launch pass PULLS a page-locked picture over PCIe itself, a pageable one is staged under the queued launch, the
        # launch's last block hands the probabilities back; profiles/r04_latency_host.txt)
        import numpy as np
        h2h = {"unit": "us per call (host luma -> host probabilities)"}
        for name, w, h in (("1920x1080", 1920, 1080), ("3840x2160", 3840, 2160)):
            luma = synth_luma(w, h, 1, 5)
            nctu = ((w + 63) // 64) * ((h + 63) // 64)
            pin = ctx.host_buffer(w * h)
            pin[:] = luma.reshape(-1)
            pout = ctx.host_buffer(nctu * 84).view(np.float32)
            row = {}
            for label, src in (("page_locked", pin.reshape(1, h, w)), ("pageable", luma)):
                def call():
                    if label == "page_locked":
                        ctx._chk(ctx.lib.ethcnn_predict_luma(ctx.h, pin.ctypes.data, w, h, w, w * h, 1, QP, pout.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
                    else:
                        ctx.predict_luma(src, w, h, 1, QP)
                for _ in range(20):
                    call()
                t0 = time.perf_counter()
                for _ in range(100):
                    call()
                row[label] = (time.perf_counter() - t0) / 100 * 1e6
            ctx.free_host_buffers()
            h2h[name] = row
        out["host_to_host"] = h2h
    except Exception as exc:  # a side measurement is never fatal
        out["error"] = str(exc)
    return out


def decision_stability(ctx, luma, W, H, QP, frames=2):
    """knife-edge accounting on the first frames of the workload (oracle/stability.py; the full C3 x 4 QP x 2 gain
    table is profiles/r02_decision_stability.json): outputs near a shipped threshold and thresholded decisions that
    differ from the literal-TF-order fp32 and the float64 evaluations of the same graph"""
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import stability
        frames = min(frames, luma.shape[0])
        t1, t2 = ctx.get_thresholds()
        ctx.set_thresholds(-1.0, -1.0)
        got = ctx.predict_luma(luma[:frames], W, H, frames, QP)
        ctx.set_thresholds(t1, t2)
        lit, f64 = stability.ungated_references(ctx.get_blob(), luma[:frames], W, H, frames, QP)
        rep = stability.report(got, lit, f64)
        near = {b: sum(d["within_" + b] for d in rep["thresholds"].values()) for b in ("1e-06", "1e-05", "0.0001")}
        return {"sample": "first %d frame(s), %d outputs x %d shipped thresholds" % (frames, rep["outputs"], len(rep["thresholds"])),
                "max_abs_vs_literal_fp32": rep["max_abs_vs_literal_fp32"], "max_abs_vs_float64": rep["max_abs_vs_float64"],
                "flips_vs_literal_fp32": rep["flips_vs_literal_fp32_total"], "flips_vs_float64": rep["flips_vs_float64_total"],
                "outputs_within_of_a_threshold": near}
    except Exception as exc:
        return "unchecked: %s" % exc


def ldp_parity(ctx, luma, W, H, QP):
    """first three frames of the LDP chain through the host entry point vs the oracle chain"""
    try:
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import ethcnn_np as oracle
        import ethcnn_lstm_np as ol
        cb, lb = ctx.get_blob(), ctx.get_lstm_blob()
        gs = os_ = None
        for i in (1, 2, 3):
            gp, gs = ctx.ldp_predict_frame(luma[i - 1], W, H, QP, i, gs)
            op, os_ = ol.lstm_step(lb, oracle.resi_vectors(cb, luma[i - 1], W, H), os_, QP, i, 0.5, 0.5, mode=0)
            if not (np.array_equal(gp.view(np.uint32), op.view(np.uint32)) and
                    np.array_equal(gs.view(np.uint32), os_.view(np.uint32))):
                return False
        return True
    except Exception as exc:
        return "unchecked: %s" % exc


def cpu_baseline_ldp(luma, W, H, QP, target_seconds):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ethcnn_np as oracle
    import ethcnn_lstm_np as ol
    cb, lb = oracle.synth_blob(1, 8.0), ol.synth_lstm_blob(2, 3.0)
    nctu = ((W + 63) // 64) * ((H + 63) // 64)
    logical, cores, quota = usable_host_cpus()
    oracle.set_threads(cores)
    st, n, t0 = None, 0, time.perf_counter()
    while time.perf_counter() - t0 < target_seconds or n < 2:
        _, st = ol.lstm_step(lb, oracle.resi_vectors(cb, luma[n % luma.shape[0]], W, H), st, QP, n + 1, 0.5, 0.5, mode=0)
        n += 1
    dt = time.perf_counter() - t0
    return {"value": n * nctu / dt, "unit": "CTU/s", "cores": cores, "kind": "port",
            "host": "%d logical CPUs, cgroup CPU quota %s" % (logical, "none" if quota is None else "%.1f cores" % quota),
            "sample": "%d consecutive frames of %dx%d (%d CTUs each), oracle resi_vectors (OpenMP) + oracle_lstm_step, %.1f s"
                      % (n, W, H, nctu, dt)}


def _step_traffic():
    """profiles/step_traffic.json (scripts/gpu_step_traffic.sh -> scripts/pmc_traffic.py), or None when it was taken at other kernel
    sources: the committed PMC passes are only valid for the device code they ran (one hash over every .hip / .h of csrc/)"""
    d = json.load(open(os.path.join(ROOT, "profiles", "step_traffic.json")))
    return d if d.get("kernel_source_stamp") == kernel_source_stamp() else None


def pmc_traffic(key):
    """HBM bytes per FC1 launch of the step `key` (c3 / c2 / c3_plan2 ...).  PMC counters cannot be read from inside this process: they
    come from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this command restricted to ONE workload
    (--no-other-configs), aggregated per kernel AND grid size (scripts/pmc_traffic.py; VERDICT r05: the round-5 figure averaged the
    FC1 dispatches of three workloads).  The number is the sum of the FC1 rows of hbm.per_kernel_bytes -- the same file, the same rows.
    FETCH_SIZE is doubled (gfx950 under-counts wide coalesced reads by 2x, MI355X_MICROARCH.md)."""
    try:
        d = _step_traffic()
        if d is None:
            return {"traffic": None, "traffic_note": "profiles/step_traffic.json was taken at other kernel sources: re-run scripts/gpu_step_traffic.sh"}
        e = d[key]
        return {"traffic": e["fc1_bytes_per_launch"], "traffic_unit": "B/launch", "traffic_algorithmic": e["fc1_algorithmic_bytes_per_launch"],
                "traffic_over_algorithmic": e["fc1_bytes_per_launch"] / e["fc1_algorithmic_bytes_per_launch"],
                "traffic_rows": {k: v["bytes"] for k, v in e["per_kernel"].items() if k.startswith("k_fc1")},
                "traffic_source": d["source"], "traffic_kernel_source_stamp": d["kernel_source_stamp"]}
    except Exception:
        return {"traffic": None}


def ctu_load_counters(key, n_ctus):
    """FETCH / WRITE counter bytes per CTU of the CTU-load stage (k0_tile_slab) from the same stamped file"""
    try:
        d = _step_traffic()
        e = next(v for k, v in d[key]["per_kernel"].items() if k.startswith("k0_tile"))
        return {"fetched": round(e["fetch_bytes"] / n_ctus, 1), "written": round(e["write_bytes"] / n_ctus, 1),
                "source": "profiles/step_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 / WRITE_SIZE of k0_tile_slab, scripts/gpu_step_traffic.sh)"}
    except Exception:
        return {"fetched": None, "written": None, "source": "profiles/step_traffic.json has no current k0_tile_slab row: re-run scripts/gpu_step_traffic.sh"}


def kernel_source_stamp():
    """identifies the device code of the whole step: one hash over the git blob hashes of every .hip / .h file of csrc/"""
    import hashlib
    src = os.path.join(ROOT, "hevc-complexity-reduction_amd", "csrc")
    names = sorted(f for f in os.listdir(src) if f.endswith((".hip", ".h")))
    return hashlib.sha1("".join(git_blob_sha1(os.path.join(src, f)) for f in names).encode()).hexdigest()[:16]


def step_hbm(key, ms_per_step):
    """HBM-side bytes of ONE step of a plan from the committed PMC passes (profiles/step_traffic.json, scripts/gpu_step_traffic.sh;
    key: c3 / c3_plan2 / c3_plan3) against this run's step time: how close the STEP is to the memory system, beside the FC1
    `roofline` object.  Valid only for the kernel sources the passes were taken at."""
    try:
        d = _step_traffic()
        if d is None:
            return {"bytes_per_step": None, "note": "profiles/step_traffic.json was taken at other kernel sources: re-run scripts/gpu_step_traffic.sh"}
        e = d[key]
        gbps = e["bytes_per_step"] / (ms_per_step * 1e-3) / 1e9
        return {"bytes_per_step": e["bytes_per_step"], "gbps": gbps, "frac_of_6.3TBps": gbps / 6300.0,
                "algorithmic_bytes_per_step": e["algorithmic_bytes_per_step"], "per_kernel_bytes": {k: v["bytes"] for k, v in e["per_kernel"].items()},
                "source": d["source"], "note": "counter bytes (FETCH_SIZE x 2 + WRITE_SIZE) of a separate PMC run / this run's ms_per_step; "
                                               "6.3 TB/s = what the guide calls achievable of the 8 TB/s peak"}
    except Exception as exc:  # noqa: BLE001
        return {"bytes_per_step": None, "note": "unavailable: %s" % exc}


def git_blob_sha1(path):
    """what `git hash-object <path>` prints (no git needed on the GPU box)"""
    import hashlib
    data = open(path, "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


class YuvFile:
    """the batch as an 8-bit 4:2:0 file (chroma = 128) on tmpfs, shared by the file-scope measurements"""

    def __init__(self, luma, W, H):
        import tempfile
        import numpy as np
        self.dir = tempfile.mkdtemp(prefix="ethcnn_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        self.path = os.path.join(self.dir, "seq.yuv")
        chroma = np.full(W * H // 2, 128, dtype=np.uint8).tobytes()
        with open(self.path, "wb") as f:
            for k in range(luma.shape[0]):
                f.write(luma[k].tobytes())
                f.write(chroma)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import shutil
        shutil.rmtree(self.dir, ignore_errors=True)
        return False


def stage_fracs(stage_ms, ctus):
    """fraction of the fp32-MFMA peak each MFMA stage reaches alone on the GPU (algorithmic FLOP of the stage / its time):
    trunk 279,552 MAC, FC1 1,204,224, heads 68,373 per CTU"""
    mac = {"trunk": 279552, "fc1": 1204224, "heads": 68373}
    return {k: (2.0 * m * ctus / (stage_ms[k] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS) for k, m in mac.items() if stage_ms.get(k)}


def host_scopes(ctx, luma, W, H, NF, QP, yuv):
    """Side measurements OUTSIDE the timed region (never `value`): the same batch through the
    host entry points.  S2 = pageable host luma -> host probabilities (pinned staging, H2D,
    kernels, D2H); S3 = the reference's own scope ('Predicting Time', video_to_cu_depth.py:142-145):
    4:2:0 file -> cu_depth.dat on a tmpfs-backed temp dir.  Best of 3 (single shots are noisy)."""
    nctu = ((W + 63) // 64) * ((H + 63) // 64)
    out = {}
    ctx.predict_luma(luma, W, H, NF, QP)  # warm the staging buffers
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.predict_luma(luma, W, H, NF, QP)
        best = min(best, time.perf_counter() - t0)
    out["s2_host_to_host_ctus_per_s"] = NF * nctu / best
    out["s2_h2d_gbps"] = NF * W * H / best / 1e9
    dat = os.path.join(yuv.dir, "cu_depth.dat")
    ctx.predict_yuv_file(yuv.path, W, H, QP, dat)
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.predict_yuv_file(yuv.path, W, H, QP, dat)
        best = min(best, time.perf_counter() - t0)
    out["s3_file_to_file_ctus_per_s"] = NF * nctu / best
    out["s3_luma_gbps"] = NF * W * H / best / 1e9
    out["cold_start_ms"] = cold_start_ms()
    out["note"] = ("best of 3; measured H2D rate of this box's DMA engine from pinned memory: 57.5 GB/s = 14.0 M CTU/s at 4096 B/CTU "
                   "(profiles/r02_host_copy.txt)")
    return out


def cold_start_ms():
    """What the reference's caller sees: HM blocks in system("python video_to_cu_depth.py ...") (TAppEncCfg.cpp:2317-2321), so the
    COMMAND's wall time is the cost -- on the reference's own C1 case (768x512 x 1 frame = 96 CTUs = 41 us of GPU) all of it is cold
    start: process, imports, HIP runtime, context, weights, exit.  Median of 3 runs behind one warm-up run, Python launcher and native C
    tool, in a tmpfs directory with seeded weights (no checkpoint parse: +~10 ms with one).  scripts/cold_start.py has the break-down
    and the sharded forms (profiles/r06_cold_start.txt).  The reference quotes 1~10 s of TensorFlow start-up (README.md:124)."""
    import shutil
    import subprocess
    import tempfile
    import numpy as np
    out = {}
    d = tempfile.mkdtemp(prefix="cold_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        w, h = 768, 512
        np.random.default_rng(1).integers(0, 256, size=w * h * 3 // 2, dtype=np.uint8).tofile(os.path.join(d, "seq.yuv"))
        open(os.path.join(d, "Thr_info.txt"), "w").write("0.5 0.5 0.5 0.5 0.5 0.5\n")
        env = dict(os.environ, ETHCNN_SYNTHETIC_SEED="3")
        for name, cmd in (("python_launcher", [sys.executable, os.path.join(ROOT, "video_to_cu_depth.py")]),
                          ("native_tool", [os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin", "video_to_cu_depth")])):
            if not os.path.exists(cmd[-1]):
                out[name] = None
                continue
            walls = []
            for rep in range(4):
                t0 = time.perf_counter()
                r = subprocess.run(cmd + ["seq.yuv", str(w), str(h), "32"], cwd=d, env=env, capture_output=True)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-300:])
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
            out[name] = sorted(walls)[len(walls) // 2]
        out["what"] = "wall ms of the whole C1 command (768x512, 1 frame, 96 CTUs), median of 3"
    except Exception as exc:  # noqa: BLE001  (a side measurement never fails the bench line)
        out["error"] = str(exc)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def usable_host_cpus():
    """-> (logical cpus visible, cpus this process may actually burn).  The GPU boxes run the job in a cgroup with a CPU
    quota (cpu.max 1600000/100000 = 16 cores of the 256 logical ones): more runnable threads than that get throttled by CFS
    and the oracle collapses (measured: 16 threads 125 k CTU/s, 32: 136 k, 256: 27 k)."""
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    usable = logical if quota is None else max(1, min(logical, int(quota + 0.5)))
    return logical, usable, quota


def cpu_baselines(luma, W, H, QP, target_seconds, yuv, full=True):
    """CPU baselines on the host cores of this box, each on a bounded sample of the same workload
    (BASELINE.md section 4).  [0] is also reported as `cpu_baseline`:
      [0] B1/S1  oracle (C port of the reference's CPU path, OpenMP over CTUs), all USABLE cores (the cgroup CPU quota of
                 the box, not its logical CPU count), frames in memory -> probabilities in memory (the scope of the GPU step);
      [1] B1/S1  the same on ONE thread;
      [2] B1/S3  the oracle at the reference's own timed scope: 4:2:0 file -> cu_depth.dat;
      [3] B2/S3  the TF-CPU proxy: per-CTU Python tiling loop + 1024-CTU feeds through torch-CPU ops
                 (video_to_cu_depth.py:61-73,88-106,142-145; TensorFlow itself cannot run here)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ethcnn_np as oracle
    logical, cores, quota = usable_host_cpus()
    host = "%d logical CPUs, cgroup CPU quota %s" % (logical, "none" if quota is None else "%.1f cores" % quota)
    blob = oracle.synth_blob(1, 8.0)
    NF = luma.shape[0]
    nctu = ((W + 63) // 64) * ((H + 63) // 64)
    budget = {"all": 0.35 * target_seconds, "one": 0.2 * target_seconds, "s3": 0.15 * target_seconds, "proxy": 0.3 * target_seconds}
    out = []

    def timed_passes(frames, seconds, label, threads):
        oracle.set_threads(threads)
        t0 = time.perf_counter()
        oracle.predict_frames(blob, luma[:frames], W, H, frames, QP, 0.5, 0.5, mode=0)  # warm: threads up, pages touched
        per_pass = time.perf_counter() - t0
        reps = int(max(1, min(200, round(seconds / max(per_pass, 1e-6)))))
        t0 = time.perf_counter()
        for _ in range(reps):
            oracle.predict_frames(blob, luma[:frames], W, H, frames, QP, 0.5, 0.5, mode=0)
        dt = time.perf_counter() - t0
        n = reps * frames * nctu
        return {"value": n / dt, "unit": "CTU/s", "cores": threads, "kind": "port", "scope": "S1 memory -> memory", "name": label, "host": host,
                "sample": "%d pass(es) over %d frame(s) of %dx%d (%d CTUs), oracle/ethcnn_oracle.c canonical mode, OpenMP over the "
                          "CTUs of a frame group, %.1f s" % (reps, frames, W, H, n, dt)}

    if not full:  # N > 1 lines: the all-cores oracle on a shorter sample only (rank 0; the other ranks are idle meanwhile)
        out.append(timed_passes(min(NF, 10), target_seconds, "B1 oracle, all usable host cores", cores))
        return out
    out.append(timed_passes(NF, budget["all"], "B1 oracle, all usable host cores", cores))
    # one thread: ~0.5 k CTU/s -> one frame is seconds of work; never more than one frame, one pass
    one = timed_passes(1, 0.0, "B1 oracle, 1 thread", 1)
    out.append(one)
    oracle.set_threads(cores)
    # S3, oracle: read the file, predict, write cu_depth.dat (the reference's 'Predicting Time' scope)
    dat = os.path.join(yuv.dir, "cpu_cu_depth.dat")
    reps, t0 = 0, time.perf_counter()
    while reps == 0 or time.perf_counter() - t0 < budget["s3"]:
        buf = np.fromfile(yuv.path, dtype=np.uint8)
        P = oracle.predict_frames(blob, buf, W, H, NF, QP, 0.5, 0.5, mode=0, frame_stride=W * H * 3 // 2)
        P.tofile(dat)
        reps += 1
    dt = time.perf_counter() - t0
    out.append({"value": reps * NF * nctu / dt, "unit": "CTU/s", "cores": cores, "kind": "port", "name": "B1 oracle, all usable host cores, file scope", "host": host,
                "scope": "S3 4:2:0 file -> cu_depth.dat (video_to_cu_depth.py:142-145)",
                "sample": "%d pass(es) over the %d-frame %dx%d file on tmpfs, %.1f s" % (reps, NF, W, H, dt)})
    try:
        import tf_cpu_proxy as proxy
        import torch
        pt = min(cores, 64)  # more does not help ops this small; the count used is reported
        proxy.predict_file(blob, yuv.path, W, H, QP, dat, max_frames=1, threads=pt)  # warm
        frames, ctus, dt = proxy.predict_file(blob, yuv.path, W, H, QP, dat, max_seconds=budget["proxy"], threads=pt)
        out.append({"value": ctus / dt, "unit": "CTU/s", "cores": pt, "kind": "port", "name": "B2 TF-CPU proxy (torch-CPU ops, reference-shaped driver)", "host": host,
                    "scope": "S3 4:2:0 file -> cu_depth.dat (video_to_cu_depth.py:142-145)",
                    "sample": "first %d frame(s) of the %dx%d file (%d CTUs): per-CTU Python tiling loop, <=1024-CTU feeds, torch %s CPU, "
                              "%d threads, %.1f s" % (frames, W, H, ctus, torch.__version__, pt, dt)})
    except Exception as exc:  # a baseline is a side measurement: never fatal
        out.append({"name": "B2 TF-CPU proxy", "error": str(exc)})
    return out


if __name__ == "__main__":
    sys.exit(main())
