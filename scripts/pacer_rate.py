"""What pacing one frame costs on one MI355X -> profiles/pacer_rate.json (method: scripts/budget_rate.py).  A record, not a gate.

  pacer    ethcnn_pacer_frame on a page-locked buffer, in place (what the Low-Delay-P daemons call), default ladder (513 rungs + the full
           search), at 416x240, 1920x1080 and 3840x2160.  After a warm-up, LAUNCHES synchronous calls in one window, best of three.
  offline  the only per-frame route without a pacer, in the same job: ethcnn_sim_reset + ethcnn_sim_add_frames of the one frame +
           ethcnn_budget_control, from and to pageable memory, which is all those entries take.  The ratio is the finding.
  check    the pacer's baked rows and rung of the last frame against that route's
  daemon   the native daemon's frame time from the encoder's side (tools/ldp_client.c, its "handshake p50" line) at 1920x1080 with
           and without ETHCNN_SEARCH_BUDGET=0.4, seeded synthetic weights; skipped with --no-daemon or when the binaries are not built

    python scripts/pacer_rate.py [--out profiles/pacer_rate.json] [--quick] [--no-daemon]
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from decide_rate import window  # noqa: E402

SIZES = ((416, 240), (1920, 1080), (3840, 2160))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")


def daemon_p50(budget, frames):
    """-> the client's report line for `frames` 1920x1080 frames served by the native daemon, under a budget or without"""
    with tempfile.TemporaryDirectory() as work:
        open(os.path.join(work, "Thr_info.txt"), "w").write("0.25 0.75 0.25 0.75 0.25 0.75\n")
        env = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
        env.update(ETHCNN_SYNTHETIC_SEED="21", ETHCNN_HEAD_GAIN="8.0")
        if budget is not None:
            env["ETHCNN_SEARCH_BUDGET"] = str(budget)
        d = subprocess.Popen([os.path.join(BIN, "resi_to_cu_depth_ldp"), "--max-frames", str(frames), "--idle-timeout", "60", "--quiet"], cwd=work, env=env,
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        c = subprocess.run([os.path.join(BIN, "ldp_client"), work, "1920", "1080", "32", str(frames), "--seed", "7", "--gap-us", "2000"], capture_output=True,
                           text=True, timeout=600)
        rc = d.wait(timeout=120)
        line = next((ln for ln in c.stdout.splitlines() if "handshake p50" in ln), "")
        m = re.search(r"handshake p50\s+([0-9.]+)", line)
        return dict(budget=budget, frames=frames, client_status=c.returncode, daemon_status=rc, client_report=line.strip(),
                    handshake_p50_us=float(m.group(1)) if m else None, daemon_summary=d.stderr.read().strip()[-300:])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pacer_rate.json"))
    ap.add_argument("--quick", action="store_true", help="3 launches a window (a functional check, not a measurement)")
    ap.add_argument("--no-daemon", action="store_true")
    a = ap.parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    launches = 3 if a.quick else 200
    rng = np.random.default_rng(1)
    res = {"rungs": pkg.ethcnn.BUDGET_DEFAULT_RUNGS, "budget": 0.4, "mode": "carry", "sizes": []}
    same = True
    with pkg.EthCnn(device=0) as ctx:
        res["device"] = ctx.device_name
        for w, h in SIZES:
            nctu = pkg.ethcnn.ctus_per_frame(w, h)
            probs = (rng.integers(0, 1025, size=(nctu, 21)) / 1024.0).astype(np.float32)
            pinned = ctx.host_buffer(nctu * 84).view(np.float32).reshape(nctu, 21)
            with pkg.Pacer(ctx, 0.4, "carry") as pacer, pkg.PartitionSim(ctx) as sim:
                def paced():
                    pinned[:] = probs   # (the daemon's step writes them there; the copy is inside both windows' loops alike: see offline)
                    return pacer.frame(pinned, w, h, out=pinned)

                def offline():
                    pinned[:] = probs
                    sim.reset()
                    sim.add_frames(pinned, None, w, h)
                    return sim.budget_control(0.4, "carry", width=w, height=h, nframes=1)

                t_pacer = window(ctx, paced, launches)
                t_off = window(ctx, offline, launches)
                pacer.reset()
                baked, r = paced()
                want = offline()
                ok = bool(baked.tobytes() == want["probs"].tobytes() and int(r["rung"]) == int(want["rung"][0]))
                same = same and ok
            res["sizes"].append(dict(width=w, height=h, ctus=nctu, launches_per_window=launches, windows=3, pacer_frame_seconds=t_pacer,
                                     reset_add_control_seconds=t_off, pacer_over_offline=t_pacer / t_off, identical=ok,
                                     window="synchronous calls in one window, best of three; both loops refill the %d-byte buffer first" % (nctu * 84)))
            ctx.free_host_buffers()
    if not a.no_daemon and all(os.path.exists(os.path.join(BIN, n)) for n in ("resi_to_cu_depth_ldp", "ldp_client")):
        frames = 20 if a.quick else 300
        res["daemon_1920x1080"] = [daemon_p50(None, frames), daemon_p50(0.4, frames)]
    res["identical"] = same
    res["not_measured"] = ["ethcnn_pacer_frame_device queued back to back", "pageable (staged) pointers", "the Python daemon", "other GPUs of the pool",
                           "any relation of the weighted check count to encoding time or BD-rate"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("a paced frame disagrees with reset + add_frames + budget_control")
    return 0


if __name__ == "__main__":
    sys.exit(main())
