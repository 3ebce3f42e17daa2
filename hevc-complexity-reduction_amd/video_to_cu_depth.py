"""Host mirror of the reference's predictor driver
(/root/reference/HM-16.5_Test_AI/bin/video_to_cu_depth.py): same command line, same files,
same exit-status contract, so the unchanged HM hook
(TAppEncCfg.cpp:2317-2321: system("python video_to_cu_depth.py <yuv> <w> <h> <qp>"))
drives it.  Everything below the argument handling happens in libethcnn.so.

Differences from the reference, all outside the numbers it produces:
  * cu_depth.dat is written to a temp file and renamed (never a partial file);
  * the YUV is streamed (luma only) instead of being tiled in Python;
  * when the trained checkpoint blobs are absent (they are not in the reference repo),
    ETHCNN_SYNTHETIC_SEED=<n> [ETHCNN_HEAD_GAIN=<g>] opts into seeded synthetic weights;
    without it a missing checkpoint is an error (non-zero exit, HM aborts);
  * HM's command line is fixed, so the source format of the file comes through the environment: ETHCNN_INPUT_BIT_DEPTH=8..16 (HM's
    InputBitDepth; above 8 the file holds 16-bit samples) and ETHCNN_INPUT_CHROMA_FORMAT=400|420|422|444 (InputChromaFormat).  Unset:
    the reference's 8-bit 4:2:0.  A bad value is a non-zero exit with a message.
  * ETHCNN_SEARCH_BUDGET=<share, 0..1> holds every frame's pruned search under that share of the full search's weighted checks
    (include/ethcnn.h "search budget"): the launcher predicts with open gates, picks a rung of the default ladder (or of the ladder
    file ETHCNN_SEARCH_BUDGET_LADDER, in All-Intra token order: tools/build_ladder.py --out FILE --order ai) per frame and
    writes a BAKED cu_depth.dat (values 0, 0.5, 1).  HM reads Thr_info.txt afterwards, so the launcher refuses (exit status 1, no
    cu_depth.dat) unless that file is the companion line "0.75 0.25 0.75 0.25 0.75 0.25".  ETHCNN_SEARCH_BUDGET_MODE=frame|carry
    (default frame) and ETHCNN_SEARCH_BUDGET_WEIGHTS="64 16 4 1" are optional.  One GPU only: ETHCNN_DEVICES with a budget is refused.
    ETHCNN_SEARCH_BUDGET_LADDER=auto builds the ladder from THIS file's open-gate predictions, without labels: the walk of
    tools/build_ladder.py --no-labels (include/ethcnn.h "partition-search simulation: expected wrong decisions") on grid 8, up to
    4096 rungs, no cap, under the run's weights.  ETHCNN_SEARCH_BUDGET_RELIABILITY=<table of calibrate_thresholds.py --reliability-out>
    is optional (default: the identity table); an unreadable one is refused at start-up (exit status 1, nothing written).
  * ETHCNN_FC1_PLAN_AUDIT=<N> (read only when ETHCNN_FC1_PLAN is set and the guard accepted the plan) audits the plan on min(N, frames)
    evenly spaced frames of THIS file before it is trusted (include/ethcnn.h "comparing two predictions"): plan against exact plan at
    the run's QP, open gates, Thr_info.txt as the candidate, with the single-launch pass off (the audited frames take the 16-bit path that
    the run over the whole file takes).  One line with the numbers goes to stderr; anything over 1e-4, or an audit that fails, and the
    run continues with the exact plan, as after a guard refusal.  A malformed value, or a source that is not 8-bit 4:2:0, is refused at
    start-up (exit status 1, nothing written).
"""
from __future__ import print_function

import os
import re
import sys
import time

from . import ethcnn as _e
from . import net_CNN as nt
from . import search_budget as _sb

NUM_CHANNELS = nt.NUM_CHANNELS
NUM_EXT_FEATURES = nt.NUM_EXT_FEATURES
NUM_LABEL_BYTES = nt.NUM_LABEL_BYTES
IMAGE_SIZE = nt.IMAGE_SIZE
SAVE_FILE = 'cu_depth.dat'   # video_to_cu_depth.py:20
THR_FILE = 'Thr_info.txt'    # net_CNN.py:47


def get_file_size(path):
    return os.path.getsize(path)


def get_y_conv_on_large_data(ctx, input_image, qp_seq):
    """video_to_cu_depth.py:61-73: [n,64,64,1] -> [n,21], gates per <=1024-CTU sub-batch."""
    return ctx.predict_ctus(input_image, qp_seq)


def source_format_from_env():
    """(bit_depth, chroma) from ETHCNN_INPUT_BIT_DEPTH / ETHCNN_INPUT_CHROMA_FORMAT; ValueError names a bad value"""
    fmt = []
    for name, default, ok in (('ETHCNN_INPUT_BIT_DEPTH', 8, range(8, 17)), ('ETHCNN_INPUT_CHROMA_FORMAT', 420, (400, 420, 422, 444))):
        text = os.environ.get(name)
        if text is None or text == '':
            fmt.append(default)
            continue
        try:
            value = int(text)
        except ValueError:
            value = None
        if value not in ok:
            raise ValueError("%s='%s' (allowed: %s)" % (name, text, ', '.join(str(v) for v in ok)))
        fmt.append(value)
    return tuple(fmt)


COMPANION_LINE = _sb.COMPANION_LINE_AI   # ethcnn_budget_companion_thr in All-Intra token order


def search_budget_from_env():
    """None when ETHCNN_SEARCH_BUDGET is unset or empty, else (share, mode, weights or None); ValueError names a bad value"""
    budget = _sb.from_env()
    if budget is not None and os.environ.get('ETHCNN_DEVICES'):
        raise ValueError('ETHCNN_SEARCH_BUDGET runs on one GPU: unset ETHCNN_DEVICES (ETHCNN_DEVICE picks the GPU)')
    return budget


def check_companion_thr_file(path=THR_FILE):
    """A baked cu_depth.dat means what it says only under the companion thresholds, and HM reads them from this file after the
    launcher has run: ValueError unless it holds exactly that line's six values"""
    _sb.check_companion_thr_file(path, COMPANION_LINE)


def search_ladder_from_env():
    """None (the default ladder) when ETHCNN_SEARCH_BUDGET_LADDER is unset or empty, else that ladder file read in All-Intra token order
    -> (up_k, down_k); "auto" -> (AUTO, reliability table or None): the ladder is built from the file's own predictions; ValueError
    names a bad file"""
    ladder = _sb.ladder_from_env('ai', auto=True)
    if ladder == _sb.AUTO:
        return _sb.AUTO, _sb.reliability_from_env(_e.risk_read)
    return ladder


def write_budgeted(ctx, yuv_name, qp_seq, frame_width, frame_height, budget, save_file, ladder=None):
    """budget mode: every frame of the file predicted with open gates, one rung of the ladder (None: the default one) picked per frame
    under the budget, the picked decisions baked into save_file (temp file + rename).  -> (frames, achieved share, over-budget frames)"""
    import numpy as np
    share, mode, weights = budget
    auto = ladder is not None and ladder[0] == _sb.AUTO
    if ladder is not None and not auto:
        ladder = _e.sim_thr(*ladder)
    tmp = '%s.tmp.%d' % (save_file, os.getpid())
    try:
        ctx.set_thresholds(0.0, 0.0)    # open gates, whatever Thr_info.txt says: the baked file is what the encoder reads
        n_frames = ctx.predict_yuv_file(yuv_name, frame_width, frame_height, qp_seq, tmp)
        probs = np.fromfile(tmp, dtype='<f4')
        with _e.PartitionSim(ctx) as sim:
            sim.add_frames(probs, None, frame_width, frame_height, nframes=n_frames)
            if auto:   # the ladder of this very sequence: no labels exist before the encode
                sim.set_reliability(ladder[1])
                ladder = sim.build_ladder_risk(weights, _sb.AUTO_GRID, _sb.MAX_RUNGS)['thr']
                sys.stderr.write('video_to_cu_depth: ladder of %d rungs built from the predictions of %d frames\n' % (len(ladder), n_frames))
            out = sim.budget_control(share, mode, ladder=ladder, weights=weights, width=frame_width, height=frame_height, nframes=n_frames)
        out['probs'].astype('<f4').tofile(tmp)
        os.replace(tmp, save_file)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    cost, full = sum(int(x) for x in out['cost']), sum(int(x) for x in out['full'])
    return n_frames, (float(cost) / full if full else 0.0), int(out['over'].sum())


def get_prob(ctx, yuv_name, image_size, save_file, qp_seq, n_frames_start, n_frames_end, frame_width, frame_height):
    """video_to_cu_depth.py:75-118: frames [n_frames_start, n_frames_end) of the file -> save_file (which then holds exactly
    those frames; the reference reads and discards the first n_frames_start, :86-87).  Its own call passes 0 and the frame
    count (:139-140)."""
    assert image_size == IMAGE_SIZE
    frame_bytes = _e.source_frame_bytes(frame_width, frame_height, *ctx.source_format())[1]   # width * height * 3 // 2 by default
    total = get_file_size(yuv_name) // frame_bytes
    if n_frames_start == 0 and n_frames_end == total:
        return ctx.predict_yuv_file(yuv_name, frame_width, frame_height, qp_seq, save_file)
    if not 0 <= n_frames_start <= n_frames_end <= total:
        raise ValueError("get_prob: frame range [%d, %d) outside the file's %d frames" % (n_frames_start, n_frames_end, total))
    return ctx.predict_yuv_range(yuv_name, frame_width, frame_height, qp_seq, save_file, n_frames_start, n_frames_end)


def restore_model(ctx, qp_seq, model_dir='.'):
    """video_to_cu_depth.py:126-133: QP band -> checkpoint prefix -> saver.restore."""
    prefix = os.path.join(model_dir, _e.model_name_for_qp(qp_seq))
    seed = os.environ.get('ETHCNN_SYNTHETIC_SEED')
    if os.path.exists(prefix + '.data-00000-of-00001') or seed is None:
        ctx.load_checkpoint(prefix)
        return prefix
    ctx.load_synthetic(int(seed), float(os.environ.get('ETHCNN_HEAD_GAIN', '1.0')))
    return 'synthetic(seed=%s)' % seed


AUDIT_TOL = 1e-4   # the plans' contract: within 1e-4 of the exact plan


def plan_audit_from_env(fmt=(8, 420)):
    """frames to audit: 0 unless ETHCNN_FC1_PLAN and ETHCNN_FC1_PLAN_AUDIT are both set; ValueError names a malformed value"""
    text = os.environ.get('ETHCNN_FC1_PLAN_AUDIT')
    if not os.environ.get('ETHCNN_FC1_PLAN') or text is None or text == '':
        return 0
    if not re.match(r'^[0-9]{1,6}$', text) or text.endswith('\n'):   # no sign, no blank: the native launcher's rule
        raise ValueError("ETHCNN_FC1_PLAN_AUDIT='%s' (a number of frames of one to six digits, 0 = no audit)" % text)
    if int(text) and tuple(fmt) != (8, 420):
        raise ValueError('ETHCNN_FC1_PLAN_AUDIT reads 8-bit 4:2:0 files only (the audit of other sources is not built)')
    if int(text) and ',' in os.environ.get('ETHCNN_DEVICES', ''):
        raise ValueError('ETHCNN_FC1_PLAN_AUDIT runs on one GPU: unset ETHCNN_DEVICES (ETHCNN_DEVICE picks the GPU)')
    return int(text)


def audit_fast_plan(ctx, yuv_file, width, height, qp_seq, n_audit):
    """the accepted plan against the exact plan on min(n_audit, frames) evenly spaced frames of the file itself; one line on stderr;
    anything over AUDIT_TOL, or an audit that fails: the run continues with the exact plan, as after a refusal"""
    plan = ctx.fc1_plan()
    frames = get_file_size(yuv_file) // (width * height * 3 // 2)
    count = min(int(n_audit), frames)
    if not plan or count <= 0:
        return
    try:
        thr = _e.read_thr_info_k(THR_FILE, 'ai')
    except ValueError:
        thr = None   # (values off the simulator's ranges: the differences are still measured, the search is not compared)
    step = frames // count
    # with the single-launch pass off: a few frames would run as that pass, which computes exactly under every plan, while the run over the
    # whole file takes the 16-bit path; the audit must take the path it audits
    ctx.set_small_pass_launch(False)
    try:
        r = ctx.audit_plan_yuv_file(yuv_file, width, height, qp_seq, plan, 0, step, count, AUDIT_TOL, thr)
    except _e.EthCnnError as err:   # an audit that cannot run (memory, a read error) is no reason to fail the encode
        sys.stderr.write('video_to_cu_depth: plan %d audit failed: %s\nvideo_to_cu_depth: continuing with the exact plan (0)\n' % (plan, err))
        ctx.set_fc1_plan(0)
        return
    finally:
        ctx.set_small_pass_launch(True)
    over = sum(r['over_tol'])
    if r['fast_passes'] == 0:
        verdict = 'these frames run as single-launch passes, which compute exactly under every plan: nothing to audit, plan kept'
    else:
        verdict = 'continuing with the exact plan (0)' if over else 'plan kept'
    sys.stderr.write('video_to_cu_depth: plan %d audit over %d frames (step %d): max |dp| %s, values over %g: %d, classes that differ: %s, '
                     'CTUs whose search differs: %s, fast passes %d/%d: %s\n'
                     % (plan, count, step, ' '.join('%.3g' % v for v in r['max_abs']), AUDIT_TOL, over,
                        sum(r['class_diff']) if thr else 'n/a', r['search_diff_ctus'] if thr else 'n/a', r['fast_passes'], r['passes'], verdict))
    if over:
        ctx.set_fc1_plan(0)


def guard_fast_plan(ctx):
    """ETHCNN_FC1_PLAN=2|3 is an opt-in; the encoder asserts a zero exit status (TAppEncCfg.cpp:2321).  The library REFUSES a plan
    whose load-time accuracy guard fails for the restored checkpoint (include/ethcnn.h, ethcnn_check_fc1_plan); the launcher then says
    so on stderr and runs the exact plan -- always correct, only slower -- instead of failing the encode."""
    plan = ctx.fc1_plan()
    if plan:
        g = ctx.check_fc1_plan(plan)
        if not g['accepted']:
            sys.stderr.write('video_to_cu_depth: %s\nvideo_to_cu_depth: continuing with the exact plan (0)\n' % g['message'])
            ctx.set_fc1_plan(0)


def _shard_worker(device, yuv_file, width, height, qp_seq, out_path, f0, f1, thr, nworkers=1, fmt=(8, 420)):
    """One process per GPU: own context, own frame range, pwrite into out_path.
    The node's host-CPU budget is shared: every worker starts budget / nworkers staging-fill threads
    (ethcnn_host_thread_budget), not a full pool each."""
    os.environ['ETHCNN_LOCAL_WORKERS'] = str(max(1, int(nworkers)))
    ctx = _e.EthCnn(device=device)
    ctx.set_thresholds(*thr)
    ctx.set_source_format(*fmt)
    restore_model(ctx, qp_seq)
    guard_fast_plan(ctx)
    ctx.predict_yuv_shard(yuv_file, width, height, qp_seq, out_path, f0, f1)
    ctx.close()


def predict_sharded(yuv_file, width, height, qp_seq, save_file, devices, fmt=(8, 420)):
    """Frame-range sharding over `devices` (list of HIP ordinals).  No collective: ranges are disjoint and the output offsets
    deterministic.  Default: ONE process, a worker thread per device inside the library (ethcnn_predict_yuv_file_sharded: one
    interpreter, one checkpoint parse, peers cloned from the first context -- the encoder blocks on this command, TAppEncCfg.cpp:2317-2321).
    ETHCNN_SHARD_PROCESSES=1: a worker PROCESS per device (the form the torchrun bench uses), each with its own context."""
    if os.environ.get('ETHCNN_SHARD_PROCESSES', '0') in ('', '0'):
        ctx = _e.EthCnn(device=devices[0])
        ctx.load_thresholds(THR_FILE)
        ctx.set_source_format(*fmt)
        restore_model(ctx, qp_seq)
        guard_fast_plan(ctx)
        n = ctx.predict_yuv_file_sharded(devices, yuv_file, width, height, qp_seq, save_file)
        ctx.close()
        return n
    import multiprocessing as mp
    from . import sharding
    n_frames = get_file_size(yuv_file) // _e.source_frame_bytes(width, height, *fmt)[1]
    thr = nt.get_thresholds(THR_FILE)
    tmp = '%s.tmp.%d' % (save_file, os.getpid())
    sharding.presize_output(tmp, n_frames, width, height)
    mpctx = mp.get_context('spawn')
    procs = []
    ranges = [(dev,) + sharding.frame_range(n_frames, len(devices), g) for g, dev in enumerate(devices)]
    ranges = [r for r in ranges if r[2] > r[1]]
    for dev, f0, f1 in ranges:
        p = mpctx.Process(target=_shard_worker, args=(dev, yuv_file, width, height, qp_seq, tmp, f0, f1, thr, len(ranges), fmt))
        p.start()
        procs.append(p)
    ok = True
    for p in procs:
        p.join()
        ok = ok and p.exitcode == 0
    if not ok:
        os.remove(tmp)
        raise RuntimeError('a shard worker failed')
    os.replace(tmp, save_file)
    return n_frames


def main(argv=None):
    argv = sys.argv if argv is None else argv
    assert len(argv) == 5                      # :120
    yuv_file = argv[1]
    width, height, qp_seq = int(argv[2]), int(argv[3]), int(argv[4])
    try:
        fmt = source_format_from_env()
        frame_bytes = _e.source_frame_bytes(width, height, *fmt)[1]         # :136 width * height * 3 // 2 unless the environment says otherwise
        budget = search_budget_from_env()
        n_audit = plan_audit_from_env(fmt)
        ladder = None
        if budget is not None:
            ladder = search_ladder_from_env()
            check_companion_thr_file()
    except (ValueError, _e.EthCnnError) as err:
        sys.stderr.write('video_to_cu_depth: %s\n' % err)
        return 1
    assert frame_bytes > 0 and get_file_size(yuv_file) % frame_bytes == 0   # :137
    # ETHCNN_DEVICES="0,1,2,3" shards frames over several GPUs; default: one GPU (ETHCNN_DEVICE)
    devices = [int(d) for d in os.environ.get('ETHCNN_DEVICES', os.environ.get('ETHCNN_DEVICE', '0')).split(',')]
    timing = os.environ.get('ETHCNN_TIMING', '0') not in ('', '0')
    stamps = [('imports done', time.perf_counter())]
    t1 = time.time()
    if len(devices) > 1:
        n_frames = predict_sharded(yuv_file, width, height, qp_seq, SAVE_FILE, devices, fmt)
        stamps.append(('create + weights + predict (%d workers)' % len(devices), time.perf_counter()))
    else:
        ctx = _e.EthCnn(device=devices[0])
        stamps.append(('create (HIP runtime init %.1f, whole call %.1f)' % ctx.startup_times(), time.perf_counter()))
        ctx.load_thresholds(THR_FILE)          # net_CNN.py:47 (cwd-relative; at import time there)
        ctx.set_source_format(*fmt)
        restore_model(ctx, qp_seq)
        guard_fast_plan(ctx)
        if n_audit:
            audit_fast_plan(ctx, yuv_file, width, height, qp_seq, n_audit)
        stamps.append(('thresholds + weights + plan guard', time.perf_counter()))
        t1 = time.time()                       # the reference times get_prob only (:142-145)
        if budget is not None:
            n_frames, share, over = write_budgeted(ctx, yuv_file, qp_seq, width, height, budget, SAVE_FILE, ladder)
            sys.stderr.write('video_to_cu_depth: search budget %g (%s): %.6f of the full search over %d frames, %d over budget\n'
                             % (budget[0], budget[1], share, n_frames, over))
        else:
            n_frames = get_prob(ctx, yuv_file, IMAGE_SIZE, SAVE_FILE, qp_seq, 0,
                                get_file_size(yuv_file) // frame_bytes, width, height)
        stamps.append(('predict', time.perf_counter()))
        ctx.close()
        stamps.append(('destroy', time.perf_counter()))
    t2 = time.time()
    if timing:  # (perf_counter is CLOCK_MONOTONIC: comparable with the spawning process's stamp, ETHCNN_T0_MS)
        t0 = float(os.environ.get('ETHCNN_T0_MS', '0')) * 1e-3
        up = float(os.environ.get('ETHCNN_T_UP_MS', '0')) * 1e-3
        prev, parts = (up or stamps[0][1]), []
        if t0 and up:
            parts.append('spawn -> interpreter up %.1f' % ((up - t0) * 1e3))
        for name, t in stamps:
            parts.append('%s %.1f' % (name, (t - prev) * 1e3))
            prev = t
        sys.stderr.write('video_to_cu_depth.py timing (ms): ' + ' | '.join(parts) + '\n')
    print('%s  frame %d/%d  %dx%d' % (yuv_file, n_frames, n_frames, width, height))
    print('--------\n\nPredicting Time: %.3f sec.\n\n--------' % float(t2 - t1))  # :145
    return 0
