"""Offline Low-Delay-P predictor: a whole residual sequence -> cu_depth.dat, the LDP counterpart of video_to_cu_depth.py.

    resi_video_to_cu_depth_LDP.py <resi.yuv> <width> <height> <qp> [--first-frame 1] [--frames N] [--out cu_depth.dat]
                                  [--state-out state.dat] [--model-dir DIR] [--device 0] [--chunk FRAMES]

<resi.yuv> is the whole-sequence 4:2:0 residual file HM-16.5_Resi_Pre writes per QP: frame k of the file is POC k.  POC 0 is the intra
picture and has no residual, so the first frame is 1 unless a later one is asked for (--first-frame > 1 needs the state of the frames
before it and is meant for library users; from the command line it fails unless the frames before were predicted by the same process).
The output holds float32 [frames][ctus][21] for frames [first, first + N): what the per-frame daemon (resi_to_cu_depth_LDP.py) writes
frame after frame when it carries its state through the sequence, bit for bit.  Models are restored exactly as the daemon restores
them: model_LDP_2000000_qp22~37.dat and the model_LDP_200000_qpXX.dat of the QP band from --model-dir (default: the directory of
this command's caller, '.'); ETHCNN_SYNTHETIC_SEED / ETHCNN_HEAD_GAIN select seeded weights where a checkpoint is missing.
Score the result with tools/score_cu_depth.py --skip-label-frames <first>.
"""
import argparse
import os
import sys
import time

import numpy as np

if __package__:
    from . import ethcnn as _e
    from .resi_to_cu_depth_LDP import restore_cnn, restore_lstm
else:  # run as a file: the package directory's name is no Python identifier, so it is imported by name from the repository root
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
    _e = importlib.import_module("hevc-complexity-reduction_amd.ethcnn")
    _d = importlib.import_module("hevc-complexity-reduction_amd.resi_to_cu_depth_LDP")
    restore_cnn, restore_lstm = _d.restore_cnn, _d.restore_lstm


def _fail(msg):
    sys.stderr.write("resi_video_to_cu_depth_LDP: %s\n" % msg)
    return 1


def main(argv):
    ap = argparse.ArgumentParser(prog="resi_video_to_cu_depth_LDP.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("yuv")
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("qp", type=int)
    ap.add_argument("--first-frame", type=int, default=1)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--out", default="cu_depth.dat")
    ap.add_argument("--state-out", default=None)
    ap.add_argument("--model-dir", default=".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0)
    try:
        a = ap.parse_args(argv[1:])
    except SystemExit as e:
        return int(e.code or 0)
    # everything that can be refused without a GPU is refused before one is opened
    if a.width <= 0 or a.height <= 0:
        return _fail("bad frame size %dx%d" % (a.width, a.height))
    if not os.path.isfile(a.yuv):
        return _fail("cannot read %s" % a.yuv)
    frame_bytes = a.width * a.height * 3 // 2
    size = os.path.getsize(a.yuv)
    if frame_bytes == 0 or size % frame_bytes != 0:
        return _fail("%s: size %d is not a multiple of the %dx%d 4:2:0 frame size %d" % (a.yuv, size, a.width, a.height, frame_bytes))
    total = size // frame_bytes
    if a.first_frame < 1:
        return _fail("--first-frame %d: frame 0 is the intra picture (POC 0) and has no residual; the first residual frame is 1" % a.first_frame)
    nframes = total - a.first_frame if a.frames is None else a.frames
    if nframes <= 0 or a.first_frame + nframes > total:
        return _fail("frames [%d, %d) lie outside the %d frames of %s" % (a.first_frame, a.first_frame + nframes, total, a.yuv))
    if a.chunk < 0:
        return _fail("--chunk %d" % a.chunk)
    try:
        ctx = _e.EthCnn(device=a.device)
        try:
            print("CNN  model: %s" % restore_cnn(ctx, a.model_dir))
            print("LSTM model: %s" % restore_lstm(ctx, a.qp, a.model_dir))
            thr = os.path.join(a.model_dir, "Thr_info.txt")
            if os.path.exists(thr):
                ctx.load_thresholds(thr)
            ctx.ldp_set_sequence_chunk(a.chunk)
            t0 = time.time()
            ctx.ldp_predict_yuv_file(a.yuv, a.width, a.height, a.qp, a.out, a.first_frame, a.first_frame + nframes)
            dt = time.time() - t0
            print("Predicting Time: %.3f sec. (%d frames, %d CTUs each)" % (dt, nframes, _e.ctus_per_frame(a.width, a.height)))
            if a.state_out:
                state = ctx.ldp_get_state(a.width, a.height)
                tmp = "%s.tmp.%d" % (a.state_out, os.getpid())
                np.ascontiguousarray(state, dtype="<f4").tofile(tmp)
                os.replace(tmp, a.state_out)
        finally:
            ctx.close()
    except (_e.EthCnnError, OSError, ValueError) as e:
        return _fail(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
