"""Train ETH-CNN (All-Intra) on the GPU: the driver of ETH-CNN_Training_AI/train_CNN_CTU64.py:316-399, with
command-line flags in place of its module constants.  Every step runs in the library's training kernels (Trainer,
include/ethcnn.h "training"); this file only schedules, evaluates, logs and saves.

    python train_CNN_CTU64.py --train AI_Train_2446725.dat_shuffled --valid AI_Valid_143925.dat_shuffled --model-type 3
    python train_CNN_CTU64.py ... --iters 1000000 --export-ai .   # also writes model_2000000_qp30~35.dat for video_to_cu_depth.py
    python train_CNN_CTU64.py --train ... --valid ... --model-types 1,2,3,4 --export-ai .   # the four models of a deployment at once

--model-types: the listed models train as one group (TrainerGroup, include/ethcnn.h "training, several models at once") from one
copy of the two sample sets, every step of all of them in the same launches; each model's weights, log and files are those of its
own --model-type run with the same arguments, and go to <models>/<name>/ (qp22 .. qp37).

Sample files: the reference's Extract_Data output (4992-byte records), uploaded once into HBM.  Like the reference it evaluates
every 1000 steps on 5000 random samples of each set (no dropout), appends to Models/loss_accuracy_list.dat (first line: total
iterations, then 19 columns per evaluation, CRLF), saves Models/model_<time>_<step>_<name>.dat every 50000 steps and
Models/model.dat at the end.  --reload resumes from Models/model.dat and that log.  Resume choice: the reference's Saver keeps only
the 36 trainable variables (train_CNN_CTU64.py:293), so its momentum accumulators restart at zero on reload; this driver does the
same (the library can resume them exactly, ethcnn_train_set_blob with accumulators, but the checkpoint format has no place for them).
Plotting is not ported.
"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tools"))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import sequence_table  # noqa: E402

REC = 4992
# input_data.py:39-55: MODEL_TYPE -> (MODEL_NAME, SELECT_QP_LIST)
MODEL_TYPES = {1: ("qp22", [22]), 2: ("qp27", [27]), 3: ("qp32", [32]), 4: ("qp37", [37])}
ITER_TIMES_PER_EVALUATE, ITER_TIMES_PER_SAVE, ITER_TIMES_PER_PRINT = 1000, 50000, 100
NUM_EVAL = 5000


def get_time_str():
    return time.strftime("%Y%m%d_%H%M%S", time.localtime(time.time()))


def get_tendency_2x2(m):  # train_CNN_CTU64.py:140-148
    if m[0][1] == 0 and m[1][0] == 0:
        return 0
    elif m[0][1] == 0 or m[1][1] == 0:
        return -100
    elif m[1][0] == 0 or m[0][0] == 0:
        return 100
    return -math.log10((m[0][0] / m[0][1]) / (m[1][1] / m[1][0]))


def load_records(path, rec=REC):
    data = np.memmap(path, dtype=np.uint8, mode="r")
    if data.size == 0 or data.size % rec:
        raise SystemExit("%s: %d bytes is not a whole number of %d-byte samples" % (path, data.size, rec))
    return data


def train_loop(a, pkg, tr, name, ntrain, nvalid, evaluate, export=None, num_eval=NUM_EVAL, save_every=ITER_TIMES_PER_SAVE, ckpt_io=None):
    """train_CNN_CTU64.py:296-399 (shared with train_resi_CNN_CTU64.py and train_LSTM_CTU64.py): reload, evaluate every 1000 steps
    (evaluate(which, idx) -> loss list, accuracy list, probabilities, labels of one batch), the log, periodic and final checkpoints,
    the optional export.  num_eval / save_every / ckpt_io = (read, write): the LSTM driver's 10000 samples, 10000 steps and
    18-tensor bundle; the defaults are the CNN drivers'."""
    import score_cu_depth
    read_ckpt, write_ckpt = ckpt_io or (pkg.ethcnn.read_ckpt_blob, pkg.ethcnn.write_ckpt_blob)
    log = os.path.join(a.models, "loss_accuracy_list.dat")
    rows = []
    if a.reload:
        tr.set_blob(read_ckpt(os.path.join(a.models, "model.dat")))  # accumulators: zeros, as the reference's restore
        with open(log) as f:
            iter_times_last = int(f.readline())
            rows = [ln.rstrip("\r\n") for ln in f if ln.strip()]
    else:
        tr.init_weights(a.seed)
        iter_times_last = 0
    print("iter_times_last = %d" % iter_times_last)
    eval_rng = np.random.default_rng(a.seed + iter_times_last + 1)

    def evaluate_loss_accuracy(step, lr):  # train_CNN_CTU64.py:213-250
        out = []
        for which, n in ((pkg.ethcnn.SET_TRAIN, ntrain), (pkg.ethcnn.SET_VALID, nvalid)):
            idx = eval_rng.integers(0, n, min(num_eval, n))
            l3, a3, probs, labels = evaluate(which, idx)
            ms = score_cu_depth.class_matrices(labels, probs)
            out.append((l3, a3, [get_tendency_2x2(m) for m in ms]))
        (tl, ta, tt), (vl, va, vt) = out
        print("%s step %d: loss=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], accu=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], lr=%g"
              % ((get_time_str(), step) + tuple(tl) + tuple(vl) + tuple(ta) + tuple(va) + (lr,)))
        print("tendency = [[%.3f, %.3f, %.3f] [%.3f, %.3f, %.3f]]" % (tuple(tt) + tuple(vt)))
        rows.append("%d  " % step + "  ".join("%g" % v for v in list(tl) + list(vl) + list(ta) + list(va) + list(tt) + list(vt)))

    def lr_at(step):
        return a.lr * a.decay_rate ** (step // a.decay_steps)

    if not a.reload:
        evaluate_loss_accuracy(iter_times_last, a.lr)
    step = iter_times_last
    end = iter_times_last + a.iters
    while step < end:
        # enqueue up to the next evaluation / save / print point without reading anything back
        nxt = min(end, (step // ITER_TIMES_PER_PRINT + 1) * ITER_TIMES_PER_PRINT)
        tr.run(step + 1, nxt - step)
        step = nxt
        if step % ITER_TIMES_PER_EVALUATE == 0:
            evaluate_loss_accuracy(step, lr_at(step))
        elif step % ITER_TIMES_PER_PRINT == 0:
            tr.last_stats()
            print("%s  step %d" % (get_time_str(), step))
        if step % save_every == 0:
            write_ckpt(os.path.join(a.models, "model_%s_%d_%s.dat" % (get_time_str(), step, name)), tr.get_blob())
    blob = tr.get_blob()
    with open(log, "w", newline="") as f:
        f.write("%d\r\n" % end)
        for r in rows:
            f.write(r + "\r\n")
    if end % save_every != 0:
        write_ckpt(os.path.join(a.models, "model_%s_%d_%s.dat" % (get_time_str(), end, name)), blob)
    write_ckpt(os.path.join(a.models, "model.dat"), blob)
    if export:
        write_ckpt(export, blob)
        print("exported %s" % export)


def parse_model_types(text):
    """'1,3' -> [1, 3]: distinct MODEL_TYPEs, 1..8 of them (argparse type of --model-types)"""
    try:
        types = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("expected a comma-separated list of model types, got %r" % text)
    if not types or len(set(types)) != len(types) or any(t not in MODEL_TYPES for t in types):
        raise argparse.ArgumentTypeError("model types are distinct values of %s, got %r" % (sorted(MODEL_TYPES), text))
    return types


def group_members(types):
    """[(MODEL_NAME, SELECT_QP_LIST)] of the listed model types"""
    return [MODEL_TYPES[t] for t in types]


def train_group_loop(a, pkg, grp, members, ntrain, nvalid, labels, export_dir=None):
    """train_loop for the members of a trainer group: one schedule, every step of all members in the same launches; the evaluation,
    the printing, the log and the files are per member, in <models>/<name>/, what train_loop writes for that member alone."""
    import score_cu_depth
    read_ckpt, write_ckpt = pkg.ethcnn.read_ckpt_blob, pkg.ethcnn.write_ckpt_blob
    names = [name for name, _ in members]
    qp0 = [qps[0] for _, qps in members]
    dirs = [os.path.join(a.models, name) for name in names]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    logs = [os.path.join(d, "loss_accuracy_list.dat") for d in dirs]
    rows = [[] for _ in members]
    if a.reload:
        last = []
        for m, d in enumerate(dirs):
            grp.set_blob(m, read_ckpt(os.path.join(d, "model.dat")))  # accumulators: zeros, as the reference's restore
            with open(logs[m]) as f:
                last.append(int(f.readline()))
                rows[m] = [ln.rstrip("\r\n") for ln in f if ln.strip()]
        if len(set(last)) != 1:
            raise SystemExit("--reload: the members stopped at different iterations %s" % last)
        iter_times_last = last[0]
    else:
        grp.init_weights(a.seed)
        iter_times_last = 0
    print("iter_times_last = %d" % iter_times_last)
    eval_rng = np.random.default_rng(a.seed + iter_times_last + 1)

    def evaluate_loss_accuracy(step, lr):
        out = []
        for which, n in ((pkg.ethcnn.SET_TRAIN, ntrain), (pkg.ethcnn.SET_VALID, nvalid)):
            idx = eval_rng.integers(0, n, min(NUM_EVAL, n))
            l3, a3, probs = grp.evaluate(which, qp0, idx=idx, want_probs=True)
            out.append((l3, a3, [[get_tendency_2x2(mx) for mx in score_cu_depth.class_matrices(labels[m][which][idx], probs[m])]
                                 for m in range(len(members))]))
        for m, name in enumerate(names):
            (tl, ta, tt), (vl, va, vt) = [(l3[m], a3[m], t[m]) for l3, a3, t in out]
            print("[%s] %s step %d: loss=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], accu=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], lr=%g"
                  % ((name, get_time_str(), step) + tuple(tl) + tuple(vl) + tuple(ta) + tuple(va) + (lr,)))
            print("[%s] tendency = [[%.3f, %.3f, %.3f] [%.3f, %.3f, %.3f]]" % ((name,) + tuple(tt) + tuple(vt)))
            rows[m].append("%d  " % step + "  ".join("%g" % v for v in list(tl) + list(vl) + list(ta) + list(va) + list(tt) + list(vt)))

    def lr_at(step):
        return a.lr * a.decay_rate ** (step // a.decay_steps)

    def save(step):
        for m, name in enumerate(names):
            write_ckpt(os.path.join(dirs[m], "model_%s_%d_%s.dat" % (get_time_str(), step, name)), grp.get_blob(m))

    if not a.reload:
        evaluate_loss_accuracy(iter_times_last, a.lr)
    step = iter_times_last
    end = iter_times_last + a.iters
    while step < end:
        nxt = min(end, (step // ITER_TIMES_PER_PRINT + 1) * ITER_TIMES_PER_PRINT)
        grp.run(step + 1, nxt - step)
        step = nxt
        if step % ITER_TIMES_PER_EVALUATE == 0:
            evaluate_loss_accuracy(step, lr_at(step))
        elif step % ITER_TIMES_PER_PRINT == 0:
            grp.last_stats()
            print("%s  step %d" % (get_time_str(), step))
        if step % ITER_TIMES_PER_SAVE == 0:
            save(step)
    if end % ITER_TIMES_PER_SAVE != 0:
        save(end)
    for m, (name, qps) in enumerate(members):
        blob = grp.get_blob(m)
        with open(logs[m], "w", newline="") as f:
            f.write("%d\r\n" % end)
            for r in rows[m]:
                f.write(r + "\r\n")
        write_ckpt(os.path.join(dirs[m], "model.dat"), blob)
        if export_dir:
            export = os.path.join(export_dir, pkg.ethcnn.model_name_for_qp(qps[0]))
            write_ckpt(export, blob)
            print("exported %s" % export)


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--train", help="training sample file (4992-byte records)")
    ap.add_argument("--valid", help="validation sample file")
    sequence_table.add_video_args(ap)
    sequence_table.add_format_args(ap)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--model-type", type=int, choices=sorted(MODEL_TYPES), default=1)
    g.add_argument("--qp", type=int, help="train one QP (model name qp<QP>)")
    g.add_argument("--model-types", type=parse_model_types, metavar="T[,T...]",
                   help="train the listed model types as one group from one copy of the samples; files go to <models>/<name>/")
    ap.add_argument("--iters", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--decay-steps", type=int, default=250000)
    ap.add_argument("--decay-rate", type=float, default=0.3163)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0, help="batches, dropout masks and the initial weights")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--reload", action="store_true", help="resume from <models>/model.dat and its loss_accuracy_list.dat")
    ap.add_argument("--models", default="Models")
    ap.add_argument("--export-ai", metavar="DIR", help="also write the final weights as video_to_cu_depth.py's model file in DIR")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main_group(a, pkg, ctx):
    """--model-types: the listed models as one TrainerGroup"""
    members = group_members(a.model_types)
    opt = pkg.ethcnn.train_options(batch=a.batch, lr=a.lr, momentum=a.momentum, decay_rate=a.decay_rate, decay_steps=a.decay_steps,
                                   dropout=not a.no_dropout, seed=a.seed)
    grp = pkg.TrainerGroup(ctx, [opt] * len(members))
    all_qps = sorted({q for _, qps in members for q in qps})
    labels = [dict() for _ in members]  # member -> set -> [samples, 16] depth bytes at the member's QP
    if a.yuv_dir:  # both sets cut in HBM with the label rows of every member's QPs, adopted by the group
        di = sequence_table
        for which, key in ((pkg.ethcnn.SET_TRAIN, "train"), (pkg.ethcnn.SET_VALID, "valid")):
            rows = [[] for _ in members]
            with pkg.SampleSet(ctx, "ai", all_qps) as sset:
                for sname, w, h, depth, chroma in a.video_sets[key]:
                    sset.add_sequence(w, h, di.find_one(a.yuv_dir, sname + ".yuv"), [di.info_file(a.info_dir, sname, q) for q in all_qps],
                                      bit_depth=depth, chroma=chroma)
                    for m, (_, qps) in enumerate(members):
                        rows[m].append(di.ctu_labels(di.info_file(a.info_dir, sname, qps[0]), w, h))
                grp.set_samples(which, sset.build(), take=True)
            for m in range(len(members)):
                labels[m][which] = np.concatenate(rows[m])
    else:
        for which, path in ((pkg.ethcnn.SET_TRAIN, a.train), (pkg.ethcnn.SET_VALID, a.valid)):
            data = load_records(path)
            grp.set_samples(which, data)
            for m, (_, qps) in enumerate(members):
                labels[m][which] = np.asarray(data).reshape(-1, REC)[:, 4160 + 16 * qps[0]: 4176 + 16 * qps[0]]
    for m, (_, qps) in enumerate(members):
        grp.set_qps(m, qps)
    ntrain, nvalid = len(labels[0][pkg.ethcnn.SET_TRAIN]), len(labels[0][pkg.ethcnn.SET_VALID])
    train_group_loop(a, pkg, grp, members, ntrain, nvalid, labels, a.export_ai)
    grp.close()
    return 0


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    if a.qp is not None:
        if not 0 <= a.qp <= 51:
            raise SystemExit("--qp must be in 0..51")
        name, qps = "qp%d" % a.qp, [a.qp]
    else:
        name, qps = MODEL_TYPES[a.model_type]
    sequence_table.check_source(a)
    fmt = sequence_table.source_format(a)
    if fmt != (8, 420) and not a.yuv_dir:
        raise SystemExit("--input-bit-depth / --input-chroma-format describe the YUVs of --yuv-dir: sample files hold 8-bit records")
    if a.yuv_dir:  # the sequence lists with their source formats, read (and refused) before a GPU is touched
        a.video_sets = {"train": sequence_table.select(a.sequences, sequence_table.AI_INDEX, "train", fmt),
                        "valid": sequence_table.select(a.valid_sequences or a.sequences, sequence_table.AI_INDEX, "valid", fmt)}
    os.makedirs(a.models, exist_ok=True)
    ctx = pkg.EthCnn(device=a.device)
    if a.model_types:
        rc = main_group(a, pkg, ctx)
        ctx.close()
        return rc
    tr = pkg.Trainer(ctx, batch=a.batch, lr=a.lr, momentum=a.momentum, decay_rate=a.decay_rate, decay_steps=a.decay_steps,
                     dropout=not a.no_dropout, seed=a.seed)
    labels = {}  # set -> [samples, 16] depth bytes at the model's QP
    if a.yuv_dir:  # both sets cut in HBM and adopted by the trainer: no sample file, no host copy of a record
        di = sequence_table
        for which, key in ((pkg.ethcnn.SET_TRAIN, "train"), (pkg.ethcnn.SET_VALID, "valid")):
            rows = []
            with pkg.SampleSet(ctx, "ai", qps) as sset:
                for sname, w, h, depth, chroma in a.video_sets[key]:
                    info = [di.info_file(a.info_dir, sname, q) for q in qps]
                    sset.add_sequence(w, h, di.find_one(a.yuv_dir, sname + ".yuv"), info, bit_depth=depth, chroma=chroma)
                    rows.append(di.ctu_labels(info[0], w, h))
                tr.set_samples(which, sset.build(), take=True)
            labels[which] = np.concatenate(rows)
    else:
        for which, path in ((pkg.ethcnn.SET_TRAIN, a.train), (pkg.ethcnn.SET_VALID, a.valid)):
            data = load_records(path)
            tr.set_samples(which, data)
            labels[which] = np.asarray(data).reshape(-1, REC)[:, 4160 + 16 * qps[0]: 4176 + 16 * qps[0]]
    ntrain, nvalid = len(labels[pkg.ethcnn.SET_TRAIN]), len(labels[pkg.ethcnn.SET_VALID])
    tr.set_qps(qps)

    def evaluate(which, idx):  # one ONE-batch evaluation at the model's QP -> (loss, accuracy, probs, labels)
        l3, a3, probs = tr.evaluate(which, qps[0], idx=idx, want_probs=True)
        return l3, a3, probs, labels[which][idx]

    export = os.path.join(a.export_ai, pkg.ethcnn.model_name_for_qp(qps[0])) if a.export_ai else None
    train_loop(a, pkg, tr, name, ntrain, nvalid, evaluate, export)
    tr.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
