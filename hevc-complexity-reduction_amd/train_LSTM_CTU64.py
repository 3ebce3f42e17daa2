"""Train ETH-LSTM (Low-Delay-P, one model per QP) on the GPU: the driver of ETH-LSTM_Training_LDP/train_LSTM_CTU64.py:283-431, with
command-line flags in place of its module constants.  Every step runs in the library's LSTM training kernels (LstmTrainer,
include/ethcnn.h "ETH-LSTM training"); this file only schedules, evaluates, logs and saves, through train_CNN_CTU64.py's loop.

    python train_LSTM_CTU64.py --train LDP_Train.dat_lstm_4qps_shuffled --valid LDP_Valid.dat_lstm_4qps_shuffled --qp 32
    python train_LSTM_CTU64.py ... --qp 32 --qp-scale 0.18 --export-lstm HM-16.5_Test_LDP/bin   # model_LDP_200000_qp32.dat
    python train_LSTM_CTU64.py --ldp-train LDP_Train.dat --ldp-valid LDP_Valid.dat --cnn-model Models/model.dat --qp 32
    python train_LSTM_CTU64.py --train ... --valid ... --qps 22,27,32,37 --qp-scale 0.18 --export-lstm DIR   # a deployment's four models

--qps: the listed models (1..8 distinct QPs) train as one group (LstmTrainerGroup, include/ethcnn.h "ETH-LSTM training, several models
at once") from one copy of the two sample sets, every step of all of them in the same launches; each model's weights, log and files
are those of its own --qp run with the same arguments (--seed included), and go to <models>/qp<QP>/.  With --ldp-train the slots of
all listed QPs are built in one LstmSampleSet per file and adopted by the group.

Sample files: get_LSTM_input.py's output (37264-byte samples: 64 info bytes + 20 slots of [qp | 16 labels | 448-vector] float32).
--qp keeps the samples whose slot-0 QP is that value (SELECT_QP_LIST, input_data.py:41-61,126-134; --model-type 1..4 = QP 22 / 27 /
32 / 37); they are uploaded once into HBM.  Like the reference: batch 64, lr 0.1 x 0.3163 every 25000 steps, momentum 0.9, gradients
clipped to global norm 5, 200000 steps; every 1000 steps an evaluation (no dropout) on 10000 random samples of each set as ONE batch
(NUM_TRAIN_PART / NUM_VALID_PART), with the class matrices and tendency of train_LSTM_CTU64.py:68-133 over its 20 x 10000 rows, one
19-column line in Models/loss_accuracy_list.dat, a checkpoint every 10000 steps and Models/model.dat at the end.  --reload resumes
from Models/model.dat and that log (momentum accumulators restart at zero, as the reference's Saver restore).
--qp-scale: the QP feature is qp / 51 * qp_scale.  1.0 is the training script as shipped; the deployed one-step graph (lstm_step,
both LDP daemons) computes qp / 51 * 0.18, so train with --qp-scale 0.18 for a model meant for them.
--ldp-train / --ldp-valid / --cnn-model (instead of --train / --valid): the Low-Delay-P sample files (16516-byte records) themselves.
The samples of --qp's slot alone are built in HBM with that residual CNN (LstmSampleSet: get_LSTM_input.py's samples, in its unshuffled
order) and handed to the trainer there; no 37264-byte file is written or read.  The evaluation's labels come from the records.
The slot of --qp, the slot QPs an error names and the "N of M samples" line are read from record 0; a file whose later records carry
other QPs in that slot loses those samples to the trainer's own selection (M counts them, N does not).
The reference trains "for 4 QPs separately", one process each; --qps is this port's own addition.
Not ported: the per-QP evaluation report (log_*.dat), the periodic swap of the in-memory training part (all samples are resident),
plotting.
"""
import argparse
import importlib
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import train_CNN_CTU64 as ai  # noqa: E402  (also puts the repository root and tools/ on sys.path)

REC, STEPS, SLOT = 37264, 20, 465
MODEL_TYPES = {1: 22, 2: 27, 3: 32, 4: 37}  # input_data.py:41-61
NUM_PART, ITER_TIMES_PER_SAVE = 10000, 10000  # train_LSTM_CTU64.py:57-58,64


def parse_qps(text):
    """'22,32' -> [22, 32]: 1..8 distinct QPs in 0..51 (argparse type of --qps)"""
    try:
        qps = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("expected a comma-separated list of QPs, got %r" % text)
    if not 1 <= len(qps) <= 8 or len(set(qps)) != len(qps) or any(not 0 <= q <= 51 for q in qps):
        raise argparse.ArgumentTypeError("--qps takes 1..8 distinct QPs in 0..51, got %r" % text)
    return qps


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--train", help="training sample file (37264-byte samples)")
    ap.add_argument("--valid", help="validation sample file")
    ap.add_argument("--ldp-train", metavar="FILE", help="training LDP sample file (16516-byte records): samples built in HBM")
    ap.add_argument("--ldp-valid", metavar="FILE", help="validation LDP sample file")
    ap.add_argument("--cnn-model", metavar="PREFIX", help="residual CNN checkpoint for --ldp-train / --ldp-valid")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--model-type", type=int, choices=sorted(MODEL_TYPES), default=1)
    g.add_argument("--qp", type=int, help="train the model of one QP (model name qp<QP>)")
    g.add_argument("--qps", type=parse_qps, metavar="QP[,QP...]",
                   help="train the models of the listed QPs as one group from one copy of the samples; files go to <models>/qp<QP>/")
    ap.add_argument("--qp-scale", type=float, default=1.0, help="1.0: the training script as shipped; 0.18: a model for the daemons")
    ap.add_argument("--iters", type=int, default=200000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--decay-steps", type=int, default=25000)
    ap.add_argument("--decay-rate", type=float, default=0.3163)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--clip-norm", type=float, default=5.0, help="MAX_GRAD_NORM; 0 = no clip")
    ap.add_argument("--seed", type=int, default=0, help="batches, dropout masks and the initial weights")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--reload", action="store_true", help="resume from <models>/model.dat and its loss_accuracy_list.dat")
    ap.add_argument("--models", default="Models")
    ap.add_argument("--export-lstm", metavar="DIR", help="also write the final weights as the daemons' model_LDP_200000_qp<QP>.dat in DIR")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    ldp = (a.ldp_train, a.ldp_valid, a.cnn_model)
    if any(v is not None for v in ldp):
        if a.train is not None or a.valid is not None:
            ap.error("--ldp-train / --ldp-valid / --cnn-model cannot be combined with --train / --valid")
        if any(v is None for v in ldp):
            ap.error("--ldp-train, --ldp-valid and --cnn-model go together")
    elif a.train is None or a.valid is None:
        ap.error("the following arguments are required: --train, --valid (or --ldp-train, --ldp-valid, --cnn-model)")
    return a


def ldp_set(pkg, ctx, tr, which, path, qp):
    """Builds the samples of one LDP file at QP `qp` in HBM and hands them to the trainer.  -> (kept, total, labels(idx) -> [20 n, 16])"""
    E = pkg.ethcnn
    rec = ai.load_records(path, E.LDP_RECORD_BYTES).reshape(-1, E.LDP_RECORD_BYTES)
    slot_qps = [int(rec[0, 64 + 4113 * s]) for s in range(4)]
    if qp not in slot_qps:
        raise SystemExit("%s: QP %d is not one of the file's slot QPs %s" % (path, qp, " ".join(str(q) for q in slot_qps)))
    o = 64 + 4113 * slot_qps.index(qp)
    heads, strides, _ = E.lstm_samples_plan(rec)
    with pkg.LstmSampleSet(ctx, slots=[slot_qps.index(qp)]) as ls:
        ls.build_from(rec)
        total = ls.count
        kept = tr.set_samples(which, ls, take=True)
    on = np.flatnonzero(rec[heads, o] == qp)  # the trainer's own selection (set_qps), on the slot-0 QP

    def labels(idx):
        j = on[np.asarray(idx)]
        refs = heads[j][:, None] - np.arange(STEPS)[None, :] * strides[j][:, None]
        return rec[refs.reshape(-1), o + 1: o + 17].astype(np.float32)

    return kept, total, labels


def ldp_group_set(pkg, ctx, grp, which, path, qps):
    """ldp_set for a group: the slots of all listed QPs in ONE sample set, adopted by the group.
    -> (kept [k], total, [labels(idx) -> [20 n, 16] per member])"""
    E = pkg.ethcnn
    rec = ai.load_records(path, E.LDP_RECORD_BYTES).reshape(-1, E.LDP_RECORD_BYTES)
    slot_qps = [int(rec[0, 64 + 4113 * s]) for s in range(4)]
    heads, strides, _ = E.lstm_samples_plan(rec)
    with pkg.LstmSampleSet(ctx, slots=[slot_qps.index(q) for q in qps]) as ls:
        ls.build_from(rec)
        total = ls.count
        kept = grp.set_samples(which, ls, take=True)

    def member_labels(qp):
        o = 64 + 4113 * slot_qps.index(qp)
        on = np.flatnonzero(rec[heads, o] == qp)  # the member's own selection, on the slot-0 QP

        def labels(idx):
            j = on[np.asarray(idx)]
            refs = heads[j][:, None] - np.arange(STEPS)[None, :] * strides[j][:, None]
            return rec[refs.reshape(-1), o + 1: o + 17].astype(np.float32)
        return labels

    return kept, total, [member_labels(q) for q in qps]


def check_ldp_qps(pkg, path, qps):
    """a QP that is not one of the file's slot QPs is refused before anything is built"""
    rec0 = ai.load_records(path, pkg.ethcnn.LDP_RECORD_BYTES)[:pkg.ethcnn.LDP_RECORD_BYTES]
    slot_qps = [int(rec0[64 + 4113 * s]) for s in range(4)]
    for q in qps:
        if q not in slot_qps:
            raise SystemExit("%s: QP %d is not one of the file's slot QPs %s" % (path, q, " ".join(str(x) for x in slot_qps)))


def train_group_loop(a, pkg, grp, qps, counts, evaluate_labels, export_dir=None):
    """train_CNN_CTU64.train_group_loop for the members of an LstmTrainerGroup: one schedule, every step of all members in the same
    launches; evaluation samples, printing, log and files are per member, in <models>/qp<QP>/, what train_loop writes for that
    member alone.  counts[which][m]: the samples member m keeps; evaluate_labels(m, which, idx) -> [20 n, 16]."""
    import score_cu_depth
    read_ckpt, write_ckpt = pkg.ethcnn.read_ckpt_lstm_blob, pkg.ethcnn.write_ckpt_lstm_blob
    K = len(qps)
    names = ["qp%d" % q for q in qps]
    dirs = [os.path.join(a.models, name) for name in names]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    logs = [os.path.join(d, "loss_accuracy_list.dat") for d in dirs]
    rows = [[] for _ in qps]
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
    eval_rngs = [np.random.default_rng(a.seed + iter_times_last + 1) for _ in qps]  # each member draws what its own run draws

    def evaluate_loss_accuracy(step, lr):
        out = []  # per set: [(l3, a3, tendency)] per member
        for which in (pkg.ethcnn.SET_TRAIN, pkg.ethcnn.SET_VALID):
            idx = [eval_rngs[m].integers(0, counts[which][m], min(NUM_PART, counts[which][m])) for m in range(K)]
            res = [None] * K
            for n in sorted({len(i) for i in idx}):  # one group evaluation per distinct count (one, for sets of >= 10000 samples)
                arr = np.stack([i if len(i) == n else np.resize(i, n) % counts[which][m] for m, i in enumerate(idx)])
                l3, a3, probs = grp.evaluate(which, idx=arr, want_probs=True)
                for m in range(K):
                    if len(idx[m]) == n:
                        ms = score_cu_depth.class_matrices(evaluate_labels(m, which, idx[m]), probs[m])
                        res[m] = (l3[m], a3[m], [ai.get_tendency_2x2(mx) for mx in ms])
            out.append(res)
        for m, name in enumerate(names):
            (tl, ta, tt), (vl, va, vt) = out[0][m], out[1][m]
            print("[%s] %s step %d: loss=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], accu=[[%.3f %.3f %.3f] [%.3f %.3f %.3f]], lr=%g"
                  % ((name, ai.get_time_str(), step) + tuple(tl) + tuple(vl) + tuple(ta) + tuple(va) + (lr,)))
            print("[%s] tendency = [[%.3f, %.3f, %.3f] [%.3f, %.3f, %.3f]]" % ((name,) + tuple(tt) + tuple(vt)))
            rows[m].append("%d  " % step + "  ".join("%g" % v for v in list(tl) + list(vl) + list(ta) + list(va) + list(tt) + list(vt)))

    def lr_at(step):
        return a.lr * a.decay_rate ** (step // a.decay_steps)

    def save(step):
        for m, name in enumerate(names):
            write_ckpt(os.path.join(dirs[m], "model_%s_%d_%s.dat" % (ai.get_time_str(), step, name)), grp.get_blob(m))

    if not a.reload:
        evaluate_loss_accuracy(iter_times_last, a.lr)
    step = iter_times_last
    end = iter_times_last + a.iters
    while step < end:
        nxt = min(end, (step // ai.ITER_TIMES_PER_PRINT + 1) * ai.ITER_TIMES_PER_PRINT)
        grp.run(step + 1, nxt - step)
        step = nxt
        if step % ai.ITER_TIMES_PER_EVALUATE == 0:
            evaluate_loss_accuracy(step, lr_at(step))
        elif step % ai.ITER_TIMES_PER_PRINT == 0:
            grp.last_stats()
            print("%s  step %d" % (ai.get_time_str(), step))
        if step % ITER_TIMES_PER_SAVE == 0:
            save(step)
    if end % ITER_TIMES_PER_SAVE != 0:
        save(end)
    for m, qp in enumerate(qps):
        blob = grp.get_blob(m)
        with open(logs[m], "w", newline="") as f:
            f.write("%d\r\n" % end)
            for r in rows[m]:
                f.write(r + "\r\n")
        write_ckpt(os.path.join(dirs[m], "model.dat"), blob)
        if export_dir:
            export = os.path.join(export_dir, pkg.ethcnn.lstm_model_name_for_qp(qp))
            write_ckpt(export, blob)
            print("exported %s" % export)


def main_group(a, pkg):
    """--qps: the listed models as one LstmTrainerGroup"""
    E = pkg.ethcnn
    qps = a.qps
    from_ldp = a.ldp_train is not None
    if from_ldp:
        for path in (a.ldp_train, a.ldp_valid):
            check_ldp_qps(pkg, path, qps)
    else:
        files = {E.SET_TRAIN: ai.load_records(a.train, REC), E.SET_VALID: ai.load_records(a.valid, REC)}
    os.makedirs(a.models, exist_ok=True)
    ctx = pkg.EthCnn(device=a.device)
    opt = E.lstm_train_options(batch=a.batch, lr=a.lr, momentum=a.momentum, decay_rate=a.decay_rate, decay_steps=a.decay_steps,
                               dropout=not a.no_dropout, seed=a.seed, qp_scale=a.qp_scale, clip_norm=a.clip_norm)
    grp = pkg.LstmTrainerGroup(ctx, [opt] * len(qps))
    for m, q in enumerate(qps):
        grp.set_qps(m, [q])
    counts, totals = {}, {}
    if from_ldp:
        ctx.load_checkpoint(a.cnn_model)
        lab = {}
        for which, path in ((E.SET_TRAIN, a.ldp_train), (E.SET_VALID, a.ldp_valid)):
            counts[which], totals[which], lab[which] = ldp_group_set(pkg, ctx, grp, which, path, qps)

        def evaluate_labels(m, which, idx):
            return lab[which][m](idx)
    else:
        kept = {}
        for which, data in files.items():
            counts[which] = grp.set_samples(which, data)
            totals[which] = data.size // REC
            kept[which] = [E.lstm_select_qp(data, [q]) for q in qps]

        def evaluate_labels(m, which, idx):
            data = np.asarray(files[which]).reshape(-1, REC)
            rows = np.ascontiguousarray(data[kept[which][m][np.asarray(idx)], 64:]).view(np.float32).reshape(len(idx), STEPS, SLOT)
            return rows[:, :, 1:17].reshape(-1, 16)
    for m, q in enumerate(qps):
        print("QP %d: %d of %d training and %d of %d validation samples"
              % (q, counts[E.SET_TRAIN][m], totals[E.SET_TRAIN], counts[E.SET_VALID][m], totals[E.SET_VALID]))
    train_group_loop(a, pkg, grp, qps, counts, evaluate_labels, a.export_lstm)
    grp.close()
    ctx.close()
    return 0


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    if a.qps:
        return main_group(a, pkg)
    qp = a.qp if a.qp is not None else MODEL_TYPES[a.model_type]
    if not 0 <= qp <= 51:
        raise SystemExit("--qp must be in 0..51")
    name = "qp%d" % qp
    from_ldp = a.ldp_train is not None
    if not from_ldp:
        train, valid = ai.load_records(a.train, REC), ai.load_records(a.valid, REC)
    os.makedirs(a.models, exist_ok=True)
    ctx = pkg.EthCnn(device=a.device)
    tr = pkg.LstmTrainer(ctx, batch=a.batch, lr=a.lr, momentum=a.momentum, decay_rate=a.decay_rate, decay_steps=a.decay_steps,
                         dropout=not a.no_dropout, seed=a.seed, qp_scale=a.qp_scale, clip_norm=a.clip_norm)
    tr.set_qps([qp])
    if from_ldp:
        ctx.load_checkpoint(a.cnn_model)
        ntrain, alltrain, ltrain = ldp_set(pkg, ctx, tr, pkg.ethcnn.SET_TRAIN, a.ldp_train, qp)
        nvalid, allvalid, lvalid = ldp_set(pkg, ctx, tr, pkg.ethcnn.SET_VALID, a.ldp_valid, qp)
        print("QP %d: %d of %d training and %d of %d validation samples" % (qp, ntrain, alltrain, nvalid, allvalid))
    else:
        ntrain = tr.set_samples(pkg.ethcnn.SET_TRAIN, train)
        nvalid = tr.set_samples(pkg.ethcnn.SET_VALID, valid)
        kept = {pkg.ethcnn.SET_TRAIN: pkg.ethcnn.lstm_select_qp(train, [qp]), pkg.ethcnn.SET_VALID: pkg.ethcnn.lstm_select_qp(valid, [qp])}
        print("QP %d: %d of %d training and %d of %d validation samples" % (qp, ntrain, train.size // REC, nvalid, valid.size // REC))

    def evaluate(which, idx):  # ONE batch of len(idx) samples -> (loss, accuracy, probs [20 n, 21], labels [20 n, 16])
        if from_ldp:
            l3, a3, probs = tr.evaluate(which, idx=idx, want_probs=True)
            return l3, a3, probs, (ltrain if which == pkg.ethcnn.SET_TRAIN else lvalid)(idx)
        data = np.asarray(train if which == pkg.ethcnn.SET_TRAIN else valid).reshape(-1, REC)
        l3, a3, probs = tr.evaluate(which, idx=idx, want_probs=True)
        rows = np.ascontiguousarray(data[kept[which][np.asarray(idx)], 64:]).view(np.float32).reshape(len(idx), STEPS, SLOT)
        return l3, a3, probs, rows[:, :, 1:17].reshape(-1, 16)

    export = os.path.join(a.export_lstm, pkg.ethcnn.lstm_model_name_for_qp(qp)) if a.export_lstm else None
    ai.train_loop(a, pkg, tr, name, ntrain, nvalid, evaluate, export, num_eval=NUM_PART, save_every=ITER_TIMES_PER_SAVE,
                  ckpt_io=(pkg.ethcnn.read_ckpt_lstm_blob, pkg.ethcnn.write_ckpt_lstm_blob))
    tr.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
