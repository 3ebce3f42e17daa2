"""Bits of the trainers against another checkout's: SHA-256 digests of what a short training run leaves behind, as one JSON line.

    python scripts/train_bits.py [--parent-root DIR] [--out profiles/train_bits.json] [--parent-out profiles/train_bits_parent.json]

Every case runs 20 device-drawn steps with dropout, one step on an explicit batch and one evaluation over two pieces, and digests
the weight blob, the momentum accumulators, the last step's loss / accuracy lists and the evaluation's lists and probabilities:
  solo All-Intra    batch 7 and 64, tune 0 and 2
  solo Low-Delay-P  batch 7
  solo ETH-LSTM     batch 7 and 20, under a QP list that keeps a subset of the samples
  groups            an ETH-CNN group and an ETH-LSTM group of K = 3 at batch 7
--root DIR: take the package (and its built library) from the checkout DIR instead of this one; the cases, the data and this file
stay the same.  --parent-root DIR: first the same run in a fresh child process on the checkout DIR (this process has not opened
the GPU yet), then this checkout's; the two lines must be equal, else the exit status is 1 and the differing digests are named.
"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 20


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def cnn_case(pkg, ctx, data, valid, nrec, batch, net="ai", tune=0):
    rng = np.random.default_rng(batch + 10 * tune)
    qps = [22, 27, 32, 37]
    with pkg.Trainer(ctx, batch=batch, dropout=True, seed=40 + batch, net=net, tune=tune, lr=0.02, decay_steps=8) as t:
        t.set_samples(0, data)
        t.set_samples(1, valid)
        if net == "ai":
            t.set_qps([22, 37])
        t.init_weights(3)
        t.run(1, STEPS)
        t.step_indices(STEPS + 1, rng.integers(0, nrec, batch), rng.choice(qps, batch))
        blob, accum = t.get_blob(with_accum=True)
        stats = t.last_stats()
        ev = t.evaluate(1, 32, idx=rng.permutation(1027), want_probs=True)
    return {"blob": sha(blob), "accum": sha(accum), "stats": sha(*stats), "eval": sha(*ev)}


def lstm_case(pkg, ctx, data, valid, batch):
    rng = np.random.default_rng(batch)
    with pkg.LstmTrainer(ctx, batch=batch, dropout=True, seed=60 + batch, lr=0.05, decay_steps=8) as t:
        t.set_qps([27, 37])  # keeps about half of the samples
        nkept, nvalid = t.set_samples(0, data), t.set_samples(1, valid)
        t.init_weights(4)
        t.run(1, STEPS)
        t.step_indices(STEPS + 1, rng.integers(0, nkept, batch))
        blob, accum = t.get_blob(with_accum=True)
        stats = t.last_stats()
        ev = t.evaluate(1, idx=rng.integers(0, nvalid, 259), want_probs=True)
    return {"kept": [nkept, nvalid], "blob": sha(blob), "accum": sha(accum), "stats": sha(*stats), "eval": sha(*ev)}


def cnn_group_case(pkg, ctx, data, valid, nrec, batch=7, k=3):
    rng = np.random.default_rng(77)
    opts = [pkg.ethcnn.train_options(batch=batch, dropout=True, seed=80 + m, lr=0.01 * (m + 1), decay_steps=8) for m in range(k)]
    with pkg.TrainerGroup(ctx, opts) as g:
        g.set_samples(0, data)
        g.set_samples(1, valid)
        for m in range(k):
            g.set_qps(m, [[22], [27, 32], [37]][m % 3])
        g.init_weights(list(range(1, k + 1)))
        g.run(1, STEPS)
        g.step_indices(STEPS + 1, rng.integers(0, nrec, (k, batch)), rng.choice([22, 27, 32, 37], (k, batch)))
        state = [g.get_blob(m, with_accum=True) for m in range(k)]
        stats = g.last_stats()
        ev = g.evaluate(1, [22, 32, 37][:k], idx=rng.permutation(1027), want_probs=True)
    return {"blob": sha(*[s[0] for s in state]), "accum": sha(*[s[1] for s in state]), "stats": sha(*stats), "eval": sha(*ev)}


def lstm_group_case(pkg, ctx, data, valid, batch=7, k=3):
    rng = np.random.default_rng(78)
    opts = [pkg.ethcnn.lstm_train_options(batch=batch, dropout=True, seed=90 + m, lr=0.05 * (m + 1), decay_steps=8) for m in range(k)]
    with pkg.LstmTrainerGroup(ctx, opts) as g:
        for m in range(k):
            g.set_qps(m, [[27, 37], [], [22]][m % 3])
        g.set_samples(0, data)
        g.set_samples(1, valid)
        kept = [[g.num_samples(m, s) for s in (0, 1)] for m in range(k)]
        g.init_weights(list(range(1, k + 1)))
        g.run(1, STEPS)
        g.step_indices(STEPS + 1, np.stack([rng.integers(0, kept[m][0], batch) for m in range(k)]))
        state = [g.get_blob(m, with_accum=True) for m in range(k)]
        stats = g.last_stats()
        ev = g.evaluate(1, idx=np.stack([rng.integers(0, kept[m][1], 259) for m in range(k)]), want_probs=True)
    return {"kept": kept, "blob": sha(*[s[0] for s in state]), "accum": sha(*[s[1] for s in state]), "stats": sha(*stats), "eval": sha(*ev)}


def digests(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))  # the data generators of THIS checkout, whichever library runs
    import train_data
    import train_data_ldp
    import train_data_lstm
    pkg = importlib.import_module("hevc-complexity-reduction_amd")
    assert os.path.realpath(pkg.ethcnn.LIB_PATH).startswith(os.path.realpath(root) + os.sep), pkg.ethcnn.LIB_PATH
    nrec = 500
    ai, ai_valid = train_data.make_records(nrec, seed=1), train_data.make_records(1027, seed=2)
    ldp, ldp_valid = train_data_ldp.make_records(nrec, seed=3), train_data_ldp.make_records(1027, seed=4)
    lstm, lstm_valid = train_data_lstm.make_samples(240, seed=5), train_data_lstm.make_samples(120, seed=6)
    out = {}
    with pkg.EthCnn(device=0) as ctx:
        for batch in (7, 64):
            for tune in (0, 2):
                out["ai_b%d_tune%d" % (batch, tune)] = cnn_case(pkg, ctx, ai, ai_valid, nrec, batch, tune=tune)
        out["ldp_b7"] = cnn_case(pkg, ctx, ldp, ldp_valid, nrec, 7, net="ldp")
        for batch in (7, 20):
            out["lstm_b%d" % batch] = lstm_case(pkg, ctx, lstm, lstm_valid, batch)
        out["cnn_group_k3_b7"] = cnn_group_case(pkg, ctx, ai, ai_valid, nrec)
        out["lstm_group_k3_b7"] = lstm_group_case(pkg, ctx, lstm, lstm_valid)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library run")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit, run first in a process of its own")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-out", default="")
    a = ap.parse_args()
    parent = None
    if a.parent_root:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent_root)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode:
            raise SystemExit("parent run failed:\n" + r.stdout + r.stderr)
        parent = r.stdout.strip().splitlines()[-1]
        print(parent, flush=True)
        if a.parent_out:
            with open(a.parent_out, "w") as f:
                f.write(parent + "\n")
    line = json.dumps(digests(os.path.abspath(a.root)), sort_keys=True)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if parent is not None and parent != line:
        old, new = json.loads(parent), json.loads(line)
        for case in sorted(set(old) | set(new)):
            for key in sorted(set(old.get(case, {})) | set(new.get(case, {}))):
                if old.get(case, {}).get(key) != new.get(case, {}).get(key):
                    print("DIFFERS: %s %s" % (case, key), file=sys.stderr)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
