"""TEST INFRASTRUCTURE: the inter sample set that the replay tests share (tests/test_gpu_replay.py, tests/test_gpu_second_trip.py).  Two
sequences cut from seeded residual YUVs and label files: 200x136 (3 x 2 whole CTUs, ragged edges dropped) with frames 1..4 and 128x64
with frames 1..3 -- 30 records; a context with seeded CNN and LSTM weights and open gates."""
import numpy as np

import extract_cases
import replay_ref

REC = 16516
QPS = [22, 27, 32, 37]
SEQS = (("a", 200, 136, 5), ("b", 128, 64, 4))  # name, width, height, frames of the files (frame 0 is the intra picture: not cut)


def context(pkg):
    c = pkg.EthCnn(device=0)
    c.load_synthetic(31, 8.0)
    c.load_lstm_synthetic(32, 3.0)
    c.set_thresholds(0.0, 0.0)  # open gates
    return c


class World(object):
    def close(self):
        self.set.close()
        self.ctx.close()


def build(pkg, directory):
    """the context, the files (written into `directory`), the set cut from them, its records and the planes the records came from"""
    w = World()
    w.dir = directory
    w.ctx = context(pkg)
    rng = np.random.default_rng(77)
    w.set = pkg.SampleSet(w.ctx, kind="inter", qps=QPS)
    w.luma, w.labels = [], []  # [sequence][slot] -> [frames, h, w] / [frames, h / 16, w / 16], frame 0 included
    for name, wd, ht, frames in SEQS:
        yuvs, labs = [], []
        for q in QPS:
            yuvs.append(str(w.dir / ("resi_%s_qp%d.yuv" % (name, q))))
            labs.append(str(w.dir / ("%s_qp%d_CUDepth.dat" % (name, q))))
            with open(yuvs[-1], "wb") as f:
                f.write(extract_cases.synth_yuv(rng, wd, ht, frames))
            with open(labs[-1], "wb") as f:
                f.write(rng.integers(0, 4, int(np.prod(extract_cases.label_shape(wd, ht, frames))), dtype=np.uint8).tobytes())
        w.set.add_sequence(wd, ht, yuvs, labs)
        w.luma.append([extract_cases.read_luma(p, wd, ht) for p in yuvs])
        w.labels.append([np.fromfile(p, dtype=np.uint8).reshape(extract_cases.label_shape(wd, ht, frames)) for p in labs])
    w.set.build()
    w.records = w.set.read()
    assert w.records.shape == (4 * 6 + 3 * 2, REC)
    w.plan = replay_ref.plan(w.records)
    return w
