"""TEST INFRASTRUCTURE: what the GPU tests of a large simulator set check around a boundary inside it -- the cap of k_sim_pack's grid
(tests/test_gpu_second_trip.py) or the end of a staged piece of the host entries (tests/test_gpu_host_pieces.py)."""
import numpy as np

import decide_ref
import sim_ref

# two candidates (the reference's [k, n, 16] int64 arrays grow with the count); under the AI gate order the second closes gate 1 where
# a sub-batch's largest p64 bin is <= 500 and gate 2 where its largest p32 bin is <= 600, and it is crossed (down_k > up_k: with
# down_k <= up_k the AI-order gates change nothing, a closed gate's bins would be CURRENT ONLY anyway)
SIM_CANDS = sim_ref.thr([(600, 700, 800), (300, 400, 500)], [(400, 300, 200), (500, 600, 900)])
REJECTED, LABELLED = decide_ref.REJECTED, decide_ref.LABELLED


def sim_checks(sim, s, cap, reject_at, labelled_at, rejected=1):
    """info, the evaluation of the two candidates, and the decisions over 1000 CTUs around the boundary `cap`: the records behind it,
    one by one, among them a rejected and a labelled CTU.  sim: the library's set, s: the sim_ref.Set of the same CTUs, which holds
    `rejected` rejected CTUs"""
    assert sim.info() == s.info() and s.info()["rejected_ctus"] == rejected
    want = s.evaluate(SIM_CANDS, sim_ref.GATES_AI)
    assert all(want[f].any() for f in sim_ref.FIELDS if f != "edge_split")
    assert sim_ref.equal(sim.eval(SIM_CANDS, "ai"), want)
    first, n = cap - 500, 1000
    assert first <= cap < reject_at < first + n and cap < labelled_at < first + n
    for cand in (SIM_CANDS[:1], SIM_CANDS[1:]):
        want = decide_ref.decide(s, cand, sim_ref.GATES_AI, 512, first, n)
        assert want["codes"][reject_at - first, 21] & REJECTED and want["codes"][labelled_at - first, 21] & LABELLED
        got = sim.decide(cand, "ai", 512, first, n)
        for k in ("codes", "reach", "depth"):
            assert np.array_equal(got[k], want[k]), k
