"""-m gpu: a pacer set with a POLICY PER SLOT (include/ethcnn.h "search budget, online: several sequences, a POLICY per slot") against its
defining equality: for every slot, between two binds, every result field and every baked word are those of a solo pacer created with
the slot's policy and given the same frames in the same order -- whatever policies the other slots of the calls had.  Two references,
as in tests/test_gpu_pacer_set.py, whose helpers are restated here with a policy where that file has one ladder, budget and mode:
  reference 1  a solo pacer (pkg.Pacer) per slot and per binding;
  reference 2  the numpy restatement (tests/budget_ref.py), which shares nothing with any kernel.
The references are compared with each other first.  Integers and three float constants only: every comparison is equality.
A policy is named by its RUNGS = K + 1, the rows of its ladder with the full search appended: 2, 256, 257 and 513 are one rung block,
exactly one, one more and three; 65 stands under the weights 1 1 1 1; 514 is the default ladder; 4097 is the longest (17 rung blocks)."""
import collections
import hashlib
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import budget_ref as bref
import decide_ref as dref
import sim_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hevc-complexity-reduction_amd", "bin")
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
GOLD = os.path.join(ROOT, "tests", "golden", "model_LDP_200000_qp32.dat")
M = 10 ** 6
FRAMES = 10
# name: width, height
SHAPES = {"one": (64, 64),          # 1 CTU
          "edge": (72, 72),         # 4 CTUs: edge nodes in three of them, corner nodes in the last
          "long": (4160, 64),       # 65 CTUs: two slices
          "wide": (1088, 1024)}     # 272 CTUs: five slices
ORDER = ("one", "edge", "long", "wide")
Pol = collections.namedtuple("Pol", "rungs share mode weights")
_CASES, _LADDERS, _CHECKED, _BAKED, _WANT = {}, {}, {}, {}, {}


def _per(name):
    w, h = SHAPES[name]
    return ((w + 63) // 64) * ((h + 63) // 64)


def _case(name):
    """(probs [FRAMES, per, 21], one sim_ref.Set per frame) made once and never changed (test_gpu_pacer_set.py's inputs: the k / 1024
    grid, values exactly at up / down of several rungs, a spread that differs per frame so that the picked rungs differ)"""
    if name not in _CASES:
        w, h = SHAPES[name]
        per = _per(name)
        rng = np.random.default_rng(sum(map(ord, name)) + 2000)
        k = rng.integers(0, 1025, size=(FRAMES, per, 21))
        spread = np.linspace(0.05, 1.0, FRAMES)[rng.permutation(FRAMES)]
        k = 512 + np.rint((k - 512) * spread[:, None, None]).astype(np.int64)
        at_rung = rng.choice(np.array([1024 - 100, 99, 1024 - 300, 299, 512, 511, 1024, 0, 768, 256]), size=k.shape)
        k = np.where(rng.integers(0, 6, size=k.shape) == 0, at_rung, k)
        probs = (k / 1024.0).astype(np.float32)
        sets = []
        for f in range(FRAMES):
            s = ref.Set()
            s.add_frames(probs[f], None, w, h, 0)
            sets.append(s)
        probs.setflags(write=False)
        _CASES[name] = (probs, sets)
    return _CASES[name]


def _ladder(rungs):
    """the rungs - 1 rows of a policy's ladder: the default ladder (514), its cheapest rung alone (2: a frame leaves a large remainder),
    its first 512 rows (513), every second of its rows from row 0 (256) and from row 1 (257), every eighth (65) -- no two policies share a
    ladder, and each spans the whole range of costs --, seeded candidates in no order at all otherwise"""
    if rungs not in _LADDERS:
        k, full = rungs - 1, bref.default_ladder()
        _LADDERS[rungs] = (full if rungs == 514 else full[[512]].copy() if rungs == 2 else full[:512].copy() if rungs == 513 else full[0::2][:255].copy()
                           if rungs == 256 else full[1::2].copy() if rungs == 257 else full[0::8][:64].copy() if rungs == 65
                           else dref.candidates(np.random.default_rng(rungs), max(k, 4))[:k].copy())
        assert len(_LADDERS[rungs]) == k
    return _LADDERS[rungs]


def _as_dict(p):
    return {"budget": p.share, "mode": p.mode, "ladder": None if p.rungs == 514 else _ladder(p.rungs), "weights": p.weights}


def _fields(res):
    return {"frame": int(res["frame"]), "rung": int(res["rung"]), "over": int(res["over"]), "cost": int(res["cost"]), "full": int(res["full"]),
            "carry": int(res["carry_lo"]) | int(res["carry_hi"]) << 64, "up_k": res["up_k"].tolist(), "down_k": res["down_k"].tolist()}


# ------------------------------------------------------------------------------------------------------------ the two references ---
# a slot's history is a list of events: (name, f) = frame f of case `name`, "reset", or ("bind", policy)
def _restated(events, first, policies):
    """reference 2: the choice rule of "search budget" in Python integers over the restated checks -> [(fields, baked bytes)]"""
    out, carry, count, p = [], 0, 0, first
    for ev in events:
        if ev == "reset" or ev[0] == "bind":
            carry, count, p = 0, 0, p if ev == "reset" else policies[ev[1]]
            continue
        name, f = ev
        s, ladder, weights, ppm = _case(name)[1][f], _ladder(p.rungs), p.weights or bref.WEIGHTS, int(round(p.share * 1e6))
        if (name, f, p.rungs) not in _CHECKED:
            _CHECKED[name, f, p.rungs] = bref.cost(s, ladder, 0, _per(name), 1)[0]
        costs = [sum(int(w) * int(x) for w, x in zip(weights, c)) for c in _CHECKED[name, f, p.rungs]]
        full = costs[-1]
        allow = ppm * full + carry
        fits = [i for i in range(len(costs) - 1) if costs[i] * M <= allow]
        at = fits[0] if fits else min(range(len(costs) - 1), key=lambda i: (costs[i], i))
        carry = allow - costs[at] * M if fits and p.mode == "carry" else 0
        if (name, f, p.rungs, at) not in _BAKED:
            _BAKED[name, f, p.rungs, at] = bref.bake(s, ladder, [at], 0, _per(name), 1).tobytes()
        out.append(({"frame": count, "rung": at, "over": 0 if fits else 1, "cost": costs[at], "full": full, "carry": carry,
                     "up_k": ladder[at]["up_k"].tolist(), "down_k": ladder[at]["down_k"].tolist()}, _BAKED[name, f, p.rungs, at]))
        count += 1
    return out


def _solo(pkg, ctx, events, first, policies):
    """reference 1: the slot's history through solo pacers, a fresh one of the new policy at every bind -> [(fields, baked bytes)]"""
    out = []
    make = lambda p: pkg.Pacer(ctx, p.share, p.mode, None if p.rungs == 514 else _ladder(p.rungs), p.weights)
    pacer = make(first)
    try:
        for ev in events:
            if ev == "reset":
                pacer.reset()
            elif ev[0] == "bind":
                pacer.close()
                pacer = make(policies[ev[1]])
            else:
                name, f = ev
                baked, res = pacer.frame(_case(name)[0][f], *SHAPES[name])
                out.append((_fields(res), baked.tobytes()))
    finally:
        pacer.close()
    return out


def _references(pkg, ctx, histories, policies, slot_policy):
    """{slot: [(fields, baked bytes)]} on which both references agree; a history under the same policies is computed once"""
    want = {}
    for slot, events in histories.items():
        first = policies[slot_policy[slot]]
        key = (first, tuple(events), tuple(policies[e[1]] for e in events if e != "reset" and e[0] == "bind"))
        if key not in _WANT:
            one, two = _solo(pkg, ctx, events, first, policies), _restated(events, first, policies)
            assert [x[0] for x in one] == [x[0] for x in two], "the two REFERENCES disagree on the results of slot %d (%r)" % (slot, first)
            assert [x[1] for x in one] == [x[1] for x in two], "the two REFERENCES disagree on the baked rows of slot %d (%r)" % (slot, first)
            _WANT[key] = one
        want[slot] = _WANT[key]
    return want


def _histories(calls):
    """the calls of a run -- lists of (slot, name, f), ("reset", slot) or ("bind", slot, policy) -- as one history per slot"""
    out = {}
    for call in calls:
        if call[0] == "reset":
            out.setdefault(call[1], []).append("reset")
        elif call[0] == "bind":
            out.setdefault(call[1], []).append(("bind", call[2]))
        else:
            for slot, name, f in call:
                out.setdefault(slot, []).append((name, f))
    return out


def _between(ps, call):
    if call[0] == "reset":
        ps.reset(call[1])
    elif call[0] == "bind":
        ps.bind(call[1], call[2])
        assert ps.policy_of(call[1]) == call[2]
    else:
        return False
    return True


def _run_host(ps, calls):
    """the calls through PacerSet.frames (pageable arrays: the staged route) -> {slot: [(fields, baked bytes)]}"""
    got = {}
    for call in calls:
        if _between(ps, call):
            continue
        baked, results = ps.frames([{"slot": slot, "probs": _case(name)[0][f], "width": SHAPES[name][0], "height": SHAPES[name][1]} for slot, name, f in call])
        for (slot, name, f), b, r in zip(call, baked, results):
            assert b.shape == (_per(name), 21)
            got.setdefault(slot, []).append((_fields(r), b.tobytes()))
    return got


def _run_device(pkg, ctx, ps, calls, guard=64):
    """the calls through PacerSet.frames_device, queued back to back with the resets and binds between them and ONE wait at the end; every
    frame in place in a region of its own between guard words, every result in a slot of its own -> {slot: [(fields, baked bytes)]}"""
    size = pkg.ethcnn.PACER_RESULT.itemsize
    where, at = [], 0
    for call in calls:
        if call[0] in ("reset", "bind"):
            continue
        for slot, name, f in call:
            where.append((slot, name, f, at))
            at += _per(name) * 84 + 2 * guard
    raw = np.full(at, 0xAB, np.uint8)
    for slot, name, f, o in where:
        raw[o + guard:o + guard + _per(name) * 84] = np.frombuffer(_case(name)[0][f].tobytes(), np.uint8)
    dev, d_res = ctx.alloc(raw.size), ctx.alloc(len(where) * size + 16)
    try:
        dev.upload(raw)
        d_res.upload(np.full(len(where) * size + 16, 0xCD, np.uint8))
        n = 0
        for call in calls:
            if _between(ps, call):
                continue
            frames = []
            for slot, name, f in call:
                o = where[n][3]
                frames.append({"slot": slot, "d_probs": dev.ptr + o + guard, "width": SHAPES[name][0], "height": SHAPES[name][1], "d_baked": dev.ptr + o + guard,
                               "d_result": d_res.ptr + 8 + n * size})
                n += 1
            ps.frames_device(frames)
        ctx.synchronize()
        res = d_res.download(np.uint8, len(where) * size + 16)
        out = dev.download(np.uint8, raw.size)
    finally:
        dev.free()
        d_res.free()
    assert (res[:8] == 0xCD).all() and (res[-8:] == 0xCD).all()
    records = res[8:-8].view(pkg.ethcnn.PACER_RESULT)
    got = {}
    for n, (slot, name, f, o) in enumerate(where):
        end = o + guard + _per(name) * 84
        assert (out[o:o + guard] == 0xAB).all() and (out[end:end + guard] == 0xAB).all(), (slot, name, f)
        got.setdefault(slot, []).append((_fields(records[n]), out[o + guard:end].tobytes()))
    return got


def _run(pkg, ctx, ps, calls, form):
    return _run_host(ps, calls) if form == "host" else _run_device(pkg, ctx, ps, calls)


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for slot in sorted(want):
        assert [x[0] for x in got[slot]] == [x[0] for x in want[slot]], "%s: the results of slot %d differ" % (what, slot)
        for n, (g, w) in enumerate(zip(got[slot], want[slot])):
            assert g[1] == w[1], "%s: slot %d, its frame %d: %d baked words differ" % (
                what, slot, n, int((np.frombuffer(g[1], "<u4") != np.frombuffer(w[1], "<u4")).sum()))


def _schedule(seed, slots, ncalls=10):
    """ncalls calls that name changing subsets of the slots in shuffled order; slot s takes the four shapes in turn, starting at its
    own, so that every policy meets 1, 4, 65 and 272 CTUs and its carry crosses the changes of geometry"""
    rng = np.random.default_rng(seed)
    done, calls = {s: 0 for s in slots}, []
    for c in range(ncalls):
        pick = [s for s in slots if rng.integers(0, 4) > 0] or [slots[int(rng.integers(0, len(slots)))]]
        if c == 0:
            pick = list(slots)
        pick = [pick[i] for i in rng.permutation(len(pick))]
        calls.append([(s, ORDER[(s + done[s]) % 4], done[s]) for s in pick])
        for s in pick:
            done[s] += 1
    return calls


# budgets 0, 0.13, 0.4 and 1.0 and both modes over the five ladders, in two assignments
MIXES = {"a": (Pol(2, 0.4, "carry", None), Pol(256, 0.13, "frame", None), Pol(257, 0.0, "carry", None), Pol(513, 1.0, "frame", None), Pol(65, 0.13, "carry", (1, 1, 1, 1))),
         "b": (Pol(2, 0.13, "frame", None), Pol(256, 0.4, "carry", None), Pol(257, 1.0, "carry", None), Pol(513, 0.4, "carry", None), Pol(65, 0.0, "frame", (1, 1, 1, 1)))}
SLOT_POLICY = (3, 0, 4, 1, 2)   # slot s is bound to policy SLOT_POLICY[s]: no slot has its own index


# ------------------------------------------------------------------------------------------------------------------------ cases ---
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("mix", ["a", "b"])
def test_slots_equal_their_solo_pacers(pkg, ctx, mix, form):
    policies = MIXES[mix]
    calls = _schedule(5, list(range(5)))
    assert len(calls) == 10 and {len(c) for c in calls} >= {3, 4, 5} and len({tuple(s for s, _, _ in c) for c in calls}) == 10
    hist = _histories(calls)
    assert all({e[0] for e in hist[s]} == set(ORDER) for s in range(5))              # every slot met every geometry
    want = _references(pkg, ctx, hist, policies, SLOT_POLICY)
    with pkg.PacerSet(ctx, 5, policies=[_as_dict(p) for p in policies], slot_policy=SLOT_POLICY) as ps:
        assert ps.npolicies == 5 and len(ps) == 5 and [ps.policy_of(s) for s in range(5)] == list(SLOT_POLICY)
        _same(_run(pkg, ctx, ps, calls, form), want, "mix %s, %s form" % (mix, form))
        assert ps.launches == 2 * len(calls)
    flat = {s: [x[0] for x in want[s]] for s in want}
    zero = [s for s in range(5) if policies[SLOT_POLICY[s]].share == 0.0][0]
    assert all(x["over"] for x in flat[zero])                                        # nothing fits a budget of 0 ...
    full = [s for s in range(5) if policies[SLOT_POLICY[s]].share == 1.0][0]
    assert not any(x["over"] for x in flat[full])                                    # ... and rung 0 or better fits the full budget
    assert any(x["carry"] > 0 for s in range(5) if policies[SLOT_POLICY[s]].mode == "carry" for x in flat[s])
    assert all(x["carry"] == 0 for s in range(5) if policies[SLOT_POLICY[s]].mode == "frame" for x in flat[s])
    assert len({x["rung"] for s in range(5) for x in flat[s]}) > 5


@pytest.mark.parametrize("shortest", ["first", "last"])
def test_the_place_of_a_ladder_in_the_concatenation_changes_nothing(pkg, ctx, shortest):
    """the 2-rung ladder stands first in the policy table in one run and last in the other; its dead lanes (254 of a block's 256) must
    read and count inside its own two rows, beside neighbours of 513 and 65 rungs whichever side they are on"""
    base = sorted(MIXES["a"], key=lambda p: p.rungs, reverse=shortest == "last")
    assert base[0 if shortest == "first" else -1].rungs == 2
    slot_policy = [[p.rungs for p in base].index(MIXES["a"][i].rungs) for i in SLOT_POLICY]   # every slot keeps the POLICY it had above
    calls = _schedule(5, list(range(5)))
    want = _references(pkg, ctx, _histories(calls), base, slot_policy)
    with pkg.PacerSet(ctx, 5, policies=[_as_dict(p) for p in base], slot_policy=slot_policy) as ps:
        _same(_run_host(ps, calls), want, "the shortest ladder %s" % shortest)


def test_4097_rungs_beside_a_one_ctu_slot_under_two_rungs(pkg, ctx):
    """17 rung blocks a slice and 1 rung block in one launch"""
    policies = (Pol(4097, 0.4, "carry", None), Pol(2, 0.4, "carry", None))
    calls = [[(1, "edge", 0), (0, "one", 0)], [(0, "one", 1), (1, "edge", 1)], [(1, "edge", 2)], [(0, "one", 2)]]
    assert pkg.ethcnn.pacer_set_plan([4, 1], [4096, 1])["count_blocks"] == [17, 1]
    for slot_policy in ((1, 0), (0, 1)):                                             # the long ladder on the four CTUs, then on the one
        want = _references(pkg, ctx, _histories(calls), policies, slot_policy)
        with pkg.PacerSet(ctx, 2, policies=[_as_dict(p) for p in policies], slot_policy=slot_policy) as ps:
            _same(_run_host(ps, calls), want, "4097 rungs on slot %d" % slot_policy.index(0))


@pytest.mark.parametrize("form", ["host", "device"])
def test_bind_starts_a_fresh_pacer_of_the_new_policy_and_leaves_the_neighbours_alone(pkg, ctx, form):
    policies = (Pol(513, 0.4, "carry", None), Pol(2, 0.13, "frame", None), Pol(65, 0.13, "carry", (1, 1, 1, 1)))
    slot_policy = (0, 0, 2)
    calls = []
    for t in range(9):
        if t == 3:
            calls.append(("bind", 0, 1))                                             # from the 513-rung carry policy to the 2-rung frame policy ...
        if t == 6:
            calls.append(("bind", 0, 0))                                             # ... and back
        if t == 5:
            calls.append(("bind", 2, 2))                                             # to the policy it has: a reset
        call = [(1, "wide", t), (2, "long", t)]                                      # the neighbours: slot 1 carries under policy 0 all the way
        call.insert(t % 3, (0, ORDER[t % 4], t))
        calls.append(call)
    hist = _histories(calls)
    assert hist[0][3] == ("bind", 1) and hist[0][7] == ("bind", 0) and hist[2][5] == ("bind", 2) and len(hist[1]) == 9
    want = _references(pkg, ctx, hist, policies, slot_policy)
    with pkg.PacerSet(ctx, 3, policies=[_as_dict(p) for p in policies], slot_policy=slot_policy) as ps:
        _same(_run(pkg, ctx, ps, calls, form), want, "bind, %s form" % form)
        assert [ps.policy_of(s) for s in range(3)] == [0, 0, 2]
    assert [x[0]["frame"] for x in want[0]] == [0, 1, 2, 0, 1, 2, 0, 1, 2] and [x[0]["frame"] for x in want[2]] == [0, 1, 2, 3, 4, 0, 1, 2, 3]
    assert [x[0]["frame"] for x in want[1]] == list(range(9)) and sum(x[0]["carry"] > 0 for x in want[1]) >= 5
    assert all(x[0]["carry"] == 0 and x[0]["rung"] == 0 for x in want[0][3:6]) and any(x[0]["carry"] > 0 for x in want[0][:3] + want[0][6:])
    # binding to the policy a slot has IS a reset: the same run with a reset in its place gives the same
    again = [("reset", 2) if c == ("bind", 2, 2) else c for c in calls]
    assert _references(pkg, ctx, _histories(again), policies, slot_policy)[2] == want[2]
    with pkg.PacerSet(ctx, 3, policies=[_as_dict(p) for p in policies], slot_policy=slot_policy) as ps:
        _same(_run(pkg, ctx, ps, again, form), want, "a reset in place of the bind, %s form" % form)


def test_one_policy_through_the_new_entry_is_the_old_set(pkg, ctx):
    """the same schedule through ethcnn_pacer_set_create and through ethcnn_pacer_policies_create with that one policy"""
    calls = _schedule(11, list(range(5)))
    calls.insert(6, ("reset", 3))
    for p in (Pol(514, 0.4, "carry", None), Pol(65, 0.55, "frame", (7, 5, 3, 2))):
        d = _as_dict(p)
        with pkg.PacerSet(ctx, 5, p.share, p.mode, d["ladder"], p.weights) as old:
            want = _run_host(old, calls)
            assert old.npolicies == 1 and [old.policy_of(s) for s in range(5)] == [0] * 5      # a set of one policy bound to every slot
        with pkg.PacerSet(ctx, 5, policies=[d]) as new:
            _same(_run_host(new, calls), want, "one policy, host form")
        with pkg.PacerSet(ctx, 5, policies=[d], slot_policy=[0] * 5) as new:
            _same(_run_device(pkg, ctx, new, calls), want, "one policy, device form")
        _same(_references(pkg, ctx, _histories(calls), (p,), [0] * 5), want, "the old set against the references")


def test_refusals_leave_every_slot_as_it_was(pkg, ctx):
    """a refused frame on the slot of the heaviest weights beside valid frames, a bind of slot 32, a bind to policy -1.  (The cost bound
    itself, nctu x (w64 + 4 w32 + 16 w16 + 64 w8) < 2^64, cannot fail below 2^24 CTUs even under four weights of 2^32 - 1 -- (2^24 - 1) x 85 x
    (2^32 - 1) < 2^63 --, so the frame that is refused on that slot is one the size rules refuse: the refusal comes from the same per-frame
    check, under that slot's weights.)"""
    e = pkg.ethcnn
    lib = ctx.lib
    heavy = (0, 0, 0, 2 ** 32 - 1)
    policies = (Pol(514, 0.4, "carry", None), Pol(2, 0.9, "carry", heavy), Pol(65, 0.13, "carry", (1, 1, 1, 1)))
    slot_policy = [0] * 32
    slot_policy[1], slot_policy[31] = 1, 2
    calls = [[(0, "edge", t), (1, "wide", t), (31, "long", t)] for t in range(4)]
    want = _references(pkg, ctx, _histories(calls), policies, slot_policy)
    assert max(x[0]["full"] for x in want[1]) * M >= 2 ** 64                         # that slot's allowance is past 64 bits
    nbytes = 272 * 84
    dev = ctx.alloc(3 * nbytes + 128)
    fill = np.full(3 * nbytes + 128, 0xEE, np.uint8)
    dev.upload(fill)
    at = lambda i: dev.ptr + 64 + i * nbytes
    F = e.PacerSetFrame
    with pytest.raises(pkg.EthCnnError) as err:
        pkg.PacerSet(ctx, 4, policies=[_as_dict(policies[0]), dict(_as_dict(policies[1]), weights=(1, 2, 3, 2 ** 32))])
    assert err.value.code == e.ERR_ARG and "policy 1: " in str(err.value)
    for bad in (dict(policies=[]), dict(policies=[_as_dict(policies[0])] * 33), dict(policies=[_as_dict(policies[0])], slot_policy=[0, 0, 1, 0])):
        with pytest.raises(pkg.EthCnnError) as err:
            pkg.PacerSet(ctx, 4, **bad)
        assert err.value.code == e.ERR_ARG
    with pkg.PacerSet(ctx, 32, policies=[_as_dict(p) for p in policies], slot_policy=slot_policy) as ps:
        got = _run_host(ps, calls[:2])
        before = ps.launches
        for frames, text in (([F(0, at(0), 72, 72, at(0), None), F(1, at(1), 1092, 1024, at(1), None), F(31, at(2), 4160, 64, at(2), None)], "1092"),
                             ([F(1, at(1), 1088, 65544, at(1), None), F(0, at(0), 72, 72, at(0), None)], "65544")):
            arr = (F * len(frames))(*frames)
            for entry in (lib.ethcnn_pacer_set_frames_device, lib.ethcnn_pacer_set_frames):
                assert entry(ps.h, arr, len(frames)) == e.ERR_ARG
                assert text in lib.ethcnn_last_error(ctx.h).decode()
        assert lib.ethcnn_pacer_policies_bind(ps.h, 32, 0) == e.ERR_ARG and "slot 32" in lib.ethcnn_last_error(ctx.h).decode()
        assert lib.ethcnn_pacer_policies_bind(ps.h, 1, -1) == e.ERR_ARG and "policy -1" in lib.ethcnn_last_error(ctx.h).decode()
        assert lib.ethcnn_pacer_policies_bind(ps.h, 1, 3) == e.ERR_ARG and lib.ethcnn_pacer_policies_bind(ps.h, -1, 0) == e.ERR_ARG
        assert lib.ethcnn_pacer_policies_of(ps.h, 32) == e.ERR_ARG
        with pytest.raises(pkg.EthCnnError):
            ps.bind(32, 0)
        assert ps.launches == before                                                 # nothing was enqueued ...
        assert (dev.download(np.uint8, fill.size) == 0xEE).all()                     # ... and nothing written
        assert [ps.policy_of(s) for s in (0, 1, 31)] == [0, 1, 2]                    # ... and nothing bound
        for s in (0, 1, 31):
            assert _fields(ps.last(s)) == got[s][-1][0]
        for s, v in _run_host(ps, calls[2:]).items():                                # the next frames give what they would have given
            got[s] += v
        _same(got, want, "after the refusals")
    dev.free()


@pytest.mark.parametrize("n", [1, 4, 16])
def test_a_round_of_mixed_policies_is_two_launches(pkg, ctx, n):
    policies = (Pol(2, 0.4, "carry", None), Pol(4097, 0.4, "frame", None), Pol(514, 0.13, "carry", None), Pol(65, 0.4, "carry", (1, 1, 1, 1)))
    name = "edge"
    per = _per(name)
    dev = ctx.alloc(n * per * 84)
    try:
        dev.upload(np.ascontiguousarray(np.concatenate([_case(name)[0][j % FRAMES] for j in range(n)])))
        with pkg.PacerSet(ctx, 16, policies=[_as_dict(p) for p in policies], slot_policy=[s % 4 for s in range(16)]) as ps:
            assert ps.launches == 0
            frames = [{"slot": (5 * j) % 16, "d_probs": dev.ptr + j * per * 84, "width": 72, "height": 72, "d_baked": dev.ptr + j * per * 84} for j in range(n)]
            assert n == 1 or len({ps.policy_of(f["slot"]) for f in frames}) == 4
            for rounds in (1, 2):
                ps.frames_device(frames)
                assert ps.launches == 2 * rounds
            ps.bind(frames[0]["slot"], 1)                                            # (memsets: no kernel)
            assert ps.launches == 4
            ctx.synchronize()
            assert [int(ps.last(f["slot"])["frame"]) for f in frames[1:]] == [1] * (n - 1)
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------- server ---
def _workdir(path):
    os.makedirs(path)
    open(os.path.join(path, "Thr_info.txt"), "w").write("0.25 0.75 0.25 0.75 0.25 0.75\n")
    for ext in (".index", ".data-00000-of-00001"):
        shutil.copy(GOLD + ext, os.path.join(path, "model_LDP_200000_qp32.dat" + ext))  # QP 32: the real bundle; QP 22 and 37: seeded
    return path


def test_one_server_paces_three_directories_under_three_policies(tmp_path):
    """`--sessions ... --budget-policies FILE` with a dir= line, a qp= line and * against three solo daemons, each under
    ETHCNN_SEARCH_BUDGET* set to its directory's policy: per-frame cu_depth.dat digests and state.dat files are equal"""
    jobs = [(416, 240, 22, 11), (416, 240, 37, 12), (128, 72, 32, 13)]   # width, height, QP, the client's seed
    frames = 3
    ladder = str(tmp_path / "ladder9.txt")   # nine rungs in Low-Delay-P token order (down up ...), the most thorough first
    open(ladder, "w").write("".join("%g %g %g %g %g %g\n" % ((j / 18.0, 1 - j / 18.0) * 3) for j in range(9)))
    solo = [_workdir(str(tmp_path / ("solo%d" % k))) for k in range(3)]
    many = [_workdir(str(tmp_path / ("many%d" % k))) for k in range(3)]
    # directory 0 by its dir= line (its QP 22 is in the qp= range too: dir wins), directory 2 by its QP, directory 1 by *
    policy_file = str(tmp_path / "policies.txt")
    open(policy_file, "w").write("# three ways to a policy\nqp=20..34 0.5 frame\n* 0.7 carry - 8 4 2 1\ndir=%s 0.3 carry %s   # its own ladder\n" % (many[0], ladder))
    own = [dict(ETHCNN_SEARCH_BUDGET="0.3", ETHCNN_SEARCH_BUDGET_MODE="carry", ETHCNN_SEARCH_BUDGET_LADDER=ladder),
           dict(ETHCNN_SEARCH_BUDGET="0.7", ETHCNN_SEARCH_BUDGET_MODE="carry", ETHCNN_SEARCH_BUDGET_WEIGHTS="8 4 2 1"),
           dict(ETHCNN_SEARCH_BUDGET="0.5", ETHCNN_SEARCH_BUDGET_MODE="frame")]
    plain = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    plain.update(ETHCNN_SYNTHETIC_SEED="21")
    client = os.path.join(BIN, "ldp_client")
    daemon = lambda args, cwd, env, out=subprocess.DEVNULL: subprocess.Popen([sys.executable, LAUNCHER] + args + ["--idle-timeout", "120"], cwd=cwd, env=env,
                                                                             stdout=out, stderr=subprocess.PIPE, text=True)
    start = lambda dirs: [subprocess.Popen([client, d, str(w), str(h), str(qp), str(frames), "--seed", str(seed), "--digest", os.path.join(d, "digest.txt")],
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for d, (w, h, qp, seed) in zip(dirs, jobs)]
    daemons = [daemon(["--python", "--max-frames", str(frames)], d, dict(plain, **env)) for d, env in zip(solo, own)]
    clients = []
    try:
        clients += start(solo) + start(many)
        deadline = time.monotonic() + 60
        while not all(os.path.exists(os.path.join(d, "pred_start.sig")) for d in many):
            assert time.monotonic() < deadline and all(c.poll() is None for c in clients[3:]), "the clients did not reach their first handshake"
            time.sleep(0.001)
        server = daemon(["--sessions"] + many + ["--max-frames", str(3 * frames), "--budget-policies", policy_file], str(tmp_path), plain, subprocess.PIPE)
        daemons.append(server)
        said, err = server.communicate(timeout=240)
        assert server.returncode == 0, err[-800:]
        for c in clients:
            assert c.wait(timeout=240) == 0, c.stderr.read()[-500:]
        solo_err = []
        for d in daemons[:3]:
            assert d.wait(timeout=120) == 0, d.stderr.read()[-800:]
            solo_err.append(d.stderr.read())
    finally:
        for p in clients + daemons:
            if p.poll() is None:
                p.kill()
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    shares = [("0.3", "carry"), ("0.7", "carry"), ("0.5", "frame")]
    for k in range(3):
        want = open(os.path.join(solo[k], "digest.txt")).read()
        assert len(want.splitlines()) == frames
        assert open(os.path.join(many[k], "digest.txt")).read() == want, "directory %d: per-frame cu_depth.dat digests differ" % k
        assert md5(os.path.join(many[k], "cu_depth.dat")) == md5(os.path.join(solo[k], "cu_depth.dat")), "directory %d: cu_depth.dat differs" % k
        assert md5(os.path.join(many[k], "state.dat")) == md5(os.path.join(solo[k], "state.dat")), "directory %d: state.dat differs" % k
        assert set(np.unique(np.fromfile(os.path.join(many[k], "cu_depth.dat"), "<f4")).tolist()) <= {0.0, 0.5, 1.0}
        # the per-frame lines and the summary carry the directory's own share and mode; the summary's figures are the solo daemon's
        lines = [ln for ln in said.splitlines() if ln.startswith(many[k] + ": frame ") and " of the full search" in ln]
        assert len(lines) == frames and all(ln.endswith("(budget %s, %s)" % shares[k]) for ln in lines), lines
        tail = [ln.split("search budget", 1)[1] for ln in solo_err[k].splitlines() if "search budget" in ln]
        mine = [ln.split("search budget", 1)[1] for ln in err.splitlines() if ln.startswith("resi_to_cu_depth_LDP: %s: search budget" % many[k])]
        assert len(tail) == 1 and mine == tail and tail[0].startswith(" %s (%s):" % shares[k]), (k, mine, tail)
