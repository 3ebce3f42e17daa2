"""-m gpu: the pacer set (include/ethcnn.h "search budget, online: several sequences") on the GPU against its defining equality: slot by
slot, every result field and every baked word are those of a sequence of its own, whatever shared the calls.  Two references, both fed
the slot's frames and resets in order:
  reference 1  a solo pacer (pkg.Pacer) per slot -- the kernel this one generalises;
  reference 2  the numpy restatement (tests/budget_ref.py: checks per rung, the choice in Python integers, the baked rows), which
               shares nothing with any kernel.
The references are compared with each other first; a disagreement between them is reported as such.  Inputs are built as in
tests/test_gpu_pacer.py: seeded probabilities on the k / 1024 grid over [0, 1], values exactly at up / down of several rungs, a spread that
differs per frame so that the picked rungs differ.  Integers and three float constants only: every comparison is equality."""
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
ERR_ARG = -1
MODES = {"frame": bref.FRAME, "carry": bref.CARRY}
M = 10 ** 6
# name: width, height, frames, CTUs that are rejected (a NaN in the first, a 1.5 in the second)
SHAPES = {"one": (64, 64, 10, None),        # 1 CTU
          "ragged": (200, 136, 10, None),   # 12 CTUs, partial right and bottom edges
          "wide": (1088, 1024, 10, None),   # 272 CTUs: five slices, so a segment's ticket counts several blocks
          "bad": (200, 136, 4, (3, 7))}
_CASES, _LADDERS, _CHECKED, _BAKED = {}, {}, {}, {}


def _per(name):
    w, h = SHAPES[name][:2]
    return ((w + 63) // 64) * ((h + 63) // 64)


def _case(name):
    """(probs [F, per, 21], one sim_ref.Set per frame) made once and never changed"""
    if name not in _CASES:
        w, h, frames, bad = SHAPES[name]
        per = _per(name)
        rng = np.random.default_rng(sum(map(ord, name)) + 1000)
        k = rng.integers(0, 1025, size=(frames, per, 21))
        spread = np.linspace(0.05, 1.0, frames)[rng.permutation(frames)]           # frames near 0.5 are dear, spread-out frames cheap
        k = 512 + np.rint((k - 512) * spread[:, None, None]).astype(np.int64)
        at_rung = rng.choice(np.array([1024 - 100, 99, 1024 - 300, 299, 512, 511, 1024, 0, 768, 256]), size=k.shape)
        k = np.where(rng.integers(0, 6, size=k.shape) == 0, at_rung, k)             # exactly at up / down of rungs 100, 300, 512, 0
        probs = (k / 1024.0).astype(np.float32)
        if bad is not None:
            probs[:, bad[0], 7] = np.nan
            probs[:, bad[1], 20] = 1.5
        sets = []
        for f in range(frames):
            s = ref.Set()
            s.add_frames(probs[f], None, w, h, 0)
            sets.append(s)
        probs.setflags(write=False)
        _CASES[name] = (probs, sets)
    return _CASES[name]


def _ladder(k):
    if k not in _LADDERS:
        # (2: the full search and the cheapest rung of the default ladder, so that a frame leaves a large remainder)
        _LADDERS[k] = bref.default_ladder() if k == 513 else bref.default_ladder()[[0, 512]].copy() if k == 2 else dref.candidates(np.random.default_rng(k), max(k, 4))[:k].copy()
    return _LADDERS[k]


def _fields(res):
    return {"frame": int(res["frame"]), "rung": int(res["rung"]), "over": int(res["over"]), "cost": int(res["cost"]), "full": int(res["full"]),
            "carry": int(res["carry_lo"]) | int(res["carry_hi"]) << 64, "up_k": res["up_k"].tolist(), "down_k": res["down_k"].tolist()}


# ------------------------------------------------------------------------------------------------------------ the two references ---
# a slot's history is a list of events: (name, f) = frame f of case `name`, or "reset"
def _restated(events, k, weights, ppm, mode):
    """reference 2: the choice rule of "search budget" in Python integers over the restated checks, the carry kept across frames and
    geometries, the baked rows of the picked rung -> [(fields, baked bytes)]"""
    ladder, weights = _ladder(k), weights or bref.WEIGHTS
    out, carry, count = [], 0, 0
    for ev in events:
        if ev == "reset":
            carry, count = 0, 0
            continue
        name, f = ev
        s = _case(name)[1][f]
        if (name, f, k) not in _CHECKED:
            _CHECKED[name, f, k] = bref.cost(s, ladder, 0, _per(name), 1)[0]
        costs = [sum(int(w) * int(x) for w, x in zip(weights, c)) for c in _CHECKED[name, f, k]]
        full = costs[-1]
        allow = ppm * full + carry
        fits = [i for i in range(len(costs) - 1) if costs[i] * M <= allow]
        at = fits[0] if fits else min(range(len(costs) - 1), key=lambda i: (costs[i], i))
        carry = allow - costs[at] * M if fits and mode == "carry" else 0
        if (name, f, k, at) not in _BAKED:
            _BAKED[name, f, k, at] = bref.bake(s, ladder, [at], 0, _per(name), 1).tobytes()
        out.append(({"frame": count, "rung": at, "over": 0 if fits else 1, "cost": costs[at], "full": full, "carry": carry,
                     "up_k": ladder[at]["up_k"].tolist(), "down_k": ladder[at]["down_k"].tolist()}, _BAKED[name, f, k, at]))
        count += 1
    return out


def _solo(pkg, ctx, events, k, weights, share, mode):
    """reference 1: the slot's history through a pacer of its own -> [(fields, baked bytes)]"""
    out = []
    with pkg.Pacer(ctx, share, mode, None if k == 513 else _ladder(k), weights) as pacer:
        for ev in events:
            if ev == "reset":
                pacer.reset()
                continue
            name, f = ev
            baked, res = pacer.frame(_case(name)[0][f], *SHAPES[name][:2])
            out.append((_fields(res), baked.tobytes()))
    return out


def _references(pkg, ctx, histories, k, weights, share, mode):
    """{slot: [(fields, baked bytes)]} on which both references agree"""
    want = {}
    for slot, events in histories.items():
        one, two = _solo(pkg, ctx, events, k, weights, share, mode), _restated(events, k, weights, int(round(share * 1e6)), mode)
        assert [x[0] for x in one] == [x[0] for x in two], "the two REFERENCES disagree on the results of slot %d (k %d, %s, %g)" % (slot, k, mode, share)
        assert [x[1] for x in one] == [x[1] for x in two], "the two REFERENCES disagree on the baked rows of slot %d (k %d, %s, %g)" % (slot, k, mode, share)
        want[slot] = one
    return want


def _histories(calls):
    """the calls of a run -- lists of (slot, name, f), or ("reset", slot) -- as one history per slot"""
    out = {}
    for call in calls:
        if call[0] == "reset":
            out.setdefault(call[1], []).append("reset")
        else:
            for slot, name, f in call:
                out.setdefault(slot, []).append((name, f))
    return out


def _run_host(ps, calls):
    """the calls through PacerSet.frames (pageable arrays: the staged route) -> {slot: [(fields, baked bytes)]}"""
    got = {}
    for call in calls:
        if call[0] == "reset":
            ps.reset(call[1])
            continue
        baked, results = ps.frames([{"slot": slot, "probs": _case(name)[0][f], "width": SHAPES[name][0], "height": SHAPES[name][1]} for slot, name, f in call])
        for (slot, name, f), b, r in zip(call, baked, results):
            assert b.shape == (_per(name), 21)
            got.setdefault(slot, []).append((_fields(r), b.tobytes()))
    return got


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for slot in sorted(want):
        assert [x[0] for x in got[slot]] == [x[0] for x in want[slot]], "%s: the results of slot %d differ" % (what, slot)
        for n, (g, w) in enumerate(zip(got[slot], want[slot])):
            assert g[1] == w[1], "%s: slot %d, its frame %d: %d baked words differ" % (
                what, slot, n, int((np.frombuffer(g[1], "<u4") != np.frombuffer(w[1], "<u4")).sum()))


def _schedule(seed, slots, frames=10):
    """calls that name changing subsets of the slots in permuted order until every slot has had `frames` frames"""
    rng = np.random.default_rng(seed)
    done, calls = {s: 0 for s in slots}, []
    while any(n < frames for n in done.values()):
        live = [s for s in slots if done[s] < frames]
        pick = [s for s in live if rng.integers(0, 3) > 0] or [live[int(rng.integers(0, len(live)))]]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        calls.append([(s, slots[s], done[s]) for s in pick])
        for s in pick:
            done[s] += 1
    return calls


# ------------------------------------------------------------------------------------------------------------------------ cases ---
@pytest.mark.parametrize("k", [513, 1, 65])
def test_mixed_table_equals_both_references(pkg, ctx, k):
    """1, 12 and 272 CTUs side by side; the default ladder is three rung blocks, 272 CTUs are five slices"""
    slots = {4: "one", 0: "ragged", 2: "wide"}
    seen = {"over": 0, "deep": 0, "carry": 0, "sizes": set(), "orders": set()}
    for mode in ("frame", "carry"):
        for share in (0.4, 0.0):
            calls = _schedule(k + len(mode), slots)
            seen["sizes"] |= {len(c) for c in calls}
            seen["orders"] |= {tuple(s for s, _, _ in c) for c in calls if len(c) == 3}
            want = _references(pkg, ctx, _histories(calls), k, None, share, mode)
            with pkg.PacerSet(ctx, 5, share, mode, None if k == 513 else _ladder(k)) as ps:
                got = _run_host(ps, calls)
            _same(got, want, "k %d, %s, %g" % (k, mode, share))
            flat = [x[0] for v in want.values() for x in v]
            seen["over"] += sum(x["over"] for x in flat)
            seen["deep"] += sum(x["rung"] > 0 for x in flat)
            seen["carry"] += sum(x["carry"] > 0 for x in flat)
            if share == 0.4 and k == 513:
                assert len({x[0]["rung"] for x in want[2]}) > 3   # frames of different spread take different rungs
    assert seen["sizes"] == {1, 2, 3} and len(seen["orders"]) > 1       # the subsets changed, and so did the order
    assert seen["over"] and (k == 1 or (seen["deep"] and seen["carry"]))


def test_4096_rungs_beside_a_one_ctu_slot(pkg, ctx):
    """17 rung blocks a slice"""
    calls = [[(1, "ragged", 0), (0, "one", 0)], [(0, "one", 1), (1, "ragged", 1)], [(1, "ragged", 2)]]
    assert pkg.ethcnn.pacer_set_plan([12, 1], 4096)["count_blocks"] == [17, 17]
    want = _references(pkg, ctx, _histories(calls), 4096, None, 0.4, "carry")
    with pkg.PacerSet(ctx, 2, 0.4, "carry", _ladder(4096)) as ps:
        _same(_run_host(ps, calls), want, "4096 rungs")


def test_the_full_table_twice_in_a_row(pkg, ctx):
    calls = [[(s, "one", (s + 3 * c) % 10) for s in range(32)] for c in range(2)]
    calls[1].reverse()
    want = _references(pkg, ctx, _histories(calls), 513, None, 0.4, "carry")
    with pkg.PacerSet(ctx, 32, 0.4, "carry") as ps:
        assert len(ps) == 32
        _same(_run_host(ps, calls), want, "32 slots")
    assert len({x[0]["rung"] for v in want.values() for x in v}) > 3


def test_a_reset_a_rejected_ctu_and_a_change_of_geometry_leave_the_neighbours_alone(pkg, ctx):
    calls = []
    for t in range(6):
        call = [(1, "ragged", 9 - t), (3, "wide", t % 3)]                       # the neighbours: two slots that carry all the way
        if t == 3:
            calls.append(("reset", 0))                                           # slot 0 starts again in the middle
        call.insert(t % 3, (0, "ragged", t))
        call.insert(t % 2, (2,) + (("one", t) if t < 2 else ("bad", t - 2) if t < 5 else ("wide", 5)))   # 64x64, then 200x136 with a NaN and a 1.5, then 1088x1024
        calls.append(call)
    hist = _histories(calls)
    assert hist[0][3] == "reset" and [e[0] for e in hist[2]] == ["one", "one", "bad", "bad", "bad", "wide"]
    k, weights = 65, (7, 5, 3, 2)
    want = _references(pkg, ctx, hist, k, weights, 0.55, "carry")
    with pkg.PacerSet(ctx, 4, 0.55, "carry", _ladder(k), weights) as ps:
        _same(_run_host(ps, calls), want, "independence")
    for slot in (1, 3):
        assert sum(x[0]["carry"] > 0 for x in want[slot]) >= 3, slot            # they did carry across the others' events
    assert [x[0]["frame"] for x in want[0]] == [0, 1, 2, 0, 1, 2]
    assert want[2][1][0]["carry"] > 0 or want[2][4][0]["carry"] > 0             # slot 2 took a carry into another geometry
    rows = np.frombuffer(want[2][2][1], "<f4").reshape(12, 21)
    assert (rows[3] == 0.5).all() and (rows[7] == 0.5).all()                     # a rejected CTU gets the full search


def test_eight_calls_queued_back_to_back_in_place(pkg, ctx):
    """frames_device without a host wait in between: per-frame result slots, guard words around every d_baked, d_baked == d_probs"""
    slots = {0: "one", 5: "ragged", 3: "wide"}
    rounds, guard, size = 8, 64, pkg.ethcnn.PACER_RESULT.itemsize
    rng = np.random.default_rng(3)
    calls = [[(s, slots[s], t) for s in (sorted(slots) if t % 2 else sorted(slots, reverse=True)) if not (t == 2 and s == 5)] for t in range(rounds)]
    calls[4] = [calls[4][i] for i in rng.permutation(len(calls[4]))]
    want = _references(pkg, ctx, _histories(calls), 513, None, 0.4, "carry")
    bufs, host = {}, {}
    d_res = ctx.alloc(len(slots) * rounds * size + 16)
    try:
        for s, name in slots.items():
            stride = _per(name) * 84 + 2 * guard
            raw = np.full(rounds * stride, 0xAB, np.uint8)
            for t in range(rounds):
                raw[t * stride + guard:(t + 1) * stride - guard] = np.frombuffer(_case(name)[0][t].tobytes(), np.uint8)
            bufs[s] = ctx.alloc(raw.size)
            bufs[s].upload(raw)
            host[s] = raw
        d_res.upload(np.full(len(slots) * rounds * size + 16, 0xCD, np.uint8))
        order = sorted(slots)
        with pkg.PacerSet(ctx, 6, 0.4, "carry") as ps:
            for call in calls:
                frames = []
                for s, name, t in call:
                    at = bufs[s].ptr + t * (_per(name) * 84 + 2 * guard) + guard
                    frames.append({"slot": s, "d_probs": at, "width": SHAPES[name][0], "height": SHAPES[name][1], "d_baked": at,
                                   "d_result": d_res.ptr + 8 + (order.index(s) * rounds + t) * size})
                ps.frames_device(frames)
            ctx.synchronize()
            last = {s: _fields(ps.last(s)) for s in slots}
        res = d_res.download(np.uint8, len(slots) * rounds * size + 16)
        out = {s: bufs[s].download(np.uint8, host[s].size) for s in slots}
    finally:
        for b in list(bufs.values()) + [d_res]:
            b.free()
    assert (res[:8] == 0xCD).all() and (res[-8:] == 0xCD).all()
    records = res[8:-8].view(pkg.ethcnn.PACER_RESULT).reshape(len(slots), rounds)
    for s, name in slots.items():
        stride = _per(name) * 84 + 2 * guard
        mine = [t for t in range(rounds) if any(x[0] == s for x in calls[t])]
        assert [_fields(records[order.index(s), t]) for t in mine] == [x[0] for x in want[s]], s
        assert last[s] == want[s][-1][0]
        for n, t in enumerate(mine):
            frame = out[s][t * stride:(t + 1) * stride]
            assert (frame[:guard] == 0xAB).all() and (frame[-guard:] == 0xAB).all(), (s, t)
            assert frame[guard:-guard].tobytes() == want[s][n][1], (s, t)
        for t in set(range(rounds)) - set(mine):   # a frame no call named: its bytes and its result slot are as uploaded
            assert out[s][t * stride:(t + 1) * stride].tobytes() == host[s][t * stride:(t + 1) * stride].tobytes()
            assert (records[order.index(s), t].tobytes() == b"\xcd" * size)


def test_one_slot_carries_past_64_bits_beside_one_that_stays_small(pkg, ctx):
    weights = (2 ** 32 - 1,) * 4
    calls = [[(0, "wide", t), (1, "one", t)] if t % 2 else [(1, "one", t), (0, "wide", t)] for t in range(6)]
    want = _references(pkg, ctx, _histories(calls), 2, weights, 0.9, "carry")
    with pkg.PacerSet(ctx, 2, 0.9, "carry", _ladder(2), weights) as ps:
        _same(_run_host(ps, calls), want, "128-bit carry")
    assert max(x[0]["carry"] for x in want[0]) >= 2 ** 64 and max(x[0]["cost"] for x in want[0]) * M >= 2 ** 64
    assert 0 < max(x[0]["carry"] for x in want[1]) < 2 ** 64


def test_in_place_and_staged_routes_in_one_call(pkg):
    with pkg.EthCnn(device=0) as own:   # (a context of its own: its page-locked buffer goes with it)
        _routes(pkg, own)


def _routes(pkg, ctx):
    """slot 0: page-locked input, pageable output; slot 1: pageable input, page-locked output; slot 2: page-locked, in place; slot 3:
    pageable, in place -- all four in every call"""
    name, frames = "ragged", 5
    probs = _case(name)[0]
    w, h = SHAPES[name][:2]
    per = _per(name)
    calls = [[(s, name, (t + 2 * s) % 10) for s in ((0, 1, 2, 3) if t % 2 else (3, 1, 0, 2))] for t in range(frames)]
    want = _references(pkg, ctx, _histories(calls), 513, None, 0.4, "carry")
    pinned = ctx.host_buffer(3 * (per * 84 + 16) + 16).view(np.float32)
    pins = [pinned[4 + i * (per * 21 + 4):4 + i * (per * 21 + 4) + per * 21].reshape(per, 21) for i in range(3)]
    got = {}
    with pkg.PacerSet(ctx, 4, 0.4, "carry") as ps:
        with pytest.raises(pkg.EthCnnError):
            ps.last(2)                      # nothing paced yet
        for call in calls:
            pinned[:] = 7.25
            arrays = {}
            for s, _, f in call:
                src = probs[f].copy()
                if s == 0:
                    pins[0][:] = src
                    arrays[s] = {"probs": pins[0]}
                elif s == 1:
                    arrays[s] = {"probs": src, "out": pins[1]}
                elif s == 2:
                    pins[2][:] = src
                    arrays[s] = {"probs": pins[2], "out": pins[2]}
                else:
                    arrays[s] = {"probs": src, "out": src}
            baked, results = ps.frames([dict(arrays[s], slot=s, width=w, height=h) for s, _, _ in call])
            for (s, _, f), b, r in zip(call, baked, results):
                got.setdefault(s, []).append((_fields(r), b.tobytes()))
                assert _fields(ps.last(s)) == _fields(r)
            assert pins[0].tobytes() == probs[dict((s, f) for s, _, f in call)[0]].tobytes()      # an input that is not in place stays
            gaps = np.ones(pinned.size, bool)
            for i in range(3):
                gaps[4 + i * (per * 21 + 4):4 + i * (per * 21 + 4) + per * 21] = False
            assert (pinned[gaps] == 7.25).all()
        _same(got, want, "routes")
        ps.reset(1)
        with pytest.raises(pkg.EthCnnError):
            ps.last(1)
        assert _fields(ps.last(0)) == want[0][-1][0]


def test_refusals_leave_every_slot_as_it_was(pkg, ctx):
    e = pkg.ethcnn
    lib = ctx.lib
    calls = [[(0, "ragged", t), (1, "one", t), (31, "ragged", 9 - t)] for t in range(4)]
    want = _references(pkg, ctx, _histories(calls), 513, None, 0.4, "carry")
    per, w, h = _per("ragged"), 200, 136
    nbytes = per * 84
    dev = ctx.alloc(4 * nbytes + 128)
    fill = np.full(4 * nbytes + 128, 0xEE, np.uint8)
    dev.upload(fill)
    at = lambda i: dev.ptr + 64 + i * nbytes
    F = e.PacerSetFrame
    good = [F(0, at(0), w, h, at(0), None), F(2, at(1), w, h, at(2), None)]
    with pytest.raises(ValueError):
        pkg.PacerSet(ctx, 4, 1.5)
    with pytest.raises(ValueError):
        pkg.PacerSet(ctx, 4, 0.4, "both")
    for bad in (dict(nslots=0), dict(nslots=33), dict(ladder=np.resize(bref.default_ladder(), 4097)), dict(weights=(1, 2, 3, 2 ** 32))):
        with pytest.raises(pkg.EthCnnError) as err:
            pkg.PacerSet(ctx, bad.pop("nslots", 4), 0.4, "frame", **bad)
        assert err.value.code == e.ERR_ARG
    with pkg.PacerSet(ctx, 32, 0.4, "carry") as ps:
        got = _run_host(ps, calls[:2])
        before = ps.launches

        def refused(frames, n, text):
            arr = (F * max(len(frames), 1))(*frames)
            for entry in (lib.ethcnn_pacer_set_frames_device, lib.ethcnn_pacer_set_frames):
                assert entry(ps.h, arr, n) == e.ERR_ARG, text
                assert text in lib.ethcnn_last_error(ctx.h).decode(), (text, lib.ethcnn_last_error(ctx.h).decode())

        refused([good[0], F(0, at(1), w, h, at(2), None)], 2, "slot 0 is named by frames 0 and 1")
        refused([good[0], F(32, at(1), w, h, at(2), None)], 2, "slot 32")
        refused([F(-1, at(1), w, h, at(2), None)], 1, "slot -1")
        refused(good, 0, "0 frames")
        refused([good[0]] * 33, 33, "33 frames")
        refused([good[0], F(2, None, w, h, at(2), None)], 2, "frame 1: null")
        refused([good[0], F(2, at(1), w, h, None, None)], 2, "frame 1: null")
        refused([good[0], F(2, at(1) + 2, w, h, at(2), None)], 2, "not 4-byte aligned")
        refused([good[0], F(2, at(1), w, h, at(2) + 2, None)], 2, "not 4-byte aligned")
        refused([F(0, at(0), w, h, at(3), None), F(2, at(1), w, h, at(0) + 84, None)], 2, "the output of frame 1 overlaps a buffer of frame 0")   # another's probs
        refused([F(0, at(0), w, h, at(3), None), F(2, at(1), w, h, at(3) - 4, None)], 2, "overlaps")                        # another's baked alone
        refused([F(0, at(0), w, h, at(1) + 4, None), F(2, at(1), w, h, at(2), None)], 2, "the output of frame 0 overlaps a buffer of frame 1")
        refused([good[0], F(2, at(1), 204, h, at(2), None)], 2, "204")
        refused([good[0], F(2, at(1), w, 65544, at(2), None)], 2, "65544")
        assert lib.ethcnn_pacer_set_frames_device(ps.h, None, 1) == e.ERR_ARG and lib.ethcnn_pacer_set_reset(ps.h, 32) == e.ERR_ARG
        assert lib.ethcnn_pacer_set_last(ps.h, 32, np.zeros(72, np.uint8).ctypes.data) == e.ERR_ARG
        assert lib.ethcnn_pacer_set_frames_device(ps.h, (F * 1)(F(0, at(0), w, h, at(0), at(3) + 2)), 1) == e.ERR_ARG      # a misaligned d_result
        assert ps.launches == before                                           # nothing was enqueued ...
        assert (dev.download(np.uint8, fill.size) == 0xEE).all()               # ... and nothing written
        for s in (0, 1, 31):
            assert _fields(ps.last(s)) == got[s][-1][0]
        with pytest.raises(pkg.EthCnnError):
            ps.last(2)                                                         # the refused calls left slot 2 without a frame
        for s, v in _run_host(ps, calls[2:]).items():                          # the next frames give what they would have given
            got[s] += v
        _same(got, want, "after the refusals")
    dev.free()
    with pytest.raises(ValueError):
        ps.frames([{"slot": 0, "probs": _case("one")[0][0], "width": 64, "height": 64}])   # a closed set
    own = pkg.EthCnn(device=0)   # a set goes before its context: closing the context closes it
    mine = pkg.PacerSet(own, 2, 0.4)
    own.close()
    assert mine.h is None


@pytest.mark.parametrize("n", [1, 4, 16])
def test_a_round_is_two_launches(pkg, ctx, n):
    """whatever the number of frames: counted by the set, which adds what it enqueues where it enqueues it"""
    name = "ragged"
    per = _per(name)
    dev = ctx.alloc(n * per * 84)
    try:
        dev.upload(np.ascontiguousarray(np.concatenate([_case(name)[0][j % 10] for j in range(n)])))
        with pkg.PacerSet(ctx, 16, 0.4, "carry") as ps:
            assert ps.launches == 0
            frames = [{"slot": (5 * j) % 16, "d_probs": dev.ptr + j * per * 84, "width": 200, "height": 136, "d_baked": dev.ptr + j * per * 84} for j in range(n)]
            for rounds in (1, 2):
                ps.frames_device(frames)
                assert ps.launches == 2 * rounds
            ctx.synchronize()
            assert [int(ps.last(f["slot"])["frame"]) for f in frames] == [1] * n
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------- server ---
def _workdir(path):
    os.makedirs(path)
    open(os.path.join(path, "Thr_info.txt"), "w").write("0.25 0.75 0.25 0.75 0.25 0.75\n")
    for ext in (".index", ".data-00000-of-00001"):
        shutil.copy(GOLD + ext, os.path.join(path, "model_LDP_200000_qp32.dat" + ext))  # QP 32: the real bundle; QP 22: seeded
    return path


def test_one_paced_server_for_three_directories(tmp_path):
    """`--sessions ... --budget 0.4 --budget-mode carry` against three solo daemons under ETHCNN_SEARCH_BUDGET=0.4 and
    ETHCNN_SEARCH_BUDGET_MODE=carry: per-frame cu_depth.dat digests and state.dat files are equal"""
    jobs = [(416, 240, 22, 11), (416, 240, 32, 12), (200, 136, 32, 13)]  # width, height, QP, the client's seed
    frames = 5
    plain = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_SEARCH_BUDGET")}
    plain.update(ETHCNN_SYNTHETIC_SEED="21")
    paced = dict(plain, ETHCNN_SEARCH_BUDGET="0.4", ETHCNN_SEARCH_BUDGET_MODE="carry")
    client = os.path.join(BIN, "ldp_client")
    solo = [_workdir(str(tmp_path / ("solo%d" % k))) for k in range(3)]
    many = [_workdir(str(tmp_path / ("many%d" % k))) for k in range(3)]
    daemon = lambda args, cwd, env, out=subprocess.DEVNULL: subprocess.Popen([sys.executable, LAUNCHER] + args + ["--idle-timeout", "120"], cwd=cwd, env=env,
                                                                             stdout=out, stderr=subprocess.PIPE, text=True)
    start = lambda dirs: [subprocess.Popen([client, d, str(w), str(h), str(qp), str(frames), "--seed", str(seed), "--digest", os.path.join(d, "digest.txt")],
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for d, (w, h, qp, seed) in zip(dirs, jobs)]
    daemons = [daemon(["--python", "--max-frames", str(frames)], d, paced) for d in solo]
    clients = []
    try:
        clients += start(solo) + start(many)
        # the server starts once all three of its encoders stand in their first handshake: its first round must take the three together
        deadline = time.monotonic() + 60
        while not all(os.path.exists(os.path.join(d, "pred_start.sig")) for d in many):
            assert time.monotonic() < deadline and all(c.poll() is None for c in clients[3:]), "the clients did not reach their first handshake"
            time.sleep(0.001)
        server = daemon(["--sessions"] + many + ["--max-frames", str(3 * frames), "--budget", "0.4", "--budget-mode", "carry"], str(tmp_path), plain, subprocess.PIPE)
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
    steps = [int(ln.split("(")[1].split()[0]) for ln in said.splitlines() if "in this step" in ln]
    assert sum(steps) == 3 * frames and steps[0] == 3, steps
    for k, (w, h, qp, seed) in enumerate(jobs):
        want = open(os.path.join(solo[k], "digest.txt")).read()
        assert len(want.splitlines()) == frames
        assert open(os.path.join(many[k], "digest.txt")).read() == want, "directory %d: per-frame cu_depth.dat digests differ" % k
        md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
        assert md5(os.path.join(many[k], "state.dat")) == md5(os.path.join(solo[k], "state.dat")), "directory %d: state.dat differs" % k
        baked = np.fromfile(os.path.join(many[k], "cu_depth.dat"), "<f4")
        assert set(np.unique(baked).tolist()) <= {0.0, 0.5, 1.0}                 # the files hold baked decisions
        # one line per paced frame, and the summary in serve's wording: the same figures as the solo daemon's
        assert len([ln for ln in said.splitlines() if ln.startswith(many[k] + ": frame ") and " of the full search" in ln]) == frames
        tail = [ln.split("search budget", 1)[1] for ln in solo_err[k].splitlines() if "search budget" in ln]
        mine = [ln.split("search budget", 1)[1] for ln in err.splitlines() if ln.startswith("resi_to_cu_depth_LDP: %s: search budget" % many[k])]
        assert len(tail) == 1 and mine == tail, (k, mine, tail)
