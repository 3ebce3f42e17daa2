"""CPU: what a pacer set with a policy per slot (include/ethcnn.h "search budget, online: several sequences, a POLICY per slot") settles
without a GPU: the layout of a call whose frames stand under ladders of different lengths, against a Python restatement; the rules of a
policy list, reported per policy index; the policy file of `resi_to_cu_depth_LDP.py --sessions ... --budget-policies`, its start-up
refusals and the order in which a directory finds its policy; and the server process on a bad file: status 1, nothing written.  The
kernels are in tests/test_gpu_pacer_policies.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER = os.path.join(ROOT, "resi_to_cu_depth_LDP.py")
COMPANION_LDP = "0.25 0.75 0.25 0.75 0.25 0.75"
ERR_ARG = -1
RUNGS = (2, 256, 257, 513, 4097)   # K + 1: one rung block, exactly one, one more, the default ladder, the longest
CTUS = (1, 4, 65, 272)             # one slice of one CTU, of four, two slices, five


# ------------------------------------------------------------------------------------------------------------------------- plan ---
def _plan_ref(nctus, rungs):
    """the definition: slices of at most 64 CTUs, balanced; a frame's count blocks = slices x ceil(ITS rungs / 256), its bake blocks =
    ceil(n / 256); everything a running sum in call order"""
    out = {k: [] for k in ("count_first", "count_blocks", "slice_len", "bake_first", "rec0")}
    count = bake = rec = 0
    for n, r in zip(nctus, rungs):
        most = (n + 63) // 64
        length = (n + most - 1) // most
        slices = (n + length - 1) // length
        blocks = slices * ((r + 255) // 256)
        out["count_first"].append(count), out["count_blocks"].append(blocks), out["slice_len"].append(length)
        out["bake_first"].append(bake), out["rec0"].append(rec)
        count, bake, rec = count + blocks, bake + (n + 255) // 256, rec + n
    out.update(count_grid=count, bake_grid=bake)
    return out


def test_plan_rungs_against_its_restatement(pkg):
    plan = pkg.ethcnn.pacer_set_plan
    rng = np.random.default_rng(17)
    calls = [([n] * len(RUNGS), list(RUNGS)) for n in CTUS]                          # one size under every ladder
    calls += [(list(CTUS), [r] * len(CTUS)) for r in RUNGS]                          # every size under one ladder
    calls += [(list(CTUS) + [272], [4097, 2, 257, 256, 513]), ([272, 1], [2, 4097]), ([1, 272], [4097, 2])]
    calls += [([int(x) for x in rng.choice(CTUS, size=32)], [int(x) for x in rng.choice(RUNGS, size=32)]) for _ in range(4)]
    for nctus, rungs in calls:
        got = plan(nctus, [r - 1 for r in rungs])
        assert got == _plan_ref(nctus, rungs), (nctus, rungs)
        ends = [a + b for a, b in zip(got["count_first"], got["count_blocks"])]
        assert got["count_first"] == [0] + ends[:-1] and ends[-1] == got["count_grid"]   # disjoint, contiguous, in call order
    assert plan([1, 12], [1, 4096])["count_blocks"] == [1, 17]                       # one launch mixes 1 and 17 rung blocks
    assert plan([272, 272], [512, 256])["count_blocks"] == [15, 10]
    # with equal K: ethcnn_pacer_set_plan itself
    for r in RUNGS:
        for nctus in ([1], list(CTUS), [272] * 32, [(1 << 24) - 1] * 32):
            assert plan(nctus, [r - 1] * len(nctus)) == plan(nctus, r - 1), (r, nctus[:4])


def test_plan_rungs_refuses_per_frame_what_the_plan_refuses(pkg):
    lib = pkg.load_library()
    plan = pkg.ethcnn.pacer_set_plan
    for nctus, K in (([1] * 33, [512] * 33), ([12, 1 << 24], [512, 512]), ([12, 0], [512, 512]), ([-3], [512]), ([], []),
                     ([12, 12], [512, 0]), ([12, 12], [4097, 512]), ([12, 12, 12], [1, 4096, -1])):
        with pytest.raises(pkg.EthCnnError) as err:
            plan(nctus, K)
        assert err.value.code == ERR_ARG, (nctus[:3], K[:3])
    with pytest.raises(ValueError):
        plan([12, 12], [512])                                                        # (the binding: a K per frame)
    grid = np.full(2, 7, np.int64)
    one, k = np.array([12], np.int64), np.array([4097], np.int64)
    tail = (None, None, None, None, None, grid.ctypes.data, grid.ctypes.data + 8)
    assert lib.ethcnn_pacer_policies_plan(one.ctypes.data, k.ctypes.data, 1, *tail) == ERR_ARG
    assert lib.ethcnn_pacer_policies_plan(one.ctypes.data, None, 1, *tail) == ERR_ARG
    assert lib.ethcnn_pacer_policies_plan(None, k.ctypes.data, 1, *tail) == ERR_ARG
    assert grid.tolist() == [7, 7]                                                   # a refusal writes nothing
    k[0] = 4096
    assert lib.ethcnn_pacer_policies_plan(one.ctypes.data, k.ctypes.data, 1, *tail) == 0 and grid.tolist() == [17, 1]


# --------------------------------------------------------------------------------------------------------------- check_policies ---
def _ladder(pkg, n):
    lad = np.zeros(n, pkg.ethcnn.SIM_THR)
    lad["up_k"], lad["down_k"] = 1024, 0
    return lad


def _refusal(pkg, policies, slot_policy=None):
    with pytest.raises(pkg.EthCnnError) as err:
        pkg.ethcnn.pacer_set_check_policies(policies, slot_policy, raw=True)
    assert err.value.code == ERR_ARG
    return str(err.value)


def test_check_policies_reports_every_rule_per_policy_index(pkg):
    e = pkg.ethcnn
    good = {"budget": 400000, "mode": e.BUDGET_CARRY}
    e.pacer_set_check_policies([good], raw=True)
    e.pacer_set_check_policies([good, dict(good, ladder=_ladder(pkg, 4096), weights=(2 ** 32 - 1,) * 4, budget=1000000, mode=e.BUDGET_FRAME)] * 16, list(range(32)), raw=True)
    e.pacer_set_check_policies([{"budget": 0.4, "mode": "carry"}, {"budget": 1.0}], [1, 0, 1])   # (shares and mode names: the PacerSet form)
    up, down, both = _ladder(pkg, 3), _ladder(pkg, 3), _ladder(pkg, 3)
    up["up_k"][2, 1], down["down_k"][1, 0], both["up_k"][0, 0] = 1025, -2, -1
    rules = {"too many rungs": dict(good, ladder=_ladder(pkg, 4097)), "no rung": dict(good, ladder=_ladder(pkg, 0)),
             "an up threshold above 1": dict(good, ladder=up), "a down threshold below -1/1024": dict(good, ladder=down),
             "an up threshold below 0": dict(good, ladder=both), "a weight of 2^32": dict(good, weights=(64, 16, 2 ** 32, 1)),
             "a budget above 10^6": dict(good, budget=1000001), "mode 2": dict(good, mode=2), "mode -1": dict(good, mode=-1)}
    for what, bad in rules.items():
        # what ethcnn_pacer_check says about that policy alone ...
        with pytest.raises(e.EthCnnError) as solo:
            e.pacer_check(bad["budget"], bad["mode"], bad.get("ladder"), bad.get("weights"))
        why = str(solo.value).split(": ", 1)[1]
        # ... is what the set says about it, behind its index, wherever it stands among good ones; the first broken policy is named
        for at, n in ((0, 1), (2, 3), (31, 32), (1, 4)):
            text = _refusal(pkg, [bad if i == at else good for i in range(n)])
            assert "policy %d: %s" % (at, why) in text, (what, at, text)
        text = _refusal(pkg, [good, bad, good, rules["mode 2"]])
        assert "policy 1: " in text and "policy 3" not in text, (what, text)
    assert "0 policies" in _refusal(pkg, []) and "33 policies" in _refusal(pkg, [good] * 33)
    assert "slot 2: policy 3 is outside 0..2" in _refusal(pkg, [good] * 3, [0, 2, 3, 1])
    assert "slot 0: policy -1" in _refusal(pkg, [good] * 3, [-1, 0])
    assert "33 slots" in _refusal(pkg, [good], [0] * 33)
    lib = pkg.load_library()
    assert lib.ethcnn_pacer_policies_check(None, 1, None, 0) == ERR_ARG
    # NULL handles never reach a GPU
    assert lib.ethcnn_pacer_policies_create(None, 4, None, 1, None, None) == ERR_ARG
    assert lib.ethcnn_pacer_policies_bind(None, 0, 0) == ERR_ARG and lib.ethcnn_pacer_policies_count(None) < 0 and lib.ethcnn_pacer_policies_of(None, 0) < 0
    assert e.PACER_SET_MAX_POLICIES == 32 and "#define ETHCNN_PACER_SET_MAX_POLICIES 32" in open(os.path.join(ROOT, "include", "ethcnn.h")).read()
    import ctypes
    assert ctypes.sizeof(e.PacerPolicy) == 32 and e.PacerPolicy.budget_ppm.offset == 24 and e.PacerPolicy.mode.offset == 28
    for method in ("bind", "policy_of"):
        assert callable(getattr(pkg.PacerSet, method))
    assert isinstance(pkg.PacerSet.npolicies, property)


# ------------------------------------------------------------------------------------------------------- the policy file ---
def _dirs(tmp_path, n, thr=None):
    out = []
    for k in range(n):
        d = tmp_path / ("hm%02d" % k)
        d.mkdir()
        (d / "Thr_info.txt").write_text((thr or {}).get(k, COMPANION_LDP) + "\n")
        out.append(str(d))
    return out


def _tree(tmp_path):
    return sorted((os.path.relpath(os.path.join(dp, f), str(tmp_path)), os.path.getsize(os.path.join(dp, f)))
                  for dp, _, fs in os.walk(str(tmp_path)) for f in fs + ["."])


def _server(tmp_path, args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ETHCNN_")}
    e.update(ETHCNN_SYNTHETIC_SEED="21")
    return subprocess.run([sys.executable, LAUNCHER] + args + ["--max-frames", "0", "--idle-timeout", "0"], capture_output=True, text=True, env=e,
                          cwd=str(tmp_path), timeout=120)


def _write(tmp_path, text, name="policies.txt"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_the_parser_reads_every_field_and_the_resolver_keeps_the_order(pkg, tmp_path):
    sb = pkg.search_budget
    dirs = _dirs(tmp_path, 4)
    ladder = _write(tmp_path, "0.0 1.0 0.0 1.0 0.0 1.0\n0.25 0.75 0.25 0.75 0.25 0.75\n0.5 0.5 0.5 0.5 0.5 0.5\n", "ladder.txt")
    link = tmp_path / "link"
    link.symlink_to(dirs[2])
    path = _write(tmp_path, "# four ways to a policy\n\nqp=30..34 0.6 carry   # a range\n*  0.2\ndir=%s 0.8 frame %s 8 4 2 1\nqp=22..32 0.4 carry -\n"
                  "dir=%s/ 1 carry - 1 1 1 1\n*  0.9 carry\n" % (link, ladder, dirs[0]))
    lines = sb.read_policies(path, "ldp")
    assert [s for s, _ in lines] == [("qp", 30, 34), ("*",), ("dir", os.path.realpath(dirs[2])), ("qp", 22, 32), ("dir", os.path.realpath(dirs[0])), ("*",)]
    assert [p[:3] for _, p in lines] == [(0.6, "carry", None), (0.2, "frame", None), (0.8, "frame", [8, 4, 2, 1]), (0.4, "carry", None),
                                         (1.0, "carry", [1, 1, 1, 1]), (0.9, "carry", None)]
    assert [p[3] for _, p in lines] == [None, None, sb.read_ladder(ladder, "ldp"), None, None, None]
    assert lines[2][1][3] == ([[1024] * 3, [768] * 3, [512] * 3], [[0] * 3, [256] * 3, [512] * 3])   # (up, down) from Low-Delay-P token order: down up ...
    default = (0.5, "frame", None, None)
    pol = sb.Policies(lines, dirs, default)
    assert pol.policies == [p for _, p in lines] + [default]
    # dir over qp over * over --budget; inside a kind the first line wins; the directory is found by its realpath
    assert pol.of(dirs[2], 32) == 2 and pol.of(str(link), 99) == 2 and pol.of(dirs[0], 32) == 4
    assert pol.of(dirs[1], 32) == 0 and pol.of(dirs[1], 30) == 0 and pol.of(dirs[1], 34) == 0 and pol.of(dirs[1], 29) == 3 and pol.of(dirs[1], 22) == 3
    assert pol.of(dirs[1], 21) == 1 and pol.of(dirs[3], 35) == 1                     # the first *, never the second, never --budget
    no_star = [ln for ln in lines if ln[0] != ("*",)]
    pol = sb.Policies(no_star, dirs, default)
    assert pol.of(dirs[1], 21) == 4 == len(pol.policies) - 1 and pol.of(dirs[1], 31) == 0 and pol.of(dirs[2], 21) == 1
    only_dirs = [ln for ln in lines if ln[0][0] == "dir"]
    assert sb.Policies(only_dirs, [dirs[0], dirs[2]]).of(dirs[2], 5) == 0            # every directory has a dir= line: no default needed


def test_every_start_up_refusal_of_the_policy_file(pkg, tmp_path):
    ldp = pkg.resi_to_cu_depth_LDP if hasattr(pkg, "resi_to_cu_depth_LDP") else __import__("importlib").import_module(pkg.__name__ + ".resi_to_cu_depth_LDP")
    dirs = _dirs(tmp_path, 3)
    other = tmp_path / "elsewhere"
    other.mkdir()
    five = _write(tmp_path, "0.1 0.9 0.1 0.9 0.1\n", "five.txt")
    default = (0.4, "frame", None, None)
    cases = (("* 1.5\n", "SHARE='1.5' is not a share"), ("* nan\n", "share"), ("* lots\n", "share"), ("* 0.4 both\n", "MODE='both' (allowed: frame, carry)"),
             ("* 0.4 carry - 64 16 4\n", "got 7 fields"), ("* 0.4 carry - 64 16 4 x\n", "four integers"), ("* 0.4 carry - 64 16 4 4294967296\n", "four integers"),
             ("* 0.4 carry - 64 16 4 -1\n", "four integers"), ("* 0.4 carry %s\n" % (tmp_path / "none.txt"), "cannot be read"),
             ("* 0.4 carry %s\n" % five, "a rung is six values"), ("* 0.4 carry auto\n", "one frame at a time"), ("*\n", "got 1 fields"),
             ("* 0.4 carry - 1 2 3 4 5\n", "got 9 fields"), ("all 0.4\n", "selector 'all'"), ("dir= 0.4\n", "selector"), ("qp=30 0.4\n", "not qp=LO..HI"),
             ("qp=a..b 0.4\n", "not qp=LO..HI"), ("qp=33..32 0.4\n* 0.4\n", "LO > HI"), ("dir=%s 0.4\n* 0.5\n" % other, "names none of the --sessions directories"),
             ("dir=%s 0.4\n* 0.5\ndir=%s/. 0.6\n" % (dirs[1], dirs[1]), "two dir= lines"), ("* 0.4\n" * 32, "33 policies"))
    for n, (text, why) in enumerate(cases):
        path = _write(tmp_path, text, "bad%02d.txt" % n)
        with pytest.raises(ValueError) as err:
            ldp.check_policies(dirs, path, default)
        assert why in str(err.value) and "--budget-policies" in str(err.value), (text, str(err.value))
        if "\n" in text.rstrip("\n") and "33" not in why:
            assert "line 1" in str(err.value) or "dir=" in str(err.value)
    ldp.check_policies(dirs, _write(tmp_path, "* 0.4\n" * 31, "full.txt"), default)   # 32 with the default
    ldp.check_policies(dirs, _write(tmp_path, "* 0.4\n" * 32, "full32.txt"))          # 32 without one
    with pytest.raises(ValueError) as err:
        ldp.check_policies(dirs, str(tmp_path / "missing.txt"), default)
    assert "cannot be read" in str(err.value)
    # no default while a directory has no dir= line; with a default, or a line for every directory, the same file is taken
    partial = _write(tmp_path, "dir=%s 0.4\nqp=0..51 0.5\ndir=%s 0.6\n" % (dirs[0], dirs[2]), "partial.txt")
    with pytest.raises(ValueError) as err:
        ldp.check_policies(dirs, partial)
    assert dirs[1] in str(err.value) and "no default" in str(err.value)
    assert len(ldp.check_policies(dirs, partial, default).policies) == 4
    assert len(ldp.check_policies([dirs[0], dirs[2]], _write(tmp_path, "dir=%s 0.4\ndir=%s 0.6\n" % (dirs[0], dirs[2]), "each.txt")).policies) == 2
    with pytest.raises(ValueError) as err:
        ldp.check_policies(dirs, _write(tmp_path, "# nothing\n\n", "empty.txt"))
    assert "no policy" in str(err.value)
    # a directory whose Thr_info.txt is not the companion line
    sub = tmp_path / "thr"
    sub.mkdir()
    odd = _dirs(sub, 3, thr={1: "0.3 0.75 0.25 0.75 0.25 0.75"})
    with pytest.raises(ValueError) as err:
        ldp.check_policies(odd, _write(tmp_path, "* 0.4\n", "star.txt"))
    assert "companion" in str(err.value) and os.path.join(odd[1], "Thr_info.txt") in str(err.value)


def test_the_server_process_refuses_a_bad_file_with_status_1_and_writes_nothing(tmp_path):
    dirs = _dirs(tmp_path, 2)
    good = _write(tmp_path, "qp=22..27 0.2 carry\n* 0.6\n", "good.txt")
    bad = {"share": _write(tmp_path, "qp=22..27 0.2 carry\n* 1.6\n", "share.txt"), "auto": _write(tmp_path, "* 0.4 carry auto\n", "auto.txt"),
           "range": _write(tmp_path, "qp=37..22 0.4\n* 0.4\n", "range.txt"), "default": _write(tmp_path, "dir=%s 0.4\n" % dirs[0], "default.txt"),
           "missing": str(tmp_path / "missing.txt")}
    texts = {"share": "line 2: SHARE='1.6' is not a share", "auto": "one frame at a time", "range": "LO > HI", "default": "no default", "missing": "cannot be read"}
    base = ["--sessions"] + dirs
    before = _tree(tmp_path)
    for what, path in bad.items():
        for opts in ([], ["--budget", "0.4", "--budget-mode", "carry"]):
            if what == "default" and opts:
                continue                                                             # (--budget is the default then)
            r = _server(tmp_path, base + opts + ["--budget-policies", path])
            assert r.returncode == 1, (what, r.returncode, r.stderr[-800:])
            assert "resi_to_cu_depth_LDP: --budget-policies" in r.stderr and texts[what] in r.stderr and "Traceback" not in r.stderr, (what, r.stderr[-800:])
            assert _tree(tmp_path) == before, what
    # the value rules of --budget stay in front; the option belongs to --sessions and stands once
    r = _server(tmp_path, base + ["--budget", "1.5", "--budget-policies", good])
    assert r.returncode == 1 and "--budget='1.5' is not a share" in r.stderr and _tree(tmp_path) == before
    for args in (["--budget-policies", good], base + ["--budget-policies", good, "--budget-policies", good], base + ["--budget-policies"]):
        r = _server(tmp_path, args)
        assert r.returncode == 2 and "usage:" in r.stderr and _tree(tmp_path) == before, args
    # a good file gets past the checks: whatever happens next is none of the refusals (without a GPU the context fails, with another message)
    r = _server(tmp_path, base + ["--quiet", "--budget-policies", good])
    assert "--budget-policies" not in r.stderr and "usage" not in r.stderr and r.returncode != 2, r.stderr[-600:]
    assert not [f for d in dirs for f in os.listdir(d) if f != "Thr_info.txt"]
