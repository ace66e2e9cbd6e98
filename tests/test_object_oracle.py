"""CPU-side checks of the object stage's oracle (tests/object_oracle.py): it reproduces the reference's detections_filter,
ObjectsInitialization, Occlusions_Check, MatchObject and remove_outlier over the scripted sequences of tests/object_scenes.py — against the
recorded run tests/golden/object_stage_golden.npz, and against a live run where the reference tree is present — the sequences cover every
event the stage has, and every scene keeps its distance from every float threshold, so neither float32 storage nor library rounding can
flip a decision."""
import importlib.util
import os

import numpy as np
import pytest

import object_oracle as O
import object_scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "object_stage_golden.npz")
REFERENCE = os.environ.get("DQO_REFERENCE_ROOT", "/root/reference")
BIG = dict(cap_obj=64, cap_views=64)  # the reference has no capacities


def _generator():
    spec = importlib.util.spec_from_file_location("make_object_stage_golden", os.path.join(HERE, "golden", "make_object_stage_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert np.all((err <= 1e-12) | (got == want)), (what, float(err.max()))


def _hold_to(recorded):
    for name, make in S.ALL.items():
        _, outs, snaps = S.run_oracle(make(), np.float64, **BIG)
        for fi, (o, t) in enumerate(zip(outs, snaps)):
            g = lambda k: recorded[f"{name}/{fi}/{k}"]
            where = f"{name} frame {fi}"
            n = t.n
            assert np.array_equal(o["fate"], g("fate")), (where, o["fate"], g("fate"))
            assert np.array_equal(o["row"], g("row")), (where, o["row"], g("row"))
            assert o["header"]["has_new_object"] == int(g("has_new_object")), where
            assert n == len(g("cat")) and np.array_equal(t.cat[:n], g("cat")) and np.array_equal(t.uid[:n], g("uid")), where
            assert np.array_equal(t.nviews[:n], g("nviews")), (where, t.nviews[:n], g("nviews"))
            _close(o["depth"], g("depth"), where + " depth")
            _close(t.axes[:n], g("axes"), where + " axes")
            _close(t.R[:n], g("R"), where + " R")
            _close(t.center[:n], g("center"), where + " center")
            views = [(i, k) for i in range(n) for k in range(t.nviews[i])]
            _close(np.array([t.view_bbox[i, k] for i, k in views]).reshape(-1, 4), g("view_bbox"), where + " view_bbox")
            _close(np.array([t.view_P34[i, k] for i, k in views]).reshape(-1, 12), g("view_P34"), where + " view_P34")


def test_float64_oracle_is_the_recorded_reference():
    _hold_to(np.load(GOLDEN))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "SLAM", "multiprocess")), reason="the reference tree is not on this machine")
def test_float64_oracle_is_the_live_reference_and_the_golden_is_current():
    live = _generator().record(REFERENCE)
    _hold_to(live)
    rec = np.load(GOLDEN)
    assert sorted(rec.files) == sorted(live)
    for k in rec.files:
        assert np.array_equal(rec[k], live[k]), k


@pytest.mark.parametrize("store", [np.float64, np.float32])
def test_margins_and_events(store):
    seen = set()
    for name, make in S.ALL.items():
        seq = make()
        t, outs, _ = S.run_oracle(seq, store)
        if name in S.SEQUENCES:
            assert 6 <= len(seq["frames"]) <= 8 and all(len(f["dets"]["cat"]) <= 8 for f in seq["frames"]) and t.n <= 12
        else:  # the wide sequence: accepted detections beyond index 32
            assert all(o["header"]["accepted"] > 32 and (o["fate"][32:] != O.FATE_DROPPED).all() for o in outs)
        margin = min(m for o in outs for m in o["margins"])
        assert margin >= 1e-4, (name, margin)
        if name in S.SEQUENCES:
            for o in outs:
                seen |= o["events"]
    assert not set(S.EVENTS) - seen, set(S.EVENTS) - seen
    assert not seen - set(S.EVENTS) - {"too_deep"}, seen - set(S.EVENTS)  # (EVENTS names every event the oracle can emit but the unreachable one)
    # the overflow sequence overflows both capacities; no other one does
    for name, make in S.SEQUENCES.items():
        _, outs, _ = S.run_oracle(make(), store)
        over = (sum(o["header"]["overflow_obj"] for o in outs), sum(o["header"]["overflow_views"] for o in outs))
        assert (over[0] > 0 and over[1] > 0) if name == "overflow" else over == (0, 0), (name, over)


def test_float32_storage_flips_no_decision():
    for name, make in S.ALL.items():
        _, a, sa = S.run_oracle(make(), np.float64)
        _, b, sb = S.run_oracle(make(), np.float32)
        for fi, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x["fate"], y["fate"]) and np.array_equal(x["row"], y["row"]) and x["header"] == y["header"], (name, fi)
            assert np.array_equal(x["opt_flag"], y["opt_flag"]) and np.array_equal(sa[fi].nviews, sb[fi].nviews), (name, fi)
            assert sb[fi].axes.dtype == np.float32 and np.allclose(sa[fi].axes, sb[fi].axes, rtol=1e-6, atol=0)


def test_remove_outlier_is_any_earlier_row_of_the_category():
    """The literal double loop of quadrics.py:2403-2418 pops exactly the rows j for which some row i < j of j's category is far."""
    rng = np.random.default_rng(5)
    P = (S.K.astype(np.float64) @ np.eye(4)[:3])
    removed = 0
    for trial in range(40):
        n = int(rng.integers(2, 12))
        cats = rng.integers(0, 3, n)
        pr = []
        for i in range(n):
            c = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(1.5, 3.0)])
            pr.append(O.project(rng.uniform(0.05, 0.3, 3), np.eye(3).reshape(9), c, P))
        keep = O.remove_outlier_literal(cats, pr)
        rule = [j for j in range(n) if not any(cats[i] == cats[j] and O.calculate_distance(pr[i], pr[j]) < 0.1 for i in range(j))]
        assert keep == rule, (trial, keep, rule)
        removed += n - len(rule)
    assert removed > 20  # (the trials do remove rows, and not only last ones)


def test_key_rule_is_the_header_rule(tmp_path):
    """dqo_object_key of csrc/dqo_sample_hash.h, compiled for the host, gives the oracle's keys; the pixel rule on top of it treats an
    empty range as one value, as the header says."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler is needed"
    cases = [(0x123456789ABCDEF, 8, 77, 5 * 32 + 9), (0, 9, 0, 0), (7, 10, 53, 12 * 32 + 19), (2 ** 64 - 1, 8, 2 ** 31 - 1, 63 * 32 + 29)]
    src = tmp_path / "key.cpp"
    src.write_text('#include <stdio.h>\n#include "dqo_sample_hash.h"\nint main() {\n' + "".join(
        f'    printf("%u\\n", dqo_object_key(dqo_sample_seed_word({s}ull), {d}u, {f}u, {i}u));\n' for s, d, f, i in cases) + "    return 0;\n}\n")
    exe = tmp_path / "key"
    subprocess.check_call([cxx, "-O1", "-I", os.path.join(os.path.dirname(HERE), "dqo-map_amd", "csrc"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [O.object_key(*c) for c in cases]
    u, v = O.sample_uv(3, 4, 2, 0, [-3.5, 100.2, 12.9, 130.0], S.W, S.H)
    assert 0 <= u <= 12 and 100 <= v <= S.H - 1
    assert O.sample_uv(3, 4, 2, 0, [50.0, 60.0, 40.0, 30.0], S.W, S.H) == (50, 60)  # empty ranges: one value each
    sched = O.optimize_schedule(1, 2, 3, 4)
    assert len(sched) == 20 and all(0 <= x < 4 for x in sched[:6]) and sched[6:] == [3] * 14
