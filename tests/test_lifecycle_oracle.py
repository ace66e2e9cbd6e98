"""CPU: the map-maintenance oracle (tests/lifecycle_oracle.py) on hand-worked cases, the GPU tests' inputs (tests/lifecycle_cases.py) —
that each keeps its distance from the float thresholds and shows the events it is meant to show — and the new C-ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lifecycle_cases as lc
from lifecycle_oracle import FATES, lifecycle_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(stable_confidence_thres=20.0, unstable_time_window=30, add_color_thres=0.1, add_depth_thres=0.1, delete_thresh=10,
          park=torch.tensor([0.0, 0.0, -100.0]))


def _map(n, **cols):
    """n unit Gaussians (radius 0.02), all unstable, confidence 0, add_tick 100, no strikes; cols overwrite whole columns."""
    s = dict(xyz=torch.arange(3.0 * n).reshape(n, 3), opacity_raw=torch.ones(n, 1), scaling_raw=torch.full((n, 3), float(np.log(0.02))),
             confidence=torch.zeros(n), alive=torch.ones(n, dtype=torch.uint8), row_flags=torch.zeros(n, dtype=torch.uint8),
             stable=torch.zeros(n, dtype=torch.uint8), add_tick=torch.full((n,), 100, dtype=torch.int32),
             depth_error_counter=torch.zeros(n, dtype=torch.int32), color_error_counter=torch.zeros(n, dtype=torch.int32))
    for k, v in cols.items():
        s[k] = torch.as_tensor(v, dtype=s[k].dtype).reshape(s[k].shape)
    return s


def _frame(depth_rows, color_rows, depth_err, color_err):
    """A 1 x n frame: pixel j names depth_rows[j] / color_rows[j] and carries the given errors (target depth 2, colour error on red)."""
    n = len(depth_rows)
    gt_depth = torch.full((1, 1, n), 2.0)
    gt_color = torch.full((3, 1, n), 0.5)
    render_color = gt_color.clone()
    render_color[0, 0] += torch.tensor(color_err, dtype=torch.float32)
    return (gt_color, gt_depth, render_color, gt_depth - torch.tensor(depth_err, dtype=torch.float32).reshape(1, 1, n),
            torch.tensor(depth_rows, dtype=torch.int32).reshape(1, 1, n), torch.tensor(color_rows, dtype=torch.int32).reshape(1, 1, n))


NO_FRAME = (None,) * 6


def _fates(r):
    return [FATES[i] for i in r["fate"].tolist()]


def test_promotion_is_strict_and_clips_the_confidence():
    r = lifecycle_oracle(_map(3, confidence=[20.0, 21.0, 500.0]), 100, *NO_FRAME, **KW)
    assert _fates(r) == ["unstable", "stable", "stable"] and r["state"]["stable"].tolist() == [0, 1, 1]
    assert r["state"]["confidence"].tolist() == [20.0, 20.0, 20.0] and r["stats"] == [2, 0, 0, 0, 0, 0, 1, 2]


def test_a_strike_on_an_unstable_row_is_ignored():
    s = _map(2, stable=[0, 1])
    r = lifecycle_oracle(s, 100, *_frame([0, 1], [0, 1], [0.5, 0.5], [0.5, 0.5]), **KW)
    assert r["state"]["depth_error_counter"].tolist() == [0, 1] and r["state"]["color_error_counter"].tolist() == [0, 1]
    assert _fates(r) == ["unstable", "stable"] and r["margin"] > 0.5
    # ... and so is one whose render lies behind the target, one without a depth hit, and any on a pixel without a target depth
    f = list(_frame([1, -1, 1], [0, 0, 1], [-0.5, 0.5, 0.5], [0.0, 0.0, 0.5]))
    f[1][0, 0, 2] = 0.0
    r = lifecycle_oracle(s, 100, *f, **KW)
    assert r["state"]["depth_error_counter"].tolist() == [0, 0] and r["state"]["color_error_counter"].tolist() == [0, 0]


def test_delete_wins_over_release_and_both_need_the_full_count():
    s = _map(4, stable=[1, 1, 1, 1], depth_error_counter=[9, 0, 9, 8], color_error_counter=[9, 9, 0, 8])
    r = lifecycle_oracle(s, 107, *_frame([0, 1, 2, 3], [0, 1, 2, 3], [0.5] * 4, [0.5] * 4), **KW)
    assert _fates(r) == ["deleted_depth", "unstable", "deleted_depth", "stable"] and r["stats"] == [0, 1, 2, 0, 0, 0, 1, 1]
    st = r["state"]
    assert st["alive"].tolist() == [0, 1, 0, 1] and st["row_flags"].tolist() == [3, 0, 3, 0]
    assert torch.equal(st["xyz"][0], KW["park"]) and st["scaling_raw"][2].tolist() == [-10.0] * 3 and float(st["opacity_raw"][0]) == -10.0
    assert st["add_tick"].tolist() == [0, 107, 0, 100] and st["color_error_counter"].tolist() == [0, 10, 0, 9]
    assert st["depth_error_counter"].tolist() == [0, 1, 0, 9] and st["confidence"].tolist() == [0.0] * 4


def test_a_released_row_keeps_its_counters_and_is_released_again():
    s = _map(1, stable=[1], confidence=[20.0], color_error_counter=[9])
    f = _frame([0], [0], [0.0], [0.5])
    r = lifecycle_oracle(s, 101, *f, **KW)
    assert _fates(r) == ["unstable"] and r["state"]["color_error_counter"].tolist() == [10] and r["state"]["add_tick"].tolist() == [101]
    s = r["state"]
    r = lifecycle_oracle(s, 102, *f, **KW)  # unstable: the strike does not count
    assert r["state"]["color_error_counter"].tolist() == [10] and r["stats"][:2] == [0, 0]
    s = r["state"]
    s["confidence"][0] = 25.0
    r = lifecycle_oracle(s, 103, *f, **KW)  # promoted, struck, released in one step
    assert r["stats"][:2] == [1, 1] and r["state"]["color_error_counter"].tolist() == [11] and r["state"]["stable"].tolist() == [0]
    assert r["state"]["add_tick"].tolist() == [103] and r["state"]["confidence"].tolist() == [0.0]


def test_an_empty_unstable_cloud_and_an_empty_map():
    r = lifecycle_oracle(_map(2, stable=[1, 1]), 10 ** 6, *NO_FRAME, **KW)  # (no unstable row: the time rule has nothing to act on)
    assert _fates(r) == ["stable", "stable"] and r["stats"] == [0, 0, 0, 0, 0, 0, 0, 2] and r["margin"] == float("inf")
    r = lifecycle_oracle(_map(2, alive=[0, 0]), 100, *_frame([0], [1], [0.5], [0.5]), **KW)
    assert _fates(r) == ["spare", "spare"] and r["stats"] == [0] * 8


def test_the_time_rule_at_the_window_and_one_past_it():
    r = lifecycle_oracle(_map(3, add_tick=[70, 69, 100]), 100, *NO_FRAME, **KW)
    assert _fates(r) == ["unstable", "deleted_time", "unstable"] and r["stats"] == [0, 0, 0, 0, 1, 0, 2, 0]


def test_oversized_rows_against_their_own_clouds_mean():
    sc = np.log(np.array([0.02] * 40 + [0.6] + [0.02] * 39 + [0.7])).astype(np.float32)[:, None].repeat(3, 1)
    s = _map(81, scaling_raw=sc, stable=[0] * 41 + [1] * 40)
    r = lifecycle_oracle(s, 100, *NO_FRAME, **KW)
    assert [i for i, f in enumerate(_fates(r)) if f.startswith("deleted")] == [40] and _fates(r)[40] == "deleted_oversized_unstable"
    r = lifecycle_oracle(s, 100, *NO_FRAME, stable_oversized=True, **KW)
    assert _fates(r)[40] == "deleted_oversized_unstable" and _fates(r)[80] == "deleted_oversized_stable" and r["stats"][5] == 1
    assert r["margin"] > 0.5


@pytest.mark.parametrize("kw", [dict(seed=11), dict(seed=12, stable_outlier=True), dict(seed=13, n_alive=1, n_spare=0),
                                dict(seed=14, n_alive=0, n_spare=64)])
def test_the_gpu_cases_keep_their_distance_from_the_thresholds(kw):
    case = lc.make_case(**kw)
    r = lifecycle_oracle(case["state"], case["tick"], *[case[k] for k in lc.FRAME], stable_oversized=bool(kw.get("stable_outlier")), **case["kw"])
    assert r["margin"] >= 1e-5
    nm, fates = case["named"], _fates(r)
    if nm:
        of = lambda k: {fates[i] for i in nm[k]}
        assert of("promote") == {"stable"} and of("at_thres") == {"unstable"} and of("window") == {"unstable"}
        assert of("window_plus_1") == {"deleted_time"} and of("oversized") == {"deleted_oversized_unstable"}
        assert of("depth_strike") == of("both_strikes") == {"deleted_depth"} and of("color_strike") == {"unstable"}
        assert of("unstable_struck") == {"unstable"} and of("promoted_and_released") == {"unstable"}
        assert int(r["state"]["color_error_counter"][nm["promoted_and_released"][0]]) == 10
        assert int(r["state"]["color_error_counter"][nm["unstable_struck"][0]]) == 9
        assert all(n > 0 for n in r["stats"][:5]) and (r["stats"][5] == 1) == bool(kw.get("stable_outlier"))
        if "stable_outlier" in nm:
            assert of("stable_outlier") == {"deleted_oversized_stable"}
    elif kw["n_alive"] == 1:
        assert r["stats"][0] == 1
    else:
        assert r["stats"] == [0] * 8


def test_the_sequence_shows_every_event():
    case = lc.sequence_case()
    sc, state, seen = case["scripted"], case["state"], []
    for k in range(lc.SEQUENCE_STEPS):
        r = lifecycle_oracle(state, case["tick"] + k, *[case[m] for m in lc.FRAME], **case["kw"])
        assert r["margin"] >= 1e-5
        state = r["state"]
        seen.append({n: FATES[int(r["fate"][row])] for n, row in sc.items()} | dict(stats=r["stats"]))
        bump = lc.sequence_bump(k, sc)
        if bump:
            state["confidence"][bump[0]] = bump[1]
    assert [s["color_row"] for s in seen[:5]] == ["stable", "stable", "unstable", "unstable", "unstable"]
    assert seen[2]["stats"][1] >= 1 and seen[4]["stats"][0] >= 1 and seen[4]["stats"][1] >= 1  # released, then promoted and released again
    assert int(state["color_error_counter"][sc["color_row"]]) == 4
    assert [s["depth_row"] for s in seen[:3]] == ["stable", "stable", "deleted_depth"]
    assert [s["late_row"] for s in seen[:3]] == ["unstable", "unstable", "stable"]
    assert sum(s["stats"][4] for s in seen) > 0


def test_new_symbols_are_declared_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native as native
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    new = [s for s in re.findall(r"\b(dqo_map_lifecycle_\w+)\(", hdr)]
    assert set(new) >= {"dqo_map_lifecycle_vote", "dqo_map_lifecycle_rows", "dqo_map_lifecycle_workspace_bytes"}
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in new:
        assert hasattr(lib, s) and s in native.EXPORTS, s
    L = native.lib()
    assert L.dqo_abi_version() == 5
    assert "typedef struct DqoLifecycle" in hdr and L.dqo_abi_sizeof(14) == ctypes.sizeof(native.DqoLifecycle) > 0
    assert all(hasattr(lib, s) for s in native.EXPORTS)
