"""CPU: the geometry-evaluation oracle (tests/pcd_oracle.py) against a blocked float32 brute force and against scipy's float64 distances,
the four new C-ABI symbols and the Python surface.

Bars, and why.  nn1_oracle against the brute force: bit for bit — both are the minimum of the same float32 expression, the oracle's over
cKDTree's 8 float64-nearest candidates.  nn1_oracle against cKDTree's float64 distance: 2e-7 relative — the float32 expression rounds
three differences (exact or 2^-24 each), three squares and two sums, about 1e-7 relative on the squared distance, half of that on the
distance; the float32 minimiser may also be another reference than the float64 one, which only brings the two closer.  Metrics from
float32-derived distances against metrics from cKDTree's: counts exactly (premise: no point within 1e-4 relative of a threshold), means
within 3e-7 relative (every term within 2e-7, plus the rounding of two means)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import pcd_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRES = (0.01, 0.03)
NEW_SYMBOLS = ("dqo_nn1_workspace_bytes", "dqo_nn1", "dqo_eval_pcd_workspace_bytes", "dqo_eval_pcd")


@functools.lru_cache(maxsize=1)
def room():
    """gt, rec, and the oracle's two searches (rec -> gt, gt -> rec), computed once."""
    gt, rec = po.room_case()
    return gt, rec, po.nn1_oracle(rec, gt), po.nn1_oracle(gt, rec)


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native as native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqo_raster.h")).read(), flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS, s
    L = native.lib()
    assert L.dqo_abi_version() == 5 and L.dqo_abi_sizeof(13) == 0
    small, big = L.dqo_nn1_workspace_bytes(1, 1), L.dqo_nn1_workspace_bytes(1000000, 1000000)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert L.dqo_nn1_workspace_bytes(-1, 5) == 0 and L.dqo_nn1_workspace_bytes(5, 1 << 25) == 0
    esmall, ebig = L.dqo_eval_pcd_workspace_bytes(1, 1), L.dqo_eval_pcd_workspace_bytes(1000000, 1000000)
    assert small < esmall < ebig and ebig > big and esmall % 256 == 0 and L.dqo_eval_pcd_workspace_bytes(1 << 25, 5) == 0
    # argument validation happens before any launch: usable without a GPU
    assert L.dqo_nn1(-1, 1, None, 5, 1, None, None, None, 1, None, 1, big, None) == -1 and b"size" in L.dqo_last_error()
    assert L.dqo_nn1(5, None, None, 5, 1, None, None, None, 1, None, 1, big, None) == -1 and b"null" in L.dqo_last_error()
    assert L.dqo_nn1(5, 1, None, 5, 1, None, None, None, 1, None, 1, small - 1, None) == -2 and b"workspace" in L.dqo_last_error()
    assert L.dqo_nn1(0, None, None, 5, 1, None, None, None, None, None, None, 0, None) == 0  # (no query: nothing to do)
    th = (ctypes.c_float * 9)(*([0.03] * 9))
    assert L.dqo_eval_pcd(5, 1, None, 5, 1, None, None, 9, th, 1, 0, 1, ebig, None) == -1 and b"thresholds" in L.dqo_last_error()
    assert L.dqo_eval_pcd(5, 1, None, 5, 1, None, None, 1, th, None, 0, 1, ebig, None) == -1 and b"null" in L.dqo_last_error()
    assert L.dqo_eval_pcd(5, 1, None, 5, 1, None, None, 1, th, 1, -1, 1, ebig, None) == -1 and b"row" in L.dqo_last_error()
    assert L.dqo_eval_pcd(5, 1, None, 5, 1, None, None, 1, th, 1, 0, 1, esmall - 1, None) == -2 and b"workspace" in L.dqo_last_error()


def test_nn1_oracle_equals_the_brute_force_and_scipy_on_room():
    gt, rec, (d_rec, i_rec, d64_rec), (d_gt, i_gt, d64_gt) = room()
    assert gt.shape == (5000, 3) and rec.shape == (4000, 3) and gt.dtype == rec.dtype == np.float32
    for name, q, r, d, i, d64 in (("rec->gt", rec, gt, d_rec, i_rec, d64_rec), ("gt->rec", gt, rec, d_gt, i_gt, d64_gt)):
        brute = po.brute_force_f32(q, r)
        assert d.dtype == np.float32 and d.view(np.int32).tobytes() == brute.view(np.int32).tobytes(), name
        assert po.dist2_f32(q, r[i]).view(np.int32).tobytes() == d.view(np.int32).tobytes(), name  # (idx attains dist2)
        rel = np.abs(np.sqrt(d.astype(np.float64)) - d64) / d64
        print(f"{name}: float32 expression against cKDTree's float64 distance: max relative {rel.max():.3e}")
        assert (d64 > 0).all() and rel.max() <= 2e-7, (name, rel.max())


def test_nn1_oracle_masks_and_transforms_restate_the_gathered_search():
    gt, rec, _, _ = room()
    rng = np.random.default_rng(5)
    qk, rk = rng.uniform(size=rec.shape[0]) < 0.5, rng.uniform(size=gt.shape[0]) < 0.5
    m = np.array([[0.8, -0.6, 0.0, 0.25], [0.6, 0.8, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125]], np.float32)
    d, i, _ = po.nn1_oracle(rec, gt, (qk, rk), (m, None))
    assert (d[~qk] == po.FLT_MAX).all() and (i[~qk] == -1).all() and rk[i[qk]].all()
    want = po.brute_force_f32(po.transform_f32(rec, m)[qk], gt[rk])
    assert d[qk].view(np.int32).tobytes() == want.view(np.int32).tobytes()
    none = po.nn1_oracle(rec, gt, (None, np.zeros(gt.shape[0], bool)))
    assert (none[0] == po.FLT_MAX).all() and (none[1] == -1).all()


def test_decisions_and_metrics_on_room():
    gt, rec, (d_rec, _, d64_rec), (d_gt, _, d64_gt) = room()
    s_rec, s_gt = np.sqrt(d_rec.astype(np.float64)), np.sqrt(d_gt.astype(np.float64))
    # premise: no point decides differently in float32 and float64, and none is within 1e-4 relative of a threshold
    for th in THRES:
        for d32, d64 in ((d_rec, d64_rec), (d_gt, d64_gt)):
            kernel = d32.astype(np.float64) < float(np.float32(th)) * float(np.float32(th))  # dqo_eval_pcd's test
            assert np.array_equal(kernel, d64 < th), th
            assert (np.abs(d64 - th) > 1e-4 * th).all(), th
    want, want_counts = po.eval_pcd_oracle(d64_rec, d64_gt, THRES)
    got, got_counts = po.eval_pcd_oracle(s_rec, s_gt, THRES)
    print("room:", {k: float(v) for k, v in want.items()}, want_counts)
    assert got_counts == want_counts
    assert list(want)[:2] == ["accuracy", "completion"] and set(want) == {"accuracy", "completion", "chamfer"} | {
        f"{n} (< {th})" for n in ("P", "R", "F1") for th in THRES}
    for k in want:
        assert abs(got[k] - want[k]) <= 3e-7 * abs(want[k]), (k, got[k], want[k])
    # the anchor recorded with the case: accuracy 8.50 cm, completion 6.32 cm, P / R at 0.03 = 19.2 % / 15.66 %
    assert round(want["accuracy"], 2) == 8.50 and round(want["completion"], 2) == 6.32
    assert want_counts[1] == (768, 783) and round(want["P (< 0.03)"], 2) == 19.2 and round(want["R (< 0.03)"], 2) == 15.66
    # sanity: the floating cluster and the noise show — centimetres of error, a minority of points within 3 cm, more than within 1 cm
    assert 1 < want["accuracy"] < 20 and 1 < want["completion"] < 20
    assert 0 < want["P (< 0.01)"] < want["P (< 0.03)"] < 100 and 0 < want["R (< 0.01)"] < want["R (< 0.03)"] < 100
    assert abs(want["chamfer"] * 100 - (want["accuracy"] + want["completion"])) < 1e-9
    f = want["F1 (< 0.03)"]
    assert min(want["P (< 0.03)"], want["R (< 0.03)"]) <= f <= max(want["P (< 0.03)"], want["R (< 0.03)"])


def test_f1_is_nan_when_nothing_is_under_the_threshold():
    res, counts = po.eval_pcd_oracle(np.array([1.0, 2.0]), np.array([3.0]), (0.5,))
    assert counts == [(0, 0)] and np.isnan(res["F1 (< 0.5)"]) and res["P (< 0.5)"] == 0 and res["accuracy"] == 150.0


def test_python_surface():
    import inspect
    import torch
    import dqo_eval
    assert list(inspect.signature(dqo_eval.eval_pcd).parameters) == ["gt_points", "rec_points", "dist_thres", "transform", "gt_keep", "rec_keep",
                                                                     "out", "row", "workspace_buffer"]
    assert inspect.signature(dqo_eval.eval_pcd).parameters["dist_thres"].default == (0.03,)
    assert list(inspect.signature(dqo_eval.eval_pcd_dict).parameters)[0] == "row_tensor"
    assert len(dqo_eval.PCD_ROW) == 32 and dqo_eval.PCD_ROW[:7] == ("accuracy", "completion", "chamfer", "n_thres", "P0", "R0", "F1_0")
    assert len(set(dqo_eval.PCD_ROW)) == 32 and dqo_eval.ROW[0] == "psnr"
    for word in ("trimesh", "open3d", "sample_surface"):
        assert word in dqo_eval.__doc__, word
    z = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_pcd(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.nearest(z, z)
    row = torch.full((32,), float("nan"))
    row[:10] = torch.tensor([8.5, 6.25, 0.1475, 2.0, 5.0, 4.0, 4.5, 19.0, 15.5, 17.0])
    d = dqo_eval.eval_pcd_dict(row, (0.01, 0.03))
    assert list(d) == ["accuracy", "completion", "P (< 0.01)", "P (< 0.03)", "R (< 0.01)", "R (< 0.03)", "F1 (< 0.01)", "F1 (< 0.03)", "chamfer"]
    assert d["accuracy"] == 8.5 and d["completion"] == 6.25 and d["P (< 0.03)"] == 19.0 and d["R (< 0.01)"] == 4.0 and d["F1 (< 0.03)"] == 17.0
    with pytest.raises(RuntimeError, match="thresholds"):
        dqo_eval.eval_pcd_dict(row, (0.03,))
    from dqo_harness.fused_mapping import FusedMapper
    assert list(inspect.signature(FusedMapper.evaluate_geometry).parameters) == ["self", "gt_points", "dist_thres", "transform", "out", "row"]
