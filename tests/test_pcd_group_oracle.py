"""CPU: the per-object geometry-evaluation oracle (tests/pcd_group_oracle.py) against a blocked float32 brute force per group, the
premises of the GPU bars on the cases test_gpu_eval_pcd_objects.py uses, the five new C-ABI symbols and the Python surface.

Bars, and why.  nn1_grouped_oracle against the brute force over each group's gathered subsets: bit for bit — both are the minimum of
the same float32 expression.  The premises are the ones tests/test_pcd_oracle.py states for "counts exactly": no distance within 1e-4
relative of a threshold, and the float32 and float64 decisions agree; on top of them a grouped case must be able to tell a grouped
search from an ungrouped one (queries whose nearest neighbour regardless of group is foreign) and a count from a constant (a threshold
whose count lies strictly between 0 and the row count, per object and direction)."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

import pcd_group_oracle as go
import pcd_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dqo_nn1_grouped_workspace_bytes", "dqo_nn1_grouped", "dqo_eval_pcd_grouped_workspace_bytes", "dqo_eval_pcd_grouped",
               "dqo_map_pack_rows_by_object")


@functools.lru_cache(maxsize=1)
def objects():
    """The case "objects" and the oracle's two grouped searches (rec -> gt, gt -> rec), computed once."""
    gt, gt_object, rec, rec_object = go.objects_case()
    return (gt, gt_object, rec, rec_object, go.nn1_grouped_oracle(rec, rec_object, gt, gt_object),
            go.nn1_grouped_oracle(gt, gt_object, rec, rec_object))


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
    for s in NEW_SYMBOLS:
        assert getattr(L, s).argtypes, s
    small, big = L.dqo_nn1_grouped_workspace_bytes(1, 1), L.dqo_nn1_grouped_workspace_bytes(1000000, 1000000)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert L.dqo_nn1_grouped_workspace_bytes(-1, 5) == 0 and L.dqo_nn1_grouped_workspace_bytes(5, 1 << 25) == 0
    esmall, ebig = L.dqo_eval_pcd_grouped_workspace_bytes(1, 1), L.dqo_eval_pcd_grouped_workspace_bytes(1000000, 1000000)
    assert small < esmall < ebig and ebig > big and esmall % 256 == 0
    assert L.dqo_eval_pcd_grouped_workspace_bytes(1 << 25, 5) == 0 and L.dqo_eval_pcd_grouped_workspace_bytes(5, -1) == 0


def test_arguments_are_checked_before_any_launch():
    """Usable without a GPU: every call below fails (or has nothing to do) before anything is dereferenced or launched."""
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native as native
    L = native.lib()
    need = L.dqo_nn1_grouped_workspace_bytes(5, 5)
    nn1 = lambda Q, q, qg, R, r, rg, d, ws_bytes: L.dqo_nn1_grouped(Q, q, qg, R, r, rg, None, None, d, None, 1, ws_bytes, None)
    assert nn1(-1, 1, 1, 5, 1, 1, 1, need) == -1 and b"size" in L.dqo_last_error()
    assert nn1(5, 1, 1, 1 << 25, 1, 1, 1, need) == -1 and b"size" in L.dqo_last_error()
    assert nn1(5, None, 1, 5, 1, 1, 1, need) == -1 and b"null" in L.dqo_last_error()
    assert nn1(5, 1, 1, 5, 1, 1, None, need) == -1 and b"null" in L.dqo_last_error()
    assert nn1(5, 1, None, 5, 1, 1, 1, need) == -1 and b"group" in L.dqo_last_error()
    assert nn1(5, 1, 1, 5, 1, None, 1, need) == -1 and b"group" in L.dqo_last_error()
    assert nn1(5, 1, 1, 5, 1, 1, 1, need - 1) == -2 and b"workspace" in L.dqo_last_error()
    assert L.dqo_nn1_grouped(5, 1, 1, 5, 1, 1, None, None, 1, None, None, need, None) == -2
    assert nn1(0, None, None, 5, 1, 1, None, 0) == 0  # (no query: nothing to do)
    eneed = L.dqo_eval_pcd_grouped_workspace_bytes(5, 5)
    th = (ctypes.c_float * 9)(*([0.01] * 9))

    def ev(n_gt=5, gt=1, gg=1, n_rec=5, rec=1, rg=1, n_thres=1, thres=th, out=1, rows=64, first=0, ws=1, ws_bytes=eneed):
        return L.dqo_eval_pcd_grouped(n_gt, gt, gg, n_rec, rec, rg, None, n_thres, thres, out, rows, first, ws, ws_bytes, None)

    assert ev(n_gt=-1) == -1 and b"size" in L.dqo_last_error()
    assert ev(n_rec=1 << 25) == -1 and b"size" in L.dqo_last_error()
    assert ev(gt=None) == -1 and b"null" in L.dqo_last_error()
    assert ev(out=None) == -1 and b"null" in L.dqo_last_error()
    assert ev(gg=None) == -1 and b"group" in L.dqo_last_error()
    assert ev(rg=None) == -1 and b"group" in L.dqo_last_error()
    assert ev(n_thres=9) == -1 and b"thresholds" in L.dqo_last_error()
    assert ev(n_thres=1, thres=None) == -1 and b"thresholds" in L.dqo_last_error()
    assert ev(first=-1) == -1 and b"rows" in L.dqo_last_error()
    assert ev(rows=66, first=3) == -1 and b"rows" in L.dqo_last_error()  # (first_row + 64 > table_rows)
    assert ev(rows=63) == -1 and b"rows" in L.dqo_last_error()
    assert ev(ws_bytes=eneed - 1) == -2 and b"workspace" in L.dqo_last_error()
    assert ev(ws=None) == -2 and b"workspace" in L.dqo_last_error()
    pneed = L.dqo_map_pack_workspace_bytes(4)

    def pk(P=4, M=1, xyz=1, obj=1, table=1, rows=4, header=1, ws=1, ws_bytes=pneed):
        return L.dqo_map_pack_rows_by_object(P, M, 0, xyz, 1, 1, 1, 1, None, None, None, obj, table, rows, header, ws, ws_bytes, None)

    assert pk(P=0) == -1 and pk(M=65) == -1 and pk(xyz=None) == -1 and pk(header=None) == -1
    assert pk(obj=None) == -1 and b"object" in L.dqo_last_error()
    assert pk(rows=3) == -1 and b"capacity" in L.dqo_last_error()
    assert pk(ws_bytes=pneed - 1) == -2 and L.dqo_last_error().decode() == f"map pack workspace too small ({pneed - 1} < {pneed})"


def test_grouped_oracle_equals_the_brute_force_per_group_on_objects():
    gt, gt_object, rec, rec_object, (d_rec, i_rec, _), (d_gt, i_gt, _) = objects()
    assert gt.shape == rec.shape == (9000, 3) and gt.dtype == rec.dtype == np.float32 and gt_object.dtype == rec_object.dtype == np.int32
    assert go.groups_of(gt_object) == [0, 5, 7, 63] and go.groups_of(rec_object) == [0, 5, 63] and (rec_object == -1).sum() == 2000
    for name, q, qg, r, rg, d, i in (("rec->gt", rec, rec_object, gt, gt_object, d_rec, i_rec), ("gt->rec", gt, gt_object, rec, rec_object, d_gt, i_gt)):
        for g in go.groups_of(qg, rg):
            want = po.brute_force_f32(q[qg == g], r[rg == g])
            assert d[qg == g].view(np.int32).tobytes() == want.view(np.int32).tobytes(), (name, g)
            assert (rg[i[qg == g]] == g).all(), (name, g)  # (only references of the query's group are found)
        found = np.isin(qg, go.groups_of(qg, rg))
        assert (d[~found] == po.FLT_MAX).all() and (i[~found] == -1).all() and (i[found] >= 0).all(), name
        assert po.dist2_f32(q[found], r[i[found]]).view(np.int32).tobytes() == d[found].view(np.int32).tobytes(), name
    assert (d_gt[gt_object == 7] == po.FLT_MAX).all()  # (the object the map never saw)


def test_premises_of_the_gpu_bars_on_objects():
    gt, gt_object, rec, rec_object, (d_rec, _, d64_rec), (d_gt, _, d64_gt) = objects()
    p = go.objects_premises(gt, gt_object, rec, rec_object, go.OBJECTS_THRES)
    print("objects:", p)
    assert p["margin"] > 1e-4 and p["decisive"]
    assert sorted(p["foreign"]) == [0, 5, 63] and all(a > 0 and b > 0 for a, b in p["foreign"].values())
    # the float32 decisions of the kernel are the float64 decisions of the oracle, and the two distances agree to 2e-7
    for th in go.OBJECTS_THRES:
        for d32, d64, ids in ((d_rec, d64_rec, rec_object), (d_gt, d64_gt, gt_object)):
            rows = np.isin(ids, [0, 5, 63])
            kernel = d32[rows].astype(np.float64) < float(np.float32(th)) * float(np.float32(th))
            assert np.array_equal(kernel, d64[rows] < th), th
            rel = np.abs(np.sqrt(d32[rows].astype(np.float64)) - d64[rows]) / d64[rows]
            assert rel.max() <= 2e-7
    res = go.eval_pcd_objects_oracle(gt, gt_object, rec, rec_object, go.OBJECTS_THRES)
    assert sorted(res) == [0, 5, 63]
    for g, (results, counts, n_rec, n_gt, _, _) in res.items():
        print(g, {k: float(v) for k, v in results.items()}, counts, n_rec, n_gt)
        assert n_gt == 2250 and n_rec in (2333, 2334) and 0.1 < results["accuracy"] < 2 and 0.1 < results["completion"] < 2


def test_premises_of_the_gpu_bars_on_two_groups_and_on_the_stored_frame():
    p = go.objects_premises(*go.two_groups_case(), go.TWO_GROUPS_THRES)
    print("two groups:", p)
    assert p["margin"] > 1e-4 and p["decisive"] and all(a > 0 and b > 0 for a, b in p["foreign"].values())
    p = go.objects_premises(*go.objects_stored_case(), go.OBJECTS_THRES, go.OBJECTS_XFORM)
    print("objects, stored in another frame:", p)
    assert p["margin"] > 1e-4 and p["decisive"] and all(a > 0 and b > 0 for a, b in p["foreign"].values())


def test_python_surface():
    import torch
    import dqo_eval
    import dqo_ply
    from dqo_harness.fused_mapping import FusedMapper
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dqo_eval.nearest_grouped) == ["query", "query_group", "ref", "ref_group", "query_transform", "ref_transform", "want_idx",
                                             "workspace_buffer"]
    assert sig(dqo_eval.eval_pcd_objects) == ["gt_points", "gt_object", "rec_points", "rec_object", "dist_thres", "transform", "out", "row",
                                              "workspace_buffer"]
    assert inspect.signature(dqo_eval.eval_pcd_objects).parameters["dist_thres"].default == (0.01,)
    assert sig(dqo_eval.eval_pcd_objects_dict) == ["table", "dist_thres"] and sig(dqo_eval.sample_surface_objects) == ["meshes", "count", "seed"]
    assert sig(FusedMapper.evaluate_geometry_objects) == ["self", "gt_points", "gt_object", "dist_thres", "transform", "rows", "out", "row"]
    assert inspect.signature(FusedMapper.evaluate_geometry_objects).parameters["rows"].default == "stable"
    assert sig(FusedMapper.evaluate_geometry_objects_mesh)[:4] == ["self", "meshes", "sample_nums", "seed"]
    assert inspect.signature(FusedMapper.evaluate_geometry_objects_mesh).parameters["sample_nums"].default == 1000000
    # the per-object files are a method of their own: save_model's signature is pinned by tests/test_checkpoint_abi.py and stays
    assert sig(FusedMapper.save_model) == ["self", "path", "save_data", "save_sibr", "save_merge"] and sig(FusedMapper.save_model_objects) == ["self", "path"]
    assert "metric_obj.py" in dqo_eval.__doc__
    z, ids = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32)
    for call in (lambda: dqo_eval.nearest_grouped(z, ids, z, ids), lambda: dqo_eval.eval_pcd_objects(z, ids, z, ids),
                 lambda: dqo_eval.sample_surface_objects({0: (z, torch.zeros(2, 3, dtype=torch.int32))}, 10)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert dqo_eval.object_seed(0, 0) == 0x9E3779B97F4A7C15 and dqo_eval.object_seed(2 ** 64 - 1, 0) == 0x9E3779B97F4A7C14
    assert len({dqo_eval.object_seed(7, g) for g in range(64)}) == 64
    # eval_pcd_objects_dict on a hand-made table: the rows that are not all NaN, ids ascending, each eval_pcd_dict's dict
    table = torch.full((64, 32), float("nan"))
    table[63, :10] = torch.tensor([8.5, 6.25, 0.1475, 2.0, 5.0, 4.0, 4.5, 19.0, 15.5, 17.0])
    table[5, :10] = torch.tensor([1.5, 2.5, 0.04, 2.0, 50.0, 25.0, 33.25, 0.0, 0.0, float("nan")])
    d = dqo_eval.eval_pcd_objects_dict(table, (0.005, 0.01))
    assert list(d) == [5, 63] and d[63] == dqo_eval.eval_pcd_dict(table[63], (0.005, 0.01))
    assert list(d[5]) == ["accuracy", "completion", "P (< 0.005)", "P (< 0.01)", "R (< 0.005)", "R (< 0.01)", "F1 (< 0.005)", "F1 (< 0.01)", "chamfer"]
    assert d[5]["accuracy"] == 1.5 and d[5]["R (< 0.005)"] == 25.0 and d[5]["P (< 0.01)"] == 0.0 and np.isnan(d[5]["F1 (< 0.01)"])
    assert d[63]["F1 (< 0.01)"] == 17.0 and d[63]["chamfer"] == pytest.approx(0.1475)
    with pytest.raises(RuntimeError, match="thresholds"):
        dqo_eval.eval_pcd_objects_dict(table, (0.01,))
    with pytest.raises(RuntimeError, match="table"):
        dqo_eval.eval_pcd_objects_dict(table[:3], (0.01,))
    # the per-object files of save_model_objects from a hand-made header: the reference's names, table order, only the objects with rows
    header = np.zeros((2, 64), np.int32)
    header[0, 3], header[0, 63], header[1, 0], header[1, 3] = 7, 2, 5, 11
    files = dqo_ply.object_file_slices("/x/map", header)
    assert files == [("/x/map_obj3.ply", 0, 7), ("/x/map_obj63.ply", 7, 2), ("/x/map_stable_obj0.ply", 9, 5), ("/x/map_stable_obj3.ply", 14, 11)]
    assert files == dqo_ply.object_file_slices("/x/map", header.reshape(-1).tolist()) and dqo_ply.object_file_slices("p", np.zeros(128)) == []
    assert files[0][0] == "/x/map" + "_obj" + "{}.ply".format(3)
