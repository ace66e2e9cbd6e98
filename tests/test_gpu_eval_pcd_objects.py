"""GPU: the per-object geometry evaluation — the grouped exact 1-NN search (dqo_nn1_grouped, csrc/knn.hip), the [64,32] table built on it
(dqo_eval.eval_pcd_objects, FusedMapper.evaluate_geometry_objects — csrc/map_eval.hip) and the per-object files
(dqo_map_pack_rows_by_object, csrc/map_checkpoint.hip; FusedMapper.save_model_objects), through the Python surface.

Bars, and why: those of tests/test_gpu_eval_pcd.py, whose helpers are used as they are.  dist2: bit for bit against
tests/pcd_group_oracle.py, and bit for bit the existing dqo_eval.nearest with the two keep masks of every group — all three are the
minimum of one float32 expression over the same references.  idx: any reference OF THE QUERY'S GROUP whose recomputed float32 distance
equals dist2.  Table rows: counts exactly, slots 0-2 and P / R / F1 within 3e-7 relative (_assert_row; the premises are asserted in
tests/test_pcd_group_oracle.py on the same cases); against the masked dqo_eval.eval_pcd: counts exactly, means within the same 3e-7
(the same distances, the sums in another order).  Files: bytes."""
import os

import numpy as np
import pytest

import pcd_group_oracle as go
import pcd_oracle as po
from checkpoint_cases import values
from test_gpu_eval_pcd import REL_BAR, XFORM, _assert_row, _bits, _cloud, _t
from test_pcd_group_oracle import objects

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0ABCD  # (a NaN with a payload: only a bit comparison sees it)


def _ids(a):
    return _t(np.asarray(a, np.int32))


def _check(q, qg, r, rg, xforms=(None, None), what=""):
    """dqo_eval.nearest_grouped against nn1_grouped_oracle (dist2 bit for bit, idx by its group and its recomputed distance) and against
    dqo_eval.nearest with the keep masks of every group of the queries.  Returns (dist2, idx) as numpy."""
    import torch
    import dqo_eval
    q, r, qg, rg = np.asarray(q, np.float32), np.asarray(r, np.float32), np.asarray(qg, np.int32), np.asarray(rg, np.int32)
    tq, tr = _t(q), _t(r)
    d, i = dqo_eval.nearest_grouped(tq, _ids(qg), tr, _ids(rg), xforms[0], xforms[1])
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (q.shape[0],)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    want_d, want_i, _ = go.nn1_grouped_oracle(q, qg, r, rg, xforms)
    wrong = np.nonzero(d.view(np.int32) != want_d.view(np.int32))[0]
    print(f"{what}: Q {q.shape[0]} R {r.shape[0]} differing dist2 {wrong.size}" + (f" first {wrong[0]}: {d[wrong[0]]!r} want {want_d[wrong[0]]!r}"
                                                                                   if wrong.size else ""))
    assert wrong.size == 0, what
    found = want_i >= 0
    assert ((i >= 0) == found).all() and (i[~found] == -1).all() and (i < max(r.shape[0], 1)).all(), what
    assert (rg[i[found]] == qg[found]).all(), what  # (only references of the query's own group are found)
    mq, mr = po.transform_f32(q, xforms[0]), po.transform_f32(r, xforms[1])
    assert po.dist2_f32(mq[found], mr[i[found]]).view(np.int32).tobytes() == d[found].view(np.int32).tobytes(), what
    for g in go.groups_of(qg):
        qk = qg == g
        md, _ = dqo_eval.nearest(tq, tr, _t(qk), _t(rg == g), xforms[0], xforms[1], want_idx=False)
        assert md.cpu().numpy()[qk].view(np.int32).tobytes() == d[qk].view(np.int32).tobytes(), (what, g)
    return d, i


def test_objects_in_both_directions():
    gt, gt_object, rec, rec_object, _, _ = objects()
    d, _ = _check(rec, rec_object, gt, gt_object, what="objects rec->gt")
    assert (d[rec_object == -1] == po.FLT_MAX).all()
    d, i = _check(gt, gt_object, rec, rec_object, what="objects gt->rec")
    assert (d[gt_object == 7] == po.FLT_MAX).all() and (i[gt_object == 7] == -1).all()  # (the object the map never saw)
    assert (rec_object[i[gt_object != 7]] >= 0).all()  # (no background row is ever found)


def test_all_64_ids_interleaved_and_rows_without_a_group():
    """40 rows a side of every id in one volume: a group is smaller than a run of 64 points and every bit of a record's group set is
    used; rows with ids -1, 64 and 1000 come back FLT_MAX / -1 and are found by nobody."""
    rng = np.random.default_rng(41)
    ids = np.concatenate([np.repeat(np.arange(64), 40), np.repeat(np.int32([-1, 64, 1000]), 30)]).astype(np.int32)
    qg, rg = rng.permutation(ids), rng.permutation(ids)
    q, r = _cloud(rng, ids.size, scale=(1.0, 1.0, 1.0)), _cloud(rng, ids.size, scale=(1.0, 1.0, 1.0))
    d, i = _check(q, qg, r, rg, what="64 ids")
    none = (qg < 0) | (qg >= 64)
    assert none.sum() == 90 and (d[none] == po.FLT_MAX).all() and (i[none] == -1).all() and (d[~none] < 1).all()
    assert ((rg[i[~none]] >= 0) & (rg[i[~none]] < 64)).all()


def test_a_group_of_more_than_64_boxes_beside_small_ones():
    """70 001 references of one group (69 level-1 boxes: more than one run of 64 of them), 65 of another and 1 of a third in the same
    volume; 3000 queries over the three groups and one group that has no reference."""
    rng = np.random.default_rng(42)
    rg = rng.permutation(np.concatenate([np.full(70001, 9), np.full(65, 10), np.full(1, 11)]).astype(np.int32))
    qg = rng.permutation(np.repeat(np.int32([9, 10, 11, 12]), 750))
    d, i = _check(_cloud(rng, 3000), qg, _cloud(rng, rg.size), rg, what="70001 + 65 + 1")
    assert (d[qg == 12] == po.FLT_MAX).all() and (i[qg == 12] == -1).all() and (d[qg != 12] < po.FLT_MAX).all()
    assert len(set(i[qg == 11].tolist())) == 1


def test_two_groups_with_identical_coordinates():
    rng = np.random.default_rng(43)
    c = _cloud(rng, 1500)
    r, rg = np.concatenate([c, c]), np.repeat(np.int32([1, 2]), 1500)
    q, qg = c[::3], (np.arange(500) % 2 + 1).astype(np.int32)
    d, i = _check(q, qg, r, rg, what="identical copies")
    assert (d == 0).all() and (rg[i] == qg).all() and (r[i] == q).all()  # every query finds its own group's copy
    # the other group's copy shifted: a query of group 1 still finds its own copy at distance 0, one of group 2 its shifted one
    shift = np.float32([0.002, -0.001, 0.0015])
    d, i = _check(q, qg, np.concatenate([c, c + shift]), rg, what="one copy shifted")
    assert (d[qg == 1] == 0).all() and (i[qg == 1] < 1500).all() and (d[qg == 2] > 0).all() and (i[qg == 2] >= 1500).all()


def test_queries_far_outside_the_references_box():
    rng = np.random.default_rng(44)
    r, rg = _cloud(rng, 3000, offset=(1.0, 1.0, 1.0)), rng.integers(0, 3, 3000).astype(np.int32)
    q = np.concatenate([_cloud(rng, 600, scale=(20, 20, 20), offset=(-8, -8, -8)), _cloud(rng, 100, offset=(1.0, 1.0, 1.0))])
    assert (q < 0).any(axis=0).all() and (q > r.max(axis=0)).any(axis=0).all()
    _check(q, rng.integers(0, 3, 700).astype(np.int32), r, rg, what="outside")


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1023, 1025])
def test_group_sizes_around_a_run_and_a_box(R):
    """Two interleaved groups of R references each (and a few rows without one), 200 queries over both."""
    rng = np.random.default_rng(200 + R)
    rg = rng.permutation(np.concatenate([np.full(R, 20), np.full(R, 21), np.full(7, -1)]).astype(np.int32))
    _check(_cloud(rng, 200), rng.integers(20, 22, 200).astype(np.int32), _cloud(rng, rg.size), rg, what=f"R={R} per group")


def test_transforms_on_either_side():
    gt, gt_object, rec, rec_object, _, _ = objects()
    _check(rec, rec_object, gt, gt_object, xforms=(XFORM, None), what="query transform")
    _check(gt, gt_object, rec, rec_object, xforms=(None, XFORM), what="reference transform")
    full = np.concatenate([XFORM, np.float32([[0, 0, 0, 1]])])
    _check(gt[:500], gt_object[:500], rec, rec_object, (full, full), what="both, [4,4]")


def test_empty_sets_and_rows_without_a_group():
    rng = np.random.default_rng(45)
    q, r = _cloud(rng, 300), _cloud(rng, 400)
    qg, rg = rng.integers(0, 4, 300).astype(np.int32), rng.integers(0, 4, 400).astype(np.int32)
    d, i = _check(np.zeros((0, 3), np.float32), np.zeros((0,), np.int32), r, rg, what="Q=0")
    assert d.shape == (0,) and i.shape == (0,)
    d, i = _check(q, qg, np.zeros((0, 3), np.float32), np.zeros((0,), np.int32), what="R=0")
    assert (d == po.FLT_MAX).all() and (i == -1).all()
    for name, a, b in (("no query has a group", np.full(300, -1, np.int32), rg), ("no reference has a group", qg, np.full(400, 64, np.int32)),
                       ("nobody has a group", np.full(300, -5, np.int32), np.full(400, 1 << 20, np.int32))):
        d, i = _check(q, a, r, b, what=name)
        assert (d == po.FLT_MAX).all() and (i == -1).all(), name


# ---- the [64,32] table ------------------------------------------------------------------------------------------------------------------
def _assert_table(table, gt, gt_object, rec, rec_object, thres, what, transform=None):
    """Every one of the 64 rows against eval_pcd_objects_oracle (_assert_row's bars; NaN rows for the objects without rows on both
    sides) and against the existing dqo_eval.eval_pcd with that object's keep masks (counts exactly, means within REL_BAR)."""
    import dqo_eval
    table = np.asarray(table, np.float32)
    assert table.shape == (64, 32)
    want = go.eval_pcd_objects_oracle(gt, gt_object, rec, rec_object, thres, transform)
    tg, tr = _t(gt), _t(rec)
    for g in range(64):
        if g not in want:
            assert np.isnan(table[g]).all(), (what, g)
            continue
        _, _, n_rec, n_gt, d_rec64, d_gt64 = want[g]
        _assert_row(table[g], n_gt, n_rec, d_rec64, d_gt64, thres, f"{what} object {g}")
        masked = dqo_eval.eval_pcd(tg, tr, thres, transform, gt_keep=_t(gt_object == g), rec_keep=_t(rec_object == g)).cpu().numpy().astype(np.float64)
        a = table[g].astype(np.float64)
        assert a[3] == masked[3] == len(thres)
        for t in range(len(thres)):
            for s, n in ((4 + 3 * t, n_rec), (5 + 3 * t, n_gt)):
                assert round(a[s] * n / 100) == round(masked[s] * n / 100), (what, g, s)
        assert (np.abs(a[:3] - masked[:3]) <= REL_BAR * np.abs(masked[:3])).all(), (what, g)


def test_eval_pcd_objects_on_objects():
    import torch
    import dqo_eval
    gt, gt_object, rec, rec_object, _, _ = objects()
    th = go.OBJECTS_THRES
    g, gg, r, rg = _t(gt), _ids(gt_object), _t(rec), _ids(rec_object)
    a = dqo_eval.eval_pcd_objects(g, gg, r, rg, th)
    b = dqo_eval.eval_pcd_objects(g, gg, r, rg, th)
    table = torch.full((66, 32), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    c = dqo_eval.eval_pcd_objects(g, gg, r, rg, th, out=table, row=1)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and tuple(a.shape) == (64, 32) and a.is_cuda and c.data_ptr() == table[1].data_ptr() and tuple(c.shape) == (64, 32)
    _assert_table(a.cpu().numpy(), gt, gt_object, rec, rec_object, th, "objects")
    assert np.isnan(a[7].cpu().numpy()).all()  # the ground-truth object the map never saw
    assert _bits(a).tobytes() == _bits(b).tobytes()  # two calls: identical bytes
    t = _bits(table)
    assert t[1:65].tobytes() == _bits(a).tobytes() and (t[[0, 65]] == SENTINEL).all()
    d = dqo_eval.eval_pcd_objects_dict(a, th)
    host = a.cpu().numpy()
    assert list(d) == [0, 5, 63] and all(d[k]["accuracy"] == host[k, 0] and d[k]["F1 (< 0.01)"] == host[k, 9] and len(d[k]) == 9 for k in d)
    # the default threshold is metric_obj.py's 0.01; a transform: the reconstruction stored in another frame comes back under the motion
    one = dqo_eval.eval_pcd_objects(g, gg, r, rg).cpu().numpy()
    assert (one[[0, 5, 63], 3] == 1).all() and one[[0, 5, 63], 4:7].tolist() == host[[0, 5, 63], 7:10].tolist() and np.isnan(one[:, 7:]).all()
    stored = go.objects_stored_case()[2]
    moved = dqo_eval.eval_pcd_objects(g, gg, _t(stored), rg, th, transform=go.OBJECTS_XFORM).cpu().numpy()
    _assert_table(moved, gt, gt_object, stored, rec_object, th, "moved", transform=go.OBJECTS_XFORM)
    with pytest.raises(RuntimeError, match="rows"):
        dqo_eval.eval_pcd_objects(g, gg, r, rg, th, out=table, row=3)


def test_eval_pcd_objects_nan_tables():
    import dqo_eval
    gt, gt_object, rec, rec_object, _, _ = objects()
    g, gg, r, rg = _t(gt), _ids(gt_object), _t(rec), _ids(rec_object)
    empty, none = _t(np.zeros((0, 3), np.float32)), _ids(np.zeros((0,), np.int32))
    for name, args in (("no reconstruction", (g, gg, empty, none)), ("no ground truth", (empty, none, r, rg)), ("both empty", (empty, none, empty, none)),
                       ("no row has an object", (g, _ids(np.full(9000, -1)), r, _ids(np.full(9000, 64)))),
                       ("no object in common", (g, _ids(np.where(gt_object == 7, 7, -1)), r, rg))):
        assert np.isnan(dqo_eval.eval_pcd_objects(*args, go.OBJECTS_THRES).cpu().numpy()).all(), name
    # no distance under the threshold: P = R = 0 and F1 = 0 / 0
    far = dqo_eval.eval_pcd_objects(g, gg, _t(rec + np.float32([0, 0, 10.0])), rg, (0.01,)).cpu().numpy()
    assert (far[[0, 5, 63], 4] == 0).all() and (far[[0, 5, 63], 5] == 0).all() and np.isnan(far[[0, 5, 63], 6]).all() and (far[[0, 5, 63], 0] > 900).all()


def test_eval_pcd_objects_more_partials_than_one_stage_of_the_last_block():
    import torch
    import dqo_eval
    gt, gt_object, rec, rec_object = go.two_groups_case()
    g, gg, r, rg = _t(gt), _ids(gt_object), _t(rec), _ids(rec_object)
    a = dqo_eval.eval_pcd_objects(g, gg, r, rg, go.TWO_GROUPS_THRES)
    b = dqo_eval.eval_pcd_objects(g, gg, r, rg, go.TWO_GROUPS_THRES)
    torch.cuda.synchronize()
    _assert_table(a.cpu().numpy(), gt, gt_object, rec, rec_object, go.TWO_GROUPS_THRES, "two groups")
    assert _bits(a).tobytes() == _bits(b).tobytes()


def test_ten_calls_on_one_stream_and_a_captured_graph():
    import torch
    import dqo_eval
    gt, gt_object, rec, rec_object, _, _ = objects()
    th = go.OBJECTS_THRES
    g, gg, r, rg = _t(gt), _ids(gt_object), _t(rec), _ids(rec_object)
    table = torch.zeros((640, 32), dtype=torch.float32, device="cuda")
    for k in range(10):  # (the module's workspace, shared: the ticket words come back zero)
        dqo_eval.eval_pcd_objects(g, gg, r, rg, th, out=table, row=64 * k)
    torch.cuda.synchronize()
    t = _bits(table).reshape(10, 64, 32)
    assert all(t[k].tobytes() == t[0].tobytes() for k in range(10)) and np.isfinite(table[5, :10].cpu().numpy()).all()
    out = torch.zeros((64, 32), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dqo_eval.eval_pcd_objects(g, gg, r, rg, th, out=out, row=0)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(out).tobytes() == t[0].tobytes()


# ---- FusedMapper ------------------------------------------------------------------------------------------------------------------------
def _gated_mapper():
    """The 1700-row frustum scene of test_gpu_eval_pcd with reserve(300), holes in `alive`, an object gate of five ids and a stable pattern."""
    import torch
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    scene = scenes.frustum_cloud(17, 1700, cam)
    fm = FusedMapper(scene, mapping.make_settings(cam, dev), dev).reserve(300)
    fm.alive[5:1700:9] = 0
    ids = np.array([2, 7, 11, 40, 63], np.int32)[np.arange(2000) % 5]
    return dev, cam, scene, fm, ids


def test_evaluate_geometry_objects_equals_eval_pcd_objects_on_the_gathered_rows():
    import torch
    import dqo_eval
    dev, cam, scene, fm, ids = _gated_mapper()
    rng = np.random.default_rng(12)
    gt = _t((np.asarray(scene["xyz"], np.float32)[::2] + rng.normal(0, 0.02, (850, 3))).astype(np.float32))
    gt_object = _ids(ids[:1700:2])
    th = (0.02, 0.05)
    with pytest.raises(RuntimeError, match="set_object_gate"):
        fm.evaluate_geometry_objects(gt, gt_object, th, rows="all")
    fm.set_object_gate(ids, np.zeros((cam.H, cam.W), np.int32))
    with pytest.raises(RuntimeError, match="track_lifecycle"):
        fm.evaluate_geometry_objects(gt, gt_object, th)
    stable = torch.arange(2000, device=dev) % 3 != 0
    fm.track_lifecycle(stable_mask=stable)
    alive = fm.alive.bool()
    mask = torch.arange(2000, device=dev) % 4 != 1
    for rows, take in (("stable", alive & stable), ("all", alive), (mask, alive & mask)):
        got = fm.evaluate_geometry_objects(gt, gt_object, th, rows=rows)
        want = dqo_eval.eval_pcd_objects(gt, gt_object, fm.xyz.detach()[take].contiguous(), fm.gaussian_object[take].contiguous(), th)
        torch.cuda.synchronize()
        g, w = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
        live = [2, 7, 11, 40, 63]
        assert np.isfinite(g[live, :6]).all() and np.isnan(np.delete(g, live, axis=0)).all() and np.isnan(g[:, 10:]).all() and (g[live, 3] == 2).all()
        np.testing.assert_allclose(g[live, :10], w[live, :10], rtol=REL_BAR, atol=0, equal_nan=True, err_msg=str(rows))
        for k in live:
            n_rec, n_gt = int((take & (fm.gaussian_object == k)).sum().item()), 170
            for s, n in ((4, n_rec), (5, n_gt), (7, n_rec), (8, n_gt)):
                assert round(g[k, s] * n / 100) == round(w[k, s] * n / 100) and abs(g[k, s] * n / 100 - round(g[k, s] * n / 100)) < 1e-3
    table = torch.zeros((66, 32), dtype=torch.float32, device=dev)
    out = fm.evaluate_geometry_objects(gt, gt_object, th, rows=mask, out=table, row=2)
    torch.cuda.synchronize()
    assert out.data_ptr() == table[2].data_ptr() and _bits(table[2:]).tobytes() == _bits(got).tobytes() and not table[:2].any()
    with pytest.raises(RuntimeError, match="rows"):
        fm.evaluate_geometry_objects(gt, gt_object, th, rows="unstable")


def test_evaluate_geometry_objects_mesh_equals_the_chain_by_hand():
    import torch
    import dqo_eval
    dev, cam, scene, fm, ids = _gated_mapper()
    fm.set_object_gate(ids, np.zeros((cam.H, cam.W), np.int32))
    fm.track_lifecycle(stable_mask=torch.arange(2000, device=dev) % 3 != 0)
    xyz = np.asarray(scene["xyz"], np.float32)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    quad = lambda z: (_t(np.float32([[lo[0], lo[1], z], [hi[0], lo[1], z], [hi[0], hi[1], z], [lo[0], hi[1], z]])), _ids([[0, 1, 2], [0, 2, 3]]))
    meshes = {7: quad(float(np.median(xyz[:, 2]))), 40: quad(float(lo[2]))}
    th = (0.5, 1.0)
    got = fm.evaluate_geometry_objects_mesh(meshes, sample_nums=3000, seed=5, dist_thres=th)
    points, objects_ = dqo_eval.sample_surface_objects(meshes, 3000, seed=5)
    for k, g in enumerate((7, 40)):  # each object's part is exactly sample_surface with the documented seed
        s = dqo_eval.sample_surface(*meshes[g], 3000, seed=dqo_eval.object_seed(5, g))
        assert _bits(points[3000 * k:3000 * (k + 1)]).tobytes() == _bits(s["points"]).tobytes() and (objects_[3000 * k:3000 * (k + 1)] == g).all()
    take = fm.stable_rows()
    want = dqo_eval.eval_pcd_objects(points, objects_, fm.xyz.detach()[take].contiguous(), fm.gaussian_object[take].contiguous(), th)
    torch.cuda.synchronize()
    g, w = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
    assert tuple(points.shape) == (6000, 3) and objects_.dtype == torch.int32
    assert np.isfinite(g[[7, 40], :6]).all() and np.isnan(np.delete(g, [7, 40], axis=0)).all()
    np.testing.assert_allclose(g[[7, 40], :10], w[[7, 40], :10], rtol=REL_BAR, atol=0, equal_nan=True)
    # a mesh without area: its rows get object -1, its table row is NaN
    flat = (_t(np.zeros((3, 3), np.float32)), _ids([[0, 1, 2]]))
    p2, o2 = dqo_eval.sample_surface_objects({7: meshes[7], 11: flat}, 100)
    assert (o2[:100] == 7).all() and (o2[100:] == -1).all()
    assert np.isnan(fm.evaluate_geometry_objects_mesh({11: flat}, sample_nums=100).cpu().numpy()).all()


# ---- the per-object files ---------------------------------------------------------------------------------------------------------------
def _read(path):
    return open(path, "rb").read()


def _expected_object_files(prefix, v, alive, stable, obj):
    """{file: rows} written through dqo_ply.save_model_ply (without confidence) of the rows gathered on the host in ascending row order."""
    import dqo_ply
    host = {k: a.detach().cpu().numpy() for k, a in v.items()}
    alive, stable, obj = alive.cpu().numpy() != 0, stable.cpu().numpy() != 0, obj.cpu().numpy()
    files = {}
    for cloud, tag in ((alive & ~stable, "_obj"), (alive & stable, "_stable_obj")):
        for g in range(64):
            rows = np.nonzero(cloud & (obj == g))[0]
            if rows.size:
                name = prefix + tag + "{}.ply".format(g)
                dqo_ply.save_model_ply(name, host["xyz"][rows], host["shs"][rows], host["opacity_raw"][rows], host["scaling_raw"][rows],
                                       host["rotation_raw"][rows], include_confidence=False)
                files[name] = int(rows.size)
    return files


@pytest.mark.parametrize("M", [4, 16])
def test_pack_rows_by_object_is_save_model_ply_of_every_objects_rows(tmp_path, M):
    import torch
    import dqo_ply
    P, dev = 2000, torch.device("cuda")
    v = {k: torch.from_numpy(a).to(dev) for k, a in values(P, M, 77 + M).items()}
    rng = np.random.default_rng(M)
    alive = (rng.random(P) < 0.8).astype(np.uint8) * rng.choice(np.array([1, 2, 200], np.uint8), size=P)
    alive[1700:] = 0  # spare rows behind the map, dead rows among it
    stable = (rng.random(P) < 0.5).astype(np.uint8) * 3
    obj = rng.choice(np.array([0, 3, 17, 40, 63, -1, 64], np.int32), size=P)  # five objects, and rows without one
    alive, stable, obj = torch.from_numpy(alive).to(dev), torch.from_numpy(stable).to(dev), torch.from_numpy(obj).to(dev)
    C = 6 + 3 * M + 8
    ws = dqo_ply.pack_workspace(P, dev)
    runs = []
    for _ in range(2):
        table = torch.full((P + 3, C), 0x5EA7AB1E, dtype=torch.int32, device=dev).view(torch.float32)
        header = torch.full((2, 64), -7, dtype=torch.int32, device=dev)
        out = dqo_ply.pack_rows_by_object(v["xyz"], v["shs"], v["opacity_raw"], v["scaling_raw"], v["rotation_raw"], obj, v["confidence"], alive, stable,
                                          out=table, header=header, workspace_buffer=ws)
        torch.cuda.synchronize()
        assert out[0] is table and out[1] is header and not ws.any()
        runs.append((table.view(torch.int32).cpu().numpy().view(np.uint32), header.cpu().numpy()))
    (t0, h0), (t1, h1) = runs
    assert t0.tobytes() == t1.tobytes() and h0.tobytes() == h1.tobytes()
    want = _expected_object_files(str(tmp_path / "want"), v, alive, stable, obj)
    slices = dqo_ply.object_file_slices(str(tmp_path / "want"), h0)
    assert {name: n for name, _, n in slices} == want and len(want) == 10  # the header counts are exact
    total = int(h0.sum())
    assert (t0[total:] == 0x5EA7AB1E).all() and total < 1700  # rows behind the total keep their bytes
    for name, first, n in slices:
        got = str(tmp_path / "got.ply")
        assert dqo_ply.write_vertex_table(got, t0.view(np.float32)[first:first + n], 3 * (M - 1), False) == n
        assert _read(got) == _read(name), os.path.basename(name)
    # with the confidence column the rows are the same rows, one column wider
    wide, _ = dqo_ply.pack_rows_by_object(v["xyz"], v["shs"], v["opacity_raw"], v["scaling_raw"], v["rotation_raw"], obj, v["confidence"], alive, stable,
                                          include_confidence=True)
    wide = wide.view(torch.int32).cpu().numpy().view(np.uint32)[:total]
    assert np.array_equal(wide[:, :C], t0[:total]) and wide.shape[1] == C + 1


def test_save_model_objects_writes_the_per_object_files(tmp_path):
    import torch
    dev, cam, scene, fm, ids = _gated_mapper()
    with pytest.raises(RuntimeError, match="set_object_gate"):
        fm.save_model_objects(str(tmp_path / "none"))
    fm.set_object_gate(ids, np.zeros((cam.H, cam.W), np.int32))
    fm.track_lifecycle(stable_mask=torch.arange(2000, device=dev) % 3 != 0)
    plain = fm.save_model(str(tmp_path / "plain"))
    before = {f: _read(f) for f in plain}
    assert sorted(os.path.basename(f) for f in plain) == sorted(os.listdir(tmp_path)) and len(plain) == 6  # save_model writes today's files
    v = dict(xyz=fm.xyz, shs=fm.shs, opacity_raw=fm.opacity_raw, scaling_raw=fm.scaling_raw, rotation_raw=fm.rotation_raw)
    want = _expected_object_files(str(tmp_path / "want"), v, fm.alive, fm.stable, fm.gaussian_object)
    got = fm.save_model_objects(str(tmp_path / "got"))
    assert len(want) == 10 and {os.path.basename(f).replace("got", "want"): n for f, n in got.items()} == {os.path.basename(f): n for f, n in want.items()}
    for f in want:
        assert _read(f) == _read(os.path.join(os.path.dirname(f), os.path.basename(f).replace("want", "got"))), os.path.basename(f)
    assert len(os.listdir(tmp_path)) == 26 and all(_read(f) == blob for f, blob in before.items())
    again = fm.save_model(str(tmp_path / "plain"))  # ... and save_model after it: the shared buffers are in order
    assert again == plain and all(_read(f) == blob for f, blob in before.items())
    # the files hold the map: an object's stable file, read back, is the stable rows of that object in row order
    import dqo_ply
    props, table = dqo_ply.read_vertex_table(str(tmp_path / "got_stable_obj40.ply"))
    rows = (fm.stable_rows() & (fm.gaussian_object == 40)).nonzero().reshape(-1)
    assert "confidence" not in props and np.array_equal(table[:, :3], fm.xyz.detach()[rows].cpu().numpy())
