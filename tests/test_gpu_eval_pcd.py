"""GPU: the dense exact 1-NN search (dqo_nn1, csrc/knn.hip) bit for bit against tests/pcd_oracle.py, and the geometry metrics built on it
(dqo_eval.eval_pcd, FusedMapper.evaluate_geometry — csrc/map_eval.hip) against the float64 restatement of SLAM/eval.py:190-282.

Bars, and why.  dist2: bit for bit — the kernel and nn1_oracle both return the minimum of one float32 expression over the kept references.
idx: any reference whose recomputed float32 distance equals dist2.  Counts (P n / 100, R n / 100): exactly — both sides of the kernel's
threshold test are exact in double, and on "room" no point lies within 1e-4 relative of a threshold (tests/test_pcd_oracle.py asserts that
premise); a count is read back from a float32 percentage below 128, whose half ulp of 2^-18 is 3.8e-8 n rows: the product lies within
max(1e-3, 4e-8 n) of the integer (1e-3 up to 25 000 rows).  Slots 0-2 and P / R / F1: 3e-7 relative — the float32 distances are within
2e-7 relative of scipy's, plus two roundings to float32 (6e-8 each) and a double sum in another order."""
import numpy as np
import pytest

import pcd_oracle as po
from test_pcd_oracle import THRES, room

pytestmark = pytest.mark.gpu

REL_BAR = 3e-7
XFORM = np.array([[0.8, -0.6, 0.0, 0.25], [0.6, 0.8, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125]], np.float32)


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.asarray(a, dtype), device="cuda")


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _check(q, r, keeps=(None, None), xforms=(None, None), what=""):
    """dqo_eval.nearest against nn1_oracle: dist2 bit for bit, idx by its recomputed distance.  Returns (dist2, idx) as numpy."""
    import torch
    import dqo_eval
    q, r = np.asarray(q, np.float32), np.asarray(r, np.float32)
    d, i = dqo_eval.nearest(_t(q), _t(r), _t(keeps[0], np.uint8), _t(keeps[1], np.uint8), xforms[0], xforms[1])
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (q.shape[0],)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    want_d, want_i, _ = po.nn1_oracle(q, r, keeps, xforms)
    wrong = np.nonzero(d.view(np.int32) != want_d.view(np.int32))[0]
    print(f"{what}: Q {q.shape[0]} R {r.shape[0]} differing dist2 {wrong.size}" + (f" first {wrong[0]}: {d[wrong[0]]!r} want {want_d[wrong[0]]!r}"
                                                                                   if wrong.size else ""))
    assert wrong.size == 0, what
    found = want_i >= 0
    assert ((i >= 0) == found).all() and (i[~found] == -1).all() and (i < r.shape[0]).all(), what
    if keeps[1] is not None:
        assert np.asarray(keeps[1]).astype(bool)[i[found]].all(), what  # (only kept references are found)
    tq, tr = po.transform_f32(q, xforms[0]), po.transform_f32(r, xforms[1])
    assert po.dist2_f32(tq[found], tr[i[found]]).view(np.int32).tobytes() == d[found].view(np.int32).tobytes(), what
    return d, i


def _cloud(rng, n, scale=(4.0, 3.0, 2.5), offset=(0.0, 0.0, 0.0)):
    return (rng.uniform(0, 1, (n, 3)) * np.asarray(scale) + np.asarray(offset)).astype(np.float32)


def test_room_in_both_directions():
    gt, rec, _, _ = room()
    _check(rec, gt, what="room rec->gt")
    _check(gt, rec, what="room gt->rec")


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1023, 1025])
def test_reference_sizes_around_a_run_and_a_box(R):
    rng = np.random.default_rng(100 + R)
    _check(_cloud(rng, 200), _cloud(rng, R), what=f"R={R}")


def test_one_query_and_more_than_one_group_of_boxes():
    rng = np.random.default_rng(7)
    _check(_cloud(rng, 1), _cloud(rng, 5000), what="Q=1")
    # 70 001 references: 69 level-1 boxes = more than one run of 64 of them, and a ragged last run of points
    _check(_cloud(rng, 3000), _cloud(rng, 70001), what="R=70001")


def test_queries_outside_the_references_box_and_references_far_from_the_origin():
    rng = np.random.default_rng(8)
    r = _cloud(rng, 3000, offset=(1.0, 1.0, 1.0))
    # beyond every face of the references' bounding box (which holds the origin): the clamped Morton code
    q = np.concatenate([_cloud(rng, 600, scale=(20, 20, 20), offset=(-8, -8, -8)), _cloud(rng, 100, offset=(1.0, 1.0, 1.0))])
    assert (q < 0).any(axis=0).all() and (q > r.max(axis=0)).any(axis=0).all()
    _check(q, r, what="outside")
    # references 50 m from the origin: the grid is laid from the origin (the bounding box always contains it), its cells are coarse
    far = _cloud(rng, 3000, offset=(50.0, -40.0, 30.0))
    _check(far[:500] + rng.normal(0, 0.02, (500, 3)).astype(np.float32), far, what="far")


def test_duplicates_identical_references_and_ties():
    rng = np.random.default_rng(9)
    r = _cloud(rng, 2000)
    q = np.concatenate([r[::4], _cloud(rng, 300)])
    d, _ = _check(q, r, what="duplicates")
    assert (d[:500] == 0).all() and (d[500:] > 0).all()
    d, i = _check(_cloud(rng, 300), np.tile(np.float32([[1.5, 0.25, 2.0]]), (700, 1)), what="identical")
    assert (d > 0).all()
    # two references at the same distance from a query, on either side of it: either index, one distance
    r = np.float32([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0], [9.0, 9.0, 9.0]])
    d, i = _check(np.float32([[2.0, 1.0, 1.0], [2.0, 3.0, 1.0]]), r, what="ties")
    assert d.tolist() == [1.0, 5.0] and set(i.tolist()) <= {0, 1}


def test_masks_equal_the_search_on_the_gathered_subsets():
    import torch
    import dqo_eval
    gt, rec, _, _ = room()
    rng = np.random.default_rng(10)
    qk, rk = rng.uniform(size=rec.shape[0]) < 0.5, rng.uniform(size=gt.shape[0]) < 0.5
    # dropped rows hold what spare rows of a map hold: a far parking position — it must not stretch the grid
    rec2, gt2 = rec.copy(), gt.copy()
    rec2[~qk], gt2[~rk] = np.float32([0, 0, -1000.0]), np.float32([0, 0, -1000.0])
    d, i = _check(rec2, gt2, (qk, rk), what="masks")
    assert (d[~qk] == po.FLT_MAX).all() and (i[~qk] == -1).all()
    sub_d, sub_i = dqo_eval.nearest(_t(rec[qk]), _t(gt[rk]))
    torch.cuda.synchronize()
    assert d[qk].view(np.int32).tobytes() == _bits(sub_d).tobytes()
    rows = np.nonzero(rk)[0]
    assert po.dist2_f32(rec[qk], gt[rows[sub_i.cpu().numpy()]]).view(np.int32).tobytes() == d[qk].view(np.int32).tobytes()
    # every reference dropped
    d, i = _check(rec, gt, (None, np.zeros(gt.shape[0], bool)), what="no reference")
    assert (d == po.FLT_MAX).all() and (i == -1).all()
    d, i = _check(rec[:10], np.zeros((0, 3), np.float32), what="R=0")
    assert (d == po.FLT_MAX).all() and (i == -1).all()


def _half_dropped(seed, Q=200, R=1025):
    """Q queries against R references (one full box of 1024 and one row: a ragged last run), and a keep mask for each side that drops
    half its rows; `parked` puts a side's dropped rows where spare rows of a map lie."""
    rng = np.random.default_rng(seed)
    q, r = _cloud(rng, Q), _cloud(rng, R)
    qk, rk = np.arange(Q) % 2 == 0, rng.permutation(R) % 2 == 0

    def parked(x, keep):
        x = x.copy()
        x[~keep] = np.float32([0, 0, -1000.0])
        return x
    return q, r, qk, rk, parked


@pytest.mark.parametrize("side", ["query", "reference"])
def test_a_keep_mask_on_one_side_only(side):
    """A masked query set against a reference set built without groups, and every query against a masked reference set."""
    q, r, qk, rk, parked = _half_dropped(13)
    if side == "query":
        d, i = _check(parked(q, qk), r, (qk, None), what="query mask only")
        assert (d[~qk] == po.FLT_MAX).all() and (i[~qk] == -1).all() and (d[qk] < po.FLT_MAX).all()
    else:
        d, i = _check(q, parked(r, rk), (None, rk), what="reference mask only")
        assert (d < po.FLT_MAX).all() and rk[i].all()


def test_ids_0_and_minus_1_are_the_two_keep_masks():
    """nearest_grouped with one object is nearest with that object's two keep masks: dist2 and idx, bit for bit."""
    import torch
    import dqo_eval
    q, r, qk, rk, parked = _half_dropped(14)
    tq, tr = _t(parked(q, qk)), _t(parked(r, rk))
    gd, gi = dqo_eval.nearest_grouped(tq, _t(np.where(qk, 0, -1), np.int32), tr, _t(np.where(rk, 0, -1), np.int32))
    md, mi = dqo_eval.nearest(tq, tr, _t(qk, np.uint8), _t(rk, np.uint8))
    torch.cuda.synchronize()
    assert _bits(gd).tobytes() == _bits(md).tobytes() and gi.cpu().numpy().tobytes() == mi.cpu().numpy().tobytes()
    assert (mi.cpu().numpy()[qk] >= 0).all() and (mi.cpu().numpy()[~qk] == -1).all()


def test_transforms_match_the_oracles_restatement():
    gt, rec, _, _ = room()
    _check(rec, gt, xforms=(XFORM, None), what="query transform")
    _check(gt, rec, xforms=(None, XFORM), what="reference transform")
    full = np.concatenate([XFORM, np.float32([[0, 0, 0, 1]])])
    _check(gt[:500], rec, (None, np.arange(rec.shape[0]) % 3 != 0), (full, full), what="both, [4,4], masked")


def _assert_row(got, gt_n, rec_n, d_rec64, d_gt64, thres, what):
    want, counts = po.eval_pcd_oracle(d_rec64, d_gt64, thres)
    got = np.asarray(got, np.float64)
    assert got.shape == (32,) and got[3] == len(thres) and np.isnan(got[4 + 3 * len(thres):]).all(), what
    pairs = [("accuracy", 0), ("completion", 1), ("chamfer", 2)]
    for t, th in enumerate(thres):
        pairs += [(f"P (< {th})", 4 + 3 * t), (f"R (< {th})", 5 + 3 * t), (f"F1 (< {th})", 6 + 3 * t)]
        p_count, r_count = got[4 + 3 * t] * rec_n / 100, got[5 + 3 * t] * gt_n / 100
        print(f"{what} th {th}: counts {p_count!r} {r_count!r} want {counts[t]}")
        assert abs(p_count - round(p_count)) < max(1e-3, 4e-8 * rec_n) and abs(r_count - round(r_count)) < max(1e-3, 4e-8 * gt_n), what
        assert (round(p_count), round(r_count)) == counts[t], what
    for key, slot in pairs:
        g, w = got[slot], float(want[key])
        print(f"{what} {key:14s} got {g!r} want {w!r}")
        if np.isnan(w):
            assert np.isnan(g), (what, key)
        else:
            assert abs(g - w) <= REL_BAR * abs(w), (what, key, g, w)


def test_eval_pcd_on_room():
    import torch
    import dqo_eval
    gt, rec, (_, _, d_rec64), (_, _, d_gt64) = room()
    g, r = _t(gt), _t(rec)
    a = dqo_eval.eval_pcd(g, r, THRES)
    b = dqo_eval.eval_pcd(g, r, THRES)
    sentinel = 0x7FC0ABCD  # (a NaN with a payload: only a bit comparison sees it)
    table = torch.full((3, 32), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    c = dqo_eval.eval_pcd(g, r, THRES, out=table, row=1)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and tuple(a.shape) == (32,) and a.is_cuda and c.data_ptr() == table[1].data_ptr()
    _assert_row(a.cpu().numpy(), gt.shape[0], rec.shape[0], d_rec64, d_gt64, THRES, "room")
    assert _bits(a).tobytes() == _bits(b).tobytes()
    t = _bits(table)
    assert t[1].tobytes() == _bits(a).tobytes() and (t[[0, 2]] == sentinel).all()
    d = dqo_eval.eval_pcd_dict(a, THRES)
    row = a.cpu().numpy()
    assert d["accuracy"] == row[0] and d["completion"] == row[1] and d["chamfer"] == row[2] and d["F1 (< 0.03)"] == row[9]
    assert list(d)[:3] == ["accuracy", "completion", "P (< 0.01)"] and len(d) == 9
    # the default threshold, and a transform: the reconstruction stored in another frame comes back under the inverse motion
    one = dqo_eval.eval_pcd(g, r).cpu().numpy()
    assert one[3] == 1 and one[4:7].tolist() == row[7:10].tolist() and np.isnan(one[7:]).all()
    R3, t3 = XFORM[:, :3].astype(np.float64), XFORM[:, 3].astype(np.float64)
    stored = ((rec.astype(np.float64) - t3) @ R3).astype(np.float32)  # (R orthonormal: its inverse is its transpose)
    moved = po.transform_f32(stored, XFORM)
    dd = po.kdtree_distances(gt, moved)
    _assert_row(dqo_eval.eval_pcd(g, _t(stored), THRES, transform=XFORM).cpu().numpy(), gt.shape[0], rec.shape[0], dd[0], dd[1], THRES, "moved")


def test_eval_pcd_masks_and_nan_rows():
    import torch
    import dqo_eval
    gt, rec, _, _ = room()
    rng = np.random.default_rng(11)
    gk, rk = rng.uniform(size=gt.shape[0]) < 0.5, rng.uniform(size=rec.shape[0]) < 0.5
    got = dqo_eval.eval_pcd(_t(gt), _t(rec), THRES, gt_keep=_t(gk), rec_keep=_t(rk)).cpu().numpy()
    dd = po.kdtree_distances(gt[gk], rec[rk])
    _assert_row(got, int(gk.sum()), int(rk.sum()), dd[0], dd[1], THRES, "masked")
    # an empty kept set on either side: a row of NaN
    for kw in (dict(gt_keep=_t(np.zeros(gt.shape[0], np.uint8))), dict(rec_keep=_t(np.zeros(rec.shape[0], np.uint8)))):
        assert np.isnan(dqo_eval.eval_pcd(_t(gt), _t(rec), THRES, **kw).cpu().numpy()).all(), list(kw)
    assert np.isnan(dqo_eval.eval_pcd(_t(gt), _t(np.zeros((0, 3), np.float32)), THRES).cpu().numpy()).all()
    # no distance under the threshold: P = R = 0 and F1 = 0 / 0
    far = dqo_eval.eval_pcd(_t(gt), _t(rec + np.float32([0, 0, 10.0])), (0.03,)).cpu().numpy()
    assert far[4] == 0 and far[5] == 0 and np.isnan(far[6]) and far[0] > 700 and far[3] == 1


def test_eval_pcd_more_blocks_than_one_stage_of_the_last_block():
    """70 001 + 66 000 points, uniform in the unit cube: 69 + 65 blocks of 1 024 rows — more than the 128 partials the last block stages at
    a time, with the boundary between the two sides inside the first stage.  The bars of _assert_row; their premise, that no distance lies
    within 1e-4 relative of the threshold (so the float32 and the float64 decisions agree), is asserted here."""
    import torch
    import dqo_eval
    rng = np.random.default_rng(31)
    rec, gt = _cloud(rng, 70001, scale=(1.0, 1.0, 1.0)), _cloud(rng, 66000, scale=(1.0, 1.0, 1.0))
    d_rec64, d_gt64 = po.kdtree_distances(gt, rec)
    th = (0.03,)
    for d64 in (d_rec64, d_gt64):
        assert (np.abs(d64 - th[0]) > 1e-4 * th[0]).all() and 0 < (d64 < th[0]).sum() < d64.size
    g, r = _t(gt), _t(rec)
    a, b = dqo_eval.eval_pcd(g, r, th), dqo_eval.eval_pcd(g, r, th)
    torch.cuda.synchronize()
    _assert_row(a.cpu().numpy(), gt.shape[0], rec.shape[0], d_rec64, d_gt64, th, "unit cube")
    assert _bits(a).tobytes() == _bits(b).tobytes()


def test_ten_calls_on_one_stream_and_a_captured_graph():
    import torch
    import dqo_eval
    gt, rec, _, _ = room()
    g, r = _t(gt), _t(rec)
    table = torch.zeros((10, 32), dtype=torch.float32, device="cuda")
    for k in range(10):  # (the module's workspace, shared: the ticket words come back zero)
        dqo_eval.eval_pcd(g, r, THRES, out=table, row=k)
    torch.cuda.synchronize()
    t = _bits(table)
    assert all(t[k].tobytes() == t[0].tobytes() for k in range(10)) and np.isfinite(table[0, :10].cpu().numpy()).all()
    out = torch.zeros((1, 32), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dqo_eval.eval_pcd(g, r, THRES, out=out, row=0)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(out)[0].tobytes() == t[0].tobytes()


def test_evaluate_geometry_equals_eval_pcd_on_the_alive_rows():
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    scene = scenes.frustum_cloud(17, 1700, cam)
    fm = FusedMapper(scene, mapping.make_settings(cam, dev), dev).reserve(300)
    fm.alive[5:1700:9] = 0  # (rows a maintain() would have deleted; the 300 spare rows are parked far away)
    alive = fm.alive.bool()
    assert fm.P == 2000 and int(alive.sum().item()) == 1700 - len(range(5, 1700, 9))
    rng = np.random.default_rng(12)
    gt = _t((np.asarray(scene["xyz"], np.float32)[::2] + rng.normal(0, 0.02, (850, 3))).astype(np.float32))
    got = fm.evaluate_geometry(gt, THRES)
    want = dqo_eval.eval_pcd(gt, fm.xyz.detach()[alive].contiguous(), THRES)
    a, b = dqo_eval.nearest(gt, fm.xyz.detach(), ref_keep=fm.alive, want_idx=False)[0], dqo_eval.nearest(gt, fm.xyz.detach()[alive].contiguous())[0]
    torch.cuda.synchronize()
    assert _bits(a).tobytes() == _bits(b).tobytes()
    g, w = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
    print("evaluate_geometry", g[:10], "eval_pcd on the alive rows", w[:10])
    assert np.isfinite(g[:10]).all() and np.isnan(g[10:]).all() and g[3] == 2 and 0 < g[7] < 100
    assert (np.abs(g[:10] - w[:10]) <= REL_BAR * np.abs(w[:10])).all()  # (the same counts and distances; the sums in another block order)
    n_rec, n_gt = int(alive.sum().item()), 850
    for s, n in ((4, n_rec), (5, n_gt), (7, n_rec), (8, n_gt)):
        assert round(g[s] * n / 100) == round(w[s] * n / 100) and abs(g[s] * n / 100 - round(g[s] * n / 100)) < 1e-3
    table = torch.zeros((2, 32), dtype=torch.float32, device=dev)
    assert fm.evaluate_geometry(gt, THRES, out=table, row=1).data_ptr() == table[1].data_ptr()
    torch.cuda.synchronize()
    assert _bits(table[1]).tobytes() == _bits(got).tobytes() and not table[0].any()


def test_cpu_tensors_raise():
    import torch
    import dqo_eval
    z = torch.zeros(5, 3)
    for call in (lambda: dqo_eval.eval_pcd(z, z), lambda: dqo_eval.nearest(z, z), lambda: dqo_eval.eval_pcd(z.cuda(), z),
                 lambda: dqo_eval.nearest(z.cuda(), z.cuda(), ref_keep=torch.ones(5, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
