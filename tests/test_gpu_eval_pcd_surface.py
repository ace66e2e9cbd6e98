"""GPU: eval_pcd's row from exact point-to-surface distances (dqo_eval.eval_pcd_surface, dqo_eval_pcd_surface — csrc/map_eval.hip) and the
mesh chain that ends in it (dqo_eval.eval_mesh_surface, FusedMapper.evaluate_geometry_mesh_surface), on a small room: 3 072 and 2 028
faces, 20 000 points a side.

Bars.  The row against the float64 reduction (tests/pcd_oracle.py, eval_pcd_oracle) of the oracle's OWN float32 columns —
tests/mesh_dist_oracle.py's nearest_oracle for a side with a mesh, nn1_oracle for a side without: counts exactly (no distance of the
room lies within 1e-4 relative of a threshold: tests/test_mesh_dist_oracle.py asserts that premise), the other slots within the REL_BAR
of tests/test_gpu_eval_pcd.py — of its derivation only the two float32 roundings and the sum order remain here, the columns being
bit for bit the oracle's.  eval_mesh_surface: byte for byte the chain done by hand; eval_mesh: byte for byte the sampled chain, as
before."""
import numpy as np
import pytest

import mesh_cull_oracle as C
import mesh_dist_oracle as M
import pcd_oracle as po
import test_gpu_eval_pcd as TP
import test_gpu_mesh_eval as TM
from test_mesh_dist_oracle import THRES, XFORM, room

pytestmark = pytest.mark.gpu

_t = TP._t


def _mesh(vf):
    return dict(vertices=_t(vf[0], np.float32), faces=_t(vf[1], np.int32))


def _d(col):
    return np.sqrt(col.astype(np.float64))


def test_the_three_forms_on_the_room():
    import torch
    import dqo_eval
    gt, rec, gp, rp, to_gt, to_rec = room()
    g, r, gm, rm = _t(gp), _t(rp), _mesh(gt), _mesh(rec)
    pts_rec, pts_gt = po.nn1_oracle(rp, gp)[0], po.nn1_oracle(gp, rp)[0]  # the columns of a side without a mesh
    n = 20000
    both = dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES)
    again = dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES)
    table = torch.full((3, 32), 7.0, device="cuda")
    placed = dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES, out=table, row=1)
    torch.cuda.synchronize()
    assert both.dtype == torch.float32 and tuple(both.shape) == (32,) and placed.data_ptr() == table[1].data_ptr() and (table[[0, 2]] == 7.0).all()
    TP._assert_row(both.cpu().numpy(), n, n, _d(to_gt[0]), _d(to_rec[0]), THRES, "both meshes")
    assert TP._bits(both).tobytes() == TP._bits(again).tobytes() == TP._bits(placed).tobytes()
    TP._assert_row(dqo_eval.eval_pcd_surface(g, r, gt_mesh=gm, dist_thres=THRES).cpu().numpy(), n, n, _d(to_gt[0]), _d(pts_gt), THRES, "gt mesh")
    TP._assert_row(dqo_eval.eval_pcd_surface(g, r, rec_mesh=rm, dist_thres=THRES).cpu().numpy(), n, n, _d(pts_rec), _d(to_rec[0]), THRES, "rec mesh")
    # neither mesh: eval_pcd's row, byte for byte
    assert TP._bits(dqo_eval.eval_pcd_surface(g, r, dist_thres=THRES)).tobytes() == TP._bits(dqo_eval.eval_pcd(g, r, THRES)).tobytes()
    # the surface form is free of the sampled form's floor: accuracy against the gt mesh is below the sampled accuracy by about 2.7 cm
    sampled = dqo_eval.eval_pcd(g, r, THRES).cpu().numpy()
    assert 1.5 < sampled[0] - both.cpu().numpy()[0] < 3.5, (sampled[0], both.cpu().numpy()[0])


def test_rec_xform_moves_the_points_and_the_mesh():
    import dqo_eval
    gt, rec, gp, rp, _, _ = room()
    R3, t3 = XFORM[:, :3].astype(np.float64), XFORM[:, 3].astype(np.float64)
    stored_p = ((rp.astype(np.float64) - t3) @ R3).astype(np.float32)  # (R orthonormal: its inverse is its transpose)
    stored_v = ((rec[0].astype(np.float64) - t3) @ R3).astype(np.float32)
    to_gt = M.nearest_oracle(stored_p, gt + (None,), xforms=(XFORM, None))[0]
    to_rec = M.nearest_oracle(gp, (stored_v, rec[1], None), xforms=(None, XFORM))[0]
    for col in (to_gt, to_rec):  # the premise of the exact counts, for these columns
        for th in THRES:
            assert (np.abs(_d(col) - th) > 1e-6 * th).all()
    got = dqo_eval.eval_pcd_surface(_t(gp), _t(stored_p), _mesh(gt), _mesh((stored_v, rec[1])), THRES, transform=XFORM)
    TP._assert_row(got.cpu().numpy(), 20000, 20000, _d(to_gt), _d(to_rec), THRES, "moved")


def test_masks_nan_rows_and_a_mesh_without_a_valid_face():
    import dqo_eval
    gt, rec, gp, rp, to_gt, to_rec = room()
    g, r, gm, rm = _t(gp), _t(rp), _mesh(gt), _mesh(rec)
    rng = np.random.default_rng(11)
    gk, rk = rng.uniform(size=20000) < 0.5, rng.uniform(size=20000) < 0.5
    got = dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES, gt_keep=_t(gk), rec_keep=_t(rk)).cpu().numpy()
    TP._assert_row(got, int(gk.sum()), int(rk.sum()), _d(to_gt[0][rk]), _d(to_rec[0][gk]), THRES, "masked")  # (a mesh has no mask: the columns' rows)
    # eval_pcd's rule: a side without a kept point gives a row of NaN
    zero = _t(np.zeros(20000, np.uint8))
    for kw in (dict(gt_keep=zero), dict(rec_keep=zero)):
        assert np.isnan(dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES, **kw).cpu().numpy()).all(), list(kw)
    assert np.isnan(dqo_eval.eval_pcd_surface(g, _t(np.zeros((0, 3), np.float32)), gm, rm, THRES).cpu().numpy()).all()
    # a mesh without a valid face: its column is FLT_MAX — 100 sqrt(FLT_MAX) cm, no row under a threshold, F1 = 0 (R is not 0)
    empty = dict(gm, header=_t([gt[0].shape[0], 0, 0, 0, 0, 0, 0, 0], np.int32))
    row = dqo_eval.eval_pcd_surface(g, r, empty, rm, THRES).cpu().numpy()
    big = np.float32(100.0 * np.sqrt(np.float64(po.FLT_MAX)))
    assert row[0] == big and row[3] == 2 and row[4] == 0 and row[7] == 0 and row[5] > 0 and row[6] == 0 and row[9] == 0
    assert row[2] == np.float32(np.sqrt(np.float64(po.FLT_MAX)) + _d(to_rec[0]).mean()) and abs(row[1] - 100 * _d(to_rec[0]).mean()) <= TP.REL_BAR * row[1]


def test_ten_calls_on_one_stream_and_a_captured_graph():
    import torch
    import dqo_eval
    gt, rec, gp, rp, _, _ = room()
    g, r, gm, rm = _t(gp), _t(rp), _mesh(gt), _mesh(rec)
    table = torch.zeros((10, 32), dtype=torch.float32, device="cuda")
    for k in range(10):  # (the module's workspace, shared: the ticket words come back zero)
        dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES, out=table, row=k)
    torch.cuda.synchronize()
    t = TP._bits(table)
    assert all(t[k].tobytes() == t[0].tobytes() for k in range(10)) and np.isfinite(table[0, :10].cpu().numpy()).all()
    out = torch.zeros((1, 32), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dqo_eval.eval_pcd_surface(g, r, gm, rm, THRES, out=out, row=0)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert TP._bits(out)[0].tobytes() == t[0].tobytes()


@pytest.mark.parametrize("culled", [False, True])
def test_eval_mesh_surface_equals_the_chain_by_hand_and_eval_mesh_is_the_old_chain(culled):
    import torch
    import dqo_eval
    s = C.scene()
    n, seed = 4099, 21
    rv, rc, rf = TM._rec_of(s)
    rec, gt = TM._upload(rv, rc, rf), TM._upload(s["vertices"], None, s["faces"])
    views = None
    if culled:
        kw, dep = TM._views([0, 1, 2])
        views = dict(kw, depth=dep, eps=float(C.EPS))
    got = dqo_eval.eval_mesh_surface(rec, gt, n, seed=seed, dist_thres=THRES, views=views).clone()
    old = dqo_eval.eval_mesh(rec, gt, n, seed=seed, dist_thres=THRES, views=views).clone()
    # by hand: cull into buffers of the test's own, sample by the device counts, compare
    meshes, sets = [], []
    for m, sd in ((gt, seed), (rec, seed + 1)):
        if culled:
            cv, cf = m["vertices"].shape[0], m["faces"].shape[0]
            out = dict(vertices=torch.empty((cv, 3), device="cuda"), faces=torch.empty((cf, 3), dtype=torch.int32, device="cuda"))
            if "colors" in m:
                out["colors"] = torch.empty((cv, 3), device="cuda")
            m = dqo_eval.mesh_cull(m, out=out, **views)
        meshes.append(m)
        sets.append(dqo_eval.sample_surface_counted(m, n, seed=sd))
    hand = dqo_eval.eval_pcd_surface(sets[0]["points"], sets[1]["points"], meshes[0], meshes[1], THRES, gt_keep=sets[0]["keep"],
                                     rec_keep=sets[1]["keep"])
    hand_old = dqo_eval.eval_pcd(sets[0]["points"], sets[1]["points"], THRES, gt_keep=sets[0]["keep"], rec_keep=sets[1]["keep"])
    torch.cuda.synchronize()
    assert TP._bits(got).tobytes() == TP._bits(hand).tobytes(), (got.cpu().numpy()[:10], hand.cpu().numpy()[:10])
    assert TP._bits(old).tobytes() == TP._bits(hand_old).tobytes()
    g, o = got.cpu().numpy(), old.cpu().numpy()
    print("surface", g[:10], "samples", o[:10])
    assert np.isfinite(g[:10]).all() and g[0] < o[0] and g[1] < o[1]  # the floor is gone from accuracy and completion
    # against the oracle on the very meshes and points of the chain
    c = [dqo_eval.mesh_counts(m) if "header" in m else None for m in meshes]
    host = [(m["vertices"].cpu().numpy(), m["faces"].cpu().numpy(), None if k is None else np.int32([k["vertices"], k["faces"]]))
            for m, k in zip(meshes, c)]
    gp, rp = sets[0]["points"].cpu().numpy(), sets[1]["points"].cpu().numpy()
    to_gt, to_rec = M.nearest_oracle(rp, host[0])[0], M.nearest_oracle(gp, host[1])[0]
    for col in (to_gt, to_rec):
        for th in THRES:
            assert (np.abs(_d(col) - th) > 1e-6 * th).all(), th
    TP._assert_row(g, n, n, _d(to_gt), _d(to_rec), THRES, f"eval_mesh_surface culled {culled}")


def test_evaluate_geometry_mesh_surface_is_exact_towards_the_mesh():
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    gt, rec, gp, rp, _, _ = room()
    dev = torch.device("cuda")
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    mapper = FusedMapper(scenes.frustum_cloud(17, 1700, cam), mapping.make_settings(cam, dev), dev).reserve(300)
    mapper.alive[5:1700:9] = 0  # (rows a maintain() would have deleted; the 300 spare rows are parked far away)
    gv, gf = _t(gt[0]), _t(gt[1])
    got = mapper.evaluate_geometry_mesh_surface(gv, gf, 5000, seed=3, dist_thres=THRES)
    pts = dqo_eval.sample_surface(gv, gf, 5000, seed=3)
    hand = dqo_eval.eval_pcd_surface(pts["points"], mapper.xyz.detach(), dict(vertices=gv, faces=gf), None, THRES, gt_keep=pts["keep"],
                                     rec_keep=mapper.alive)
    assert TP._bits(got).tobytes() == TP._bits(hand).tobytes()
    old = mapper.evaluate_geometry_mesh(gv, gf, 5000, seed=3, dist_thres=THRES)
    assert TP._bits(old).tobytes() == TP._bits(dqo_eval.eval_pcd(pts["points"], mapper.xyz.detach(), THRES, gt_keep=pts["keep"],
                                                                   rec_keep=mapper.alive)).tobytes()
    g, o = got.cpu().numpy(), old.cpu().numpy()
    assert g[1] == o[1] and g[0] <= o[0]  # completion is the sampled form's; a point is never nearer to a sample of the surface than to the surface


def test_evaluate_mesh_surface_equals_eval_mesh_surface_with_the_views_gathered_by_hand():
    """FusedMapper.evaluate_mesh_surface under both visibility rules against dqo_eval.eval_mesh_surface on views formed by hand (the
    renders of _maintain_render, as tests/test_gpu_mesh_eval.py does for evaluate_mesh), without frames, its two refusals, and a sharded
    mapper: refused for its render only."""
    import torch
    import dqo_eval
    import test_gpu_mesh_sample as TS
    import test_gpu_tsdf as TT
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene_, cams, settings = TT._map_scene()
    fm = FusedMapper(scene_, settings[0], dev)
    vol = dqo_eval.TsdfVolume(origin=(-1.5, -1.5, 0.2), voxel_length=0.0625, dims=(48, 47, 50), sdf_trunc=0.25, device=dev)
    frames = [None, settings[1], settings[2]]
    mesh = fm.make_mesh(frames, vol, depth_trunc=4.0).extract(400000, 800000)
    gv, gf = (_t(a) for a in TS.box_mesh(*TS.BOX))
    gt = dict(vertices=gv, faces=gf)
    n, seed, Wd, Hd = 4099, 5, 160, 120
    kw = dict(sample_nums=n, seed=seed, dist_thres=THRES)
    with pytest.raises(ValueError, match="visibility is 'vertices' or 'faces'"):
        fm.evaluate_mesh_surface(mesh, gv, gf, frames=frames, visibility="pixels", **kw)
    with pytest.raises(ValueError, match="needs cameras"):
        fm.evaluate_mesh_surface(mesh, gv, gf, visibility="faces", **kw)
    depth = torch.stack([fm._maintain_render(st).out[1].reshape(Hd, Wd).clone() for st in settings])
    w2c = torch.stack([st.viewmatrix.reshape(4, 4).t().contiguous().reshape(16) for st in settings])
    st = settings[0]
    K = (Wd / (2.0 * float(st.tanfovx)), Hd / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
    base = dict(w2c=w2c, K=K, W=Wd, H=Hd, depth=depth, eps=0.05, depth_trunc=4.0)
    rows = {}
    for visibility, rule, arg in (("vertices", dict(min_corners=2), dict(min_corners=2)), ("faces", dict(min_pixels=2, visibility="faces"), dict(min_pixels=2))):
        got = fm.evaluate_mesh_surface(mesh, gv, gf, frames=frames, depths="render", eps=0.05, depth_trunc=4.0, visibility=visibility, **arg, **kw).clone()
        hand = dqo_eval.eval_mesh_surface(mesh, gt, n, seed=seed, dist_thres=THRES, views=dict(base, **rule)).clone()
        sampled = dqo_eval.eval_mesh(mesh, gt, n, seed=seed, dist_thres=THRES, views=dict(base, **rule)).clone()
        own = fm.evaluate_mesh_surface(mesh, gv, gf, frames=frames, depths=depth, eps=0.05, depth_trunc=4.0, visibility=visibility, **arg, **kw).clone()
        torch.cuda.synchronize()
        assert TP._bits(got).tobytes() == TP._bits(hand).tobytes() == TP._bits(own).tobytes(), visibility
        g, o = got.cpu().numpy(), sampled.cpu().numpy()
        assert np.isfinite(g[:3]).all() and g[3] == 2 and g[0] < o[0] and g[1] < o[1], visibility  # (the same samples, nearer to a face than to a sample)
        rows[visibility] = TP._bits(got).tobytes()
    assert not fm.maintain_overflowed()
    # without frames: no culling, eval_mesh_surface as it is
    table = torch.zeros((2, 32), device=dev)
    whole = fm.evaluate_mesh_surface(mesh, gv, gf, out=table, row=1, **kw)
    whole_hand = dqo_eval.eval_mesh_surface(mesh, gt, n, seed=seed, dist_thres=THRES).clone()
    torch.cuda.synchronize()
    assert whole.data_ptr() == table[1].data_ptr() and TP._bits(whole).tobytes() == TP._bits(whole_hand).tobytes() and (table[0] == 0).all()
    # a sharded mapper is refused for its render only
    shard = FusedMapper(scene_, settings[0], dev, attach_count_reducer=lambda k: k)
    for visibility in ("vertices", "faces"):
        with pytest.raises(NotImplementedError, match="sharded"):
            shard.evaluate_mesh_surface(mesh, gv, gf, frames=frames, depths="render", visibility=visibility, **kw)
    sharded = shard.evaluate_mesh_surface(mesh, gv, gf, frames=frames, depths=depth, eps=0.05, depth_trunc=4.0, min_corners=2, **kw)
    torch.cuda.synchronize()
    assert TP._bits(sharded).tobytes() == rows["vertices"]
