"""Near-plane clipping and the face cull on the GPU (csrc/map_meshrender.hip's dqo_mesh_render_depth_clip, csrc/map_meshcull.hip's
dqo_mesh_cull_faces) against tests/mesh_clip_oracle.py: depth, face_index, the header, face_pixels and the out mesh bit for bit (float32
and float64 statements without contraction, integer min and integer adds whose results do not depend on the order; where two faces give
one depth the key's lower face id wins in the kernel and in the oracle alike); dqo_eval.eval_mesh's visibility="faces",
eval_mesh_depth's clip_near=True and the two FusedMapper methods against the chain done by hand; one captured graph replayed."""
import numpy as np
import pytest

import mesh_clip_oracle as C
import mesh_render_oracle as R
import test_gpu_mesh_ops as G
import test_gpu_mesh_render as RT
import test_mesh_clip_oracle as TO

pytestmark = pytest.mark.gpu

_t, _upload, _assert_render = RT._t, RT._upload, RT._assert_render
WALL = dict(K=C.WALL_K, W=C.WALL_W, H=C.WALL_H)


def _w2c(m):
    return _t(np.asarray(m, np.float32).reshape(-1, 16))


def _out_mesh(mesh):
    """An out mesh of the caller's own for mesh_cull_visible: the input's capacities."""
    import torch
    return dict(vertices=torch.empty_like(mesh["vertices"]), faces=torch.empty_like(mesh["faces"]))


# ---- the render ---------------------------------------------------------------------------------------------------------------------------
def test_the_wall_is_an_empty_image_without_clipping_and_the_oracles_image_with_it():
    import dqo_eval
    views = C.wall_views()
    mesh = _upload(C.WALL_VERTICES, C.WALL_FACES)
    plain = dqo_eval.mesh_render_depth(mesh, _w2c(views), want_face_index=True, out={}, **WALL)
    _assert_render(plain, R.render(C.WALL_VERTICES, C.WALL_FACES, views, **WALL), "the wall, dropped")
    assert not plain["depth"].any() and plain["header"].cpu().tolist() == [3, 0, 0, 6, 0, 0, 0, 0]
    want = C.render(C.WALL_VERTICES, C.WALL_FACES, views, **WALL)
    assert want["header"][3] == 6 and want["header"][6] > 1500 and want["header"][5] >= 3
    got = dqo_eval.mesh_render_depth_clip(mesh, _w2c(views), want_face_index=True, out={}, **WALL)
    assert got["header_names"] == dqo_eval.MESH_RENDER_CLIP_HEADER
    _assert_render(got, want, "the wall, clipped")
    assert dqo_eval.mesh_counts(got)["pairs_near_clipped"] == 6
    # seen frontally nothing crosses: the plain entry's bytes
    front = R.look_at((2.0, 1.0, -3.0), (2.0, 1.0, 1.0))[None]
    a = dqo_eval.mesh_render_depth(mesh, _w2c(front), want_face_index=True, out={}, **WALL)
    b = dqo_eval.mesh_render_depth_clip(mesh, _w2c(front), want_face_index=True, out={}, **WALL)
    _assert_render(b, R.render(C.WALL_VERTICES, C.WALL_FACES, front, **WALL), "the wall, frontal")
    for k in ("depth", "face_index", "header"):
        assert G._bits(a[k]).tobytes() == G._bits(b[k]).tobytes(), k


@pytest.mark.parametrize("keep", [(1, 0, 1), None])
def test_mixed_mesh_equals_the_oracle_bit_for_bit(keep):
    import torch
    import dqo_eval
    s = R.mixed_scene()
    v, f = s["vertices"], s["faces"]
    want = C.render(v, f, s["w2c"], s["K"], s["W"], s["H"], view_keep=keep, near=s["near"])
    h = dict(zip(C.HEADER, want["header"].tolist()))
    assert h["pairs_cooperative"] > 0 and h["pairs_near_clipped"] > 0 and h["pairs_degenerate"] > 0 and h["faces_bad_index"] == 3
    assert np.isin(want["face_index"], np.nonzero(want["crossing"].any(0))[0]).any()  # a crossing face wins pixels
    V0 = 21 * 17
    behind = [[V0 + 6, V0 + 7, 356], [V0 + 6, 0, V0 + 7], [0, 336, V0 + 6]]
    mesh = _upload(v, f, behind=behind)
    n, H, W = 3, s["H"], s["W"]
    bd = torch.full((n * H * W + RT.GUARD,), RT.GF, device="cuda")
    bi = torch.full((n * H * W + RT.GUARD,), RT.GI, dtype=torch.int32, device="cuda")
    out = dict(depth=bd[:n * H * W].view(n, H, W), face_index=bi[:n * H * W].view(n, H, W))
    kw = dict(RT._views(s), view_keep=_t(keep, np.uint8), near=s["near"])
    for turn in range(2):
        got = dqo_eval.mesh_render_depth_clip(mesh, want_face_index=True, out=out, **kw)
        assert got is out
        _assert_render(got, want, f"mixed mesh keep {keep}, turn {turn}")
        assert (bd[n * H * W:] == RT.GF).all() and (bi[n * H * W:] == RT.GI).all()
    if keep is not None:
        assert not got["depth"][1].any() and (got["face_index"][1] == -1).all()
    cut = dqo_eval.mesh_render_depth_clip(mesh, want_face_index=True, depth_trunc=2.4, **kw)
    _assert_render(cut, C.render(v, f, s["w2c"], s["K"], s["W"], s["H"], view_keep=keep, near=s["near"], depth_trunc=2.4), "truncated")


@pytest.mark.parametrize("near", [0.0, 0.05])
def test_cube_from_inside(near):
    import dqo_eval
    v, f = R.cube_mesh()
    views = TO.inside_views()
    want = C.render(v, f, views, TO.K, TO.W, TO.H, near=near)
    assert (want["face_index"] >= 0).all() and want["header"][3] >= 8 * len(views)
    got = dqo_eval.mesh_render_depth_clip(_upload(v, f), _w2c(views), TO.K, TO.W, TO.H, near=near, want_face_index=True, out={})
    _assert_render(got, want, f"cube from inside, near {near}")


@pytest.mark.parametrize("W, H", [(1, 1), (64, 1), (1, 64)])
def test_smallest_shapes(W, H):
    """One face that crosses the near plane, one view; exact buffers without counts."""
    import dqo_eval
    v = np.array([[-1.0, -1.2, 2.0], [1.5, -0.8, 2.5], [0.2, 1.4, -1.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    K = (20.0, 21.0, (W - 1) / 2, (H - 1) / 2)
    eye = np.eye(4, dtype=np.float32)
    for near in (0.0, 0.25):
        want = C.render(v, f, eye[None], K, W, H, near=near)
        assert want["header"].tolist()[:5] == [1, 0, 1, 1, 0] and want["header"][6] > 0
        got = dqo_eval.mesh_render_depth_clip(dict(vertices=_t(v), faces=_t(f)), _w2c(eye), K, W, H, near=near, want_face_index=True)
        _assert_render(got, want, f"{W} x {H}, near {near}")
    none = dqo_eval.mesh_render_depth_clip(_upload(v, f, counts=(3, 0)), _w2c(eye), K, W, H, want_face_index=True)
    _assert_render(none, C.render(v, f[:0], eye[None], K, W, H), f"{W} x {H}, no face")


def test_257_faces_33_views_and_only_the_last_pair_crosses_and_is_visible():
    import dqo_eval
    W, H, K = 40, 30, (35.0, 35.0, 19.5, 14.5)
    rng = np.random.default_rng(3)
    aside = (np.array([500.0, 0.0, 5.0]) + rng.uniform(-0.2, 0.2, size=(256 * 3, 3))).astype(np.float32)
    tri = np.array([[-0.7, -0.6, 2.0], [0.9, -0.5, 2.2], [0.1, 0.8, -0.6]], np.float32)  # its third corner lies behind the last camera
    v = np.concatenate([aside, tri])
    f = np.arange(257 * 3, dtype=np.int32).reshape(257, 3)
    away = R.look_at((0.0, 0.0, -50.0), (0.0, 0.0, -51.0))  # everything lies behind it
    w2c = np.concatenate([np.repeat(away[None], 32, 0), np.eye(4, dtype=np.float32)[None]])
    want = C.render(v, f, w2c, K, W, H)
    assert want["header"].tolist()[:6] == [33, 0, 1, 1, 0, 1] and set(np.unique(want["face_index"])) == {-1, 256}
    assert not want["depth"][:32].any() and (want["depth"][32] > 0).sum() == want["header"][6] > 100
    mesh, kw = _upload(v, f), dict(w2c=_w2c(w2c), K=K, W=W, H=H)
    _assert_render(dqo_eval.mesh_render_depth_clip(mesh, want_face_index=True, **kw), want, "257 x 33")
    keep = np.zeros(33, np.uint8)
    keep[[3, 32]] = 1
    _assert_render(dqo_eval.mesh_render_depth_clip(mesh, want_face_index=True, view_keep=_t(keep), **kw),
                   C.render(v, f, w2c, K, W, H, view_keep=keep), "257 x 33, two used")


def test_a_wall_sized_crossing_pair_by_the_wave_and_a_small_one_by_its_lane():
    import dqo_eval
    W, H, K, near = 80, 72, (60.0, 60.0, 39.5, 35.5), 0.5
    v = np.array([[-30.0, -30.0, 3.0], [30.0, -20.0, 3.0], [0.0, 40.0, -2.0],            # crosses, and covers most of the image
                  [0.02, 0.02, 0.6], [0.05, 0.02, 0.6], [0.03, 0.04, 0.4]], np.float32)  # crosses within a few pixels
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    eye = np.eye(4, dtype=np.float32)
    want = C.render(v, f, eye[None], K, W, H, near=near)
    assert want["header"].tolist()[:6] == [1, 0, 2, 2, 0, 1]  # both cross, both have a box, one box is above SMALL_MAX
    big, small = (want["face_index"] == 0).sum(), (want["face_index"] == 1).sum()
    assert big > 64 * 64 and 0 < small <= R.SMALL_MAX
    got = dqo_eval.mesh_render_depth_clip(_upload(v, f), _w2c(eye), K, W, H, near=near, want_face_index=True, out={})
    _assert_render(got, want, "wave and lane")
    assert dqo_eval.mesh_counts(got)["pairs_cooperative"] == 1


# ---- the face cull ------------------------------------------------------------------------------------------------------------------------
def _assert_faces_culled(out, want, F_in, what):
    import torch
    torch.cuda.synchronize()
    assert out["header"].cpu().numpy().tolist() == want["header"].tolist(), (what, out["header"].cpu().numpy().tolist(), want["header"].tolist())
    nv, nf = int(want["header"][0]), int(want["header"][1])
    G._same(out["vertices"][:nv], want["vertices"], what + " vertices")
    if want["colors"] is not None:
        G._same(out["colors"][:nv], want["colors"], what + " colors")
    G._same(out["faces"][:nf], want["faces"], what + " faces")
    G._same(out["face_pixels"][:F_in], want["face_pixels"], what + " face_pixels")


def test_mesh_cull_visible_on_the_wall():
    import torch
    import dqo_eval
    views = C.wall_views()
    kw = dict(w2c=_w2c(views), **WALL)
    hidden = np.array([[-5.0, -5.0, 3.0], [5.0, -5.0, 3.0], [5.0, 5.0, 3.0], [-5.0, 5.0, 3.0]], np.float32)  # a quad behind the wall
    v = np.concatenate([hidden, C.WALL_VERTICES])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [4, 9, 5]], np.int32)  # (and a face with a bad index)
    cols = np.linspace(0.0, 1.0, 24, dtype=np.float32).reshape(8, 3)
    wall = _upload(C.WALL_VERTICES, C.WALL_FACES)
    # the vertex rule: no face of the wall has its three corners inside an image
    assert dqo_eval.mesh_counts(dqo_eval.mesh_cull(wall, **kw))["faces"] == 0
    r = C.render(C.WALL_VERTICES, C.WALL_FACES, views, **WALL)
    want = C.cull_faces(C.WALL_VERTICES, None, C.WALL_FACES, r["face_index"], r["depth"])
    got = dqo_eval.mesh_cull_visible(wall, want_pixels=True, **kw)
    _assert_faces_culled(got, want, 2, "the wall")
    _assert_render(got["render"], r, "the wall's render")
    counts = dqo_eval.mesh_counts(got)
    assert counts["faces"] == 2 and tuple(counts) == dqo_eval.MESH_CULL_FACES_HEADER
    assert int(got["face_pixels"][:2].sum()) == counts["pixels_counted"] == int(got["render"]["header"][6]) == int(r["header"][6])
    assert dqo_eval.mesh_cull_visible(wall, **kw)["face_pixels"] is None
    # with the quad behind it: exactly the wall stays, renumbered; colours bit for bit
    mesh = _upload(v, f)
    mesh["colors"] = torch.full((len(v) + G.PAD_V, 3), float("nan"), device="cuda")
    mesh["colors"][:len(v)] = _t(cols)
    r2 = C.render(v, f, views, **WALL)
    for keep, min_pixels in ((None, 1), ((1, 0, 1), 1), (None, 600), ((0, 0, 0), 1)):
        want = C.cull_faces(v, cols, f, r2["face_index"], r2["depth"], view_keep=keep, min_pixels=min_pixels)
        got = dqo_eval.mesh_cull_visible(mesh, view_keep=_t(keep, np.uint8), min_pixels=min_pixels, want_pixels=True, **kw)
        _assert_faces_culled(got, want, len(f), f"wall and hidden quad, keep {keep}, min_pixels {min_pixels}")
    want = C.cull_faces(v, cols, f, r2["face_index"], r2["depth"])
    assert want["header"].tolist()[:7] == [4, 2, 2, 3, 1, 2, 4] and want["faces"].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert want["vertices"].tobytes() == C.WALL_VERTICES.tobytes()
    assert C.cull_faces(v, cols, f, r2["face_index"], r2["depth"], min_pixels=600)["header"][1] < 2  # (min_pixels bites)
    # a sensor depth nearer than the wall minus eps hides it; one as far as the wall keeps it
    for shift, faces in ((-0.1, 0), (0.0, 2), (0.02, 2)):
        sensor = np.where(r2["depth"] > 0, r2["depth"] + np.float32(shift), np.float32(0)).astype(np.float32)
        want = C.cull_faces(v, cols, f, r2["face_index"], r2["depth"], depth=sensor, eps=0.03, depth_trunc=50.0)
        assert want["header"][1] == faces
        got = dqo_eval.mesh_cull_visible(mesh, depth=_t(sensor), eps=0.03, depth_trunc=50.0, want_pixels=True, **kw)
        _assert_faces_culled(got, want, len(f), f"sensor depth shifted by {shift}")
    assert torch.isnan(mesh["vertices"][len(v):]).all() and (mesh["faces"][len(f):] == 1 << 30).all()


def test_face_cull_takes_any_face_index_and_counts_runs_across_rounds():
    """dqo_mesh_cull_faces alone on hand-made renders: ids out of range are never an index; a view of more than a batch's 1024 pixels,
    a wave's 4096 and a block's 16384; runs that end inside a round, at a round's end, and that go on through rounds, batches and waves."""
    import torch
    import _dqo_native as N
    rng = np.random.default_rng(11)
    nv, H, W = 3, 131, 137  # 17947 pixels a view: two blocks, the second partly filled
    V_, F_ = 40, 23
    v = rng.normal(size=(V_, 3)).astype(np.float32)
    f = rng.integers(0, V_, size=(F_, 3)).astype(np.int32)
    f[5] = [1, V_, 2]
    fi = np.repeat(rng.integers(-1, F_, size=(nv, 400)), 50, axis=1)[:, :H * W].astype(np.int32)  # runs of 50 straddle the rounds of 64
    fi[1, :12000] = 3  # one face wins most of a view: whole rounds, batches and waves of one id
    fi[1, 12000:12064] = 5  # (a bad face's id: counted by the pixels launch, put back to 0 behind it)
    odd = fi[2, ::97]
    fi[2, ::97] = np.resize(np.array([F_, -5, 1 << 30, -(1 << 31), F_ + 1], np.int64), len(odd)).astype(np.int32)
    fi = fi.reshape(nv, H, W)
    rd = rng.uniform(1.0, 3.0, size=(nv, H, W)).astype(np.float32)
    sensor = (rd + rng.normal(0.0, 0.04, size=rd.shape)).astype(np.float32)
    sensor[rng.random(rd.shape) < 0.1] = 0.0
    mesh = _upload(v, f)
    cv, cf = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    ws = torch.zeros((N.lib().dqo_mesh_cull_workspace_bytes(cv, cf),), dtype=torch.uint8, device="cuda")
    d_fi, d_rd = _t(fi), _t(rd)
    for depth, keep, min_pixels in ((None, None, 1), (sensor, (1, 0, 1), 1000), (sensor, None, 1)):
        want = C.cull_faces(v, None, f, fi, rd, depth=depth, view_keep=keep, eps=0.03, depth_trunc=2.8, min_pixels=min_pixels)
        ov, of = torch.full((cv, 3), 9.0, device="cuda"), torch.full((cf, 3), -9, dtype=torch.int32, device="cuda")
        px, hd = torch.full((cf,), -9, dtype=torch.int32, device="cuda"), torch.full((8,), -9, dtype=torch.int32, device="cuda")
        d_keep, d_depth = _t(keep, np.uint8), _t(depth)
        N.check(N.lib().dqo_mesh_cull_faces(mesh["vertices"].data_ptr(), None, mesh["faces"].data_ptr(), mesh["header"].data_ptr(), cv, cf, nv,
                                            N.ptr(d_keep), W, H, d_fi.data_ptr(), d_rd.data_ptr(), N.ptr(d_depth), 0.03, 2.8, min_pixels,
                                            ov.data_ptr(), None, of.data_ptr(), cv, cf, px.data_ptr(), hd.data_ptr(), ws.data_ptr(), ws.numel(),
                                            N.current_stream()))
        _assert_faces_culled(dict(vertices=ov, faces=of, header=hd, face_pixels=px), want, F_, f"hand-made render, {keep}, {min_pixels}")
        assert (px[F_:] == -9).all() and (ov[int(want["header"][0]):] == 9.0).all() and want["face_pixels"][5] == 0
        assert want["header"][1] > 0 and want["face_pixels"][3] >= (12000 if depth is None else 1)


# ---- the chains ---------------------------------------------------------------------------------------------------------------------------
def _room():
    """A reconstruction-like grid in front of the wall and the wall itself as the ground truth, seen by the wall's cameras."""
    gv, gf = R.grid_mesh(14, 12, (-1.0, -2.0, 0.97), (0.45, 0.0, 0.0), (0.0, 0.4, 0.002))
    return gv, gf


def test_eval_mesh_faces_and_eval_mesh_depth_clip_near_equal_the_chain_by_hand():
    import torch
    import dqo_eval
    views = C.wall_views()
    kw = dict(w2c=_w2c(views), **WALL)
    gv, gf = _room()
    rec, gt = _upload(gv, gf), _upload(C.WALL_VERTICES, C.WALL_FACES)
    n, seed = 2049, 5
    got = dqo_eval.eval_mesh(rec, gt, n, seed=seed, dist_thres=(0.05,), views=dict(kw, visibility="faces", min_pixels=2, min_corners=3,
                                                                                  clip_near=True)).clone()
    cg = dqo_eval.mesh_cull_visible(gt, min_pixels=2, out=_out_mesh(gt), **kw)
    cr = dqo_eval.mesh_cull_visible(rec, min_pixels=2, out=_out_mesh(rec), **kw)
    a, b = dqo_eval.sample_surface_counted(cg, n, seed=seed), dqo_eval.sample_surface_counted(cr, n, seed=seed + 1)
    hand = dqo_eval.eval_pcd(a["points"], b["points"], (0.05,), None, gt_keep=a["keep"], rec_keep=b["keep"])
    torch.cuda.synchronize()
    assert G._bits(got).tobytes() == G._bits(hand).tobytes() and not np.isnan(got.cpu().numpy()[:4]).any()
    assert dqo_eval.mesh_counts(cg)["faces"] == 2 and 0 < dqo_eval.mesh_counts(cr)["faces"] < len(gf)
    # the vertex rule, the default, drops the wall: the ground truth is empty and the row is NaN
    plain = dqo_eval.eval_mesh(rec, gt, n, seed=seed, dist_thres=(0.05,), views=dict(kw, min_pixels=2))
    assert np.isnan(plain.cpu().numpy()).all()
    # Depth L1
    table = dqo_eval.eval_mesh_depth(rec, gt, dict(kw, clip_near=True, visibility="faces", min_pixels=2)).clone()
    da = dqo_eval.mesh_render_depth_clip(gt, out={}, **kw)["depth"]
    db = dqo_eval.mesh_render_depth_clip(rec, out={}, **kw)["depth"]
    hand = dqo_eval.depth_l1(da, db)
    torch.cuda.synchronize()
    RT._assert_table(table, hand.cpu().numpy(), "eval_mesh_depth, clip_near")
    G._same(da, C.render(C.WALL_VERTICES, C.WALL_FACES, views, **WALL)["depth"], "gt depth")
    G._same(db, C.render(gv, gf, views, **WALL)["depth"], "rec depth")
    t = table.cpu().numpy()
    assert t[3, 3] > 500  # pixels hit in both
    unclipped = dqo_eval.eval_mesh_depth(rec, gt, kw).cpu().numpy()  # the default: the wall is a hole
    assert unclipped[3, 3] == 0 and unclipped[3, 4] == 0


def test_the_two_mapper_methods_equal_the_chain_with_the_views_gathered_by_hand():
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    Wd, Hd = 64, 48
    cams = [scenes.Camera(Wd, Hd, 52.5, 52.5, 31.5, 23.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]), (11.0, -6.0, [0.15, -0.05, 0.0]))]
    scene_ = scenes.frustum_cloud(17, 2000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    fm = FusedMapper(scene_, settings[0], dev)
    w2c = torch.stack([st.viewmatrix.reshape(4, 4).t().contiguous().reshape(16) for st in settings])
    c2w0 = np.linalg.inv(w2c[0].reshape(4, 4).cpu().numpy().astype(np.float64))
    # a floor of two triangles under camera 0, larger than every frustum and through every near plane, then to the world
    floor = np.array([[-80.0, 0.6, -30.0], [85.0, 0.62, -35.0], [82.0, 0.58, 60.0], [-78.0, 0.61, 55.0]], np.float64)
    gv = (floor @ c2w0[:3, :3].T + c2w0[:3, 3]).astype(np.float32)
    gf = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    pv, pf = R.grid_mesh(10, 10, (-1.0, 0.57, 0.5), (0.25, 0.0, 0.0), (0.0, 0.004, 0.35))
    pv = (pv.astype(np.float64) @ c2w0[:3, :3].T + c2w0[:3, 3]).astype(np.float32)
    mesh = _upload(pv, pf)
    frames = [None, settings[1], settings[2]]
    st = settings[0]
    K = (Wd / (2.0 * float(st.tanfovx)), Hd / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
    views = dict(w2c=w2c, K=K, W=Wd, H=Hd)
    gt = dict(vertices=_t(gv), faces=_t(gf))
    with pytest.raises(ValueError, match="visibility needs cameras"):
        fm.evaluate_mesh_visible(mesh, _t(gv), _t(gf), None)
    got = fm.evaluate_mesh_depth_clipped(mesh, _t(gv), _t(gf), frames, depth_trunc=30.0).clone()
    hand = dqo_eval.eval_mesh_depth(mesh, gt, dict(views, depth_trunc=30.0, clip_near=True))
    torch.cuda.synchronize()
    RT._assert_table(got, hand.cpu().numpy(), "evaluate_mesh_depth_clipped")
    dropped = fm.evaluate_mesh_depth(mesh, _t(gv), _t(gf), frames, depth_trunc=30.0).cpu().numpy()
    assert got.cpu().numpy()[3, 3] > 100 and dropped[3, 3] == 0  # the floor is depth with the clip and a hole without
    row = fm.evaluate_mesh_visible(mesh, _t(gv), _t(gf), frames, sample_nums=1500, seed=3, dist_thres=(0.05,), min_pixels=2).clone()
    hand = dqo_eval.eval_mesh(mesh, gt, 1500, seed=3, dist_thres=(0.05,), views=dict(views, visibility="faces", min_pixels=2, eps=0.03))
    torch.cuda.synchronize()
    assert G._bits(row).tobytes() == G._bits(hand).tobytes() and not np.isnan(row.cpu().numpy()[:4]).any()
    assert np.isnan(fm.evaluate_mesh(mesh, _t(gv), _t(gf), frames, sample_nums=1500, seed=3, dist_thres=(0.05,)).cpu().numpy()).all()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------
def test_one_capture_replayed_with_changed_counts_and_matrices_equals_the_eager_calls():
    import torch
    import dqo_eval
    s = R.mixed_scene()
    v, f = s["vertices"], s["faces"]
    mesh = _upload(v, f)
    kw = dict(RT._views(s), near=s["near"])

    def chain(o):
        a = dqo_eval.mesh_render_depth_clip(mesh, want_face_index=True, out=o[0], **kw)
        c = dqo_eval.mesh_cull_visible(mesh, min_pixels=2, want_pixels=True, out=o[1], **kw)
        return dict(depth=a["depth"], face_index=a["face_index"], header=a["header"], cull_header=c["header"], faces=c["faces"],
                    vertices=c["vertices"], face_pixels=c["face_pixels"])

    def snapshot(d, counts):
        torch.cuda.synchronize()
        nv, nf = (int(x) for x in d["cull_header"][:2].cpu())
        cut = dict(faces=nf, vertices=nv, face_pixels=counts[1])  # (rows behind the counts are untouched, so not compared)
        return {k: t[:cut[k]].cpu().numpy().tobytes() if k in cut else t.cpu().numpy().tobytes() for k, t in d.items()}

    outs = [{}, _out_mesh(mesh)]
    chain(outs)  # the warm-up: the module's workspaces and render buffers exist, and this chain's own
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branch)
        out = chain(outs)
    V_, F_ = len(v), len(f)
    for counts, sel in (((V_, F_), (0, 1, 2)), ((V_, F_ // 2), (2, 0, 1)), ((V_ - 9, F_), (1, 1, 0)), ((V_, 0), (0, 1, 2))):
        mesh["header"][:2] = torch.tensor(counts, dtype=torch.int32, device="cuda")
        kw["w2c"].copy_(_t(s["w2c"][list(sel)].reshape(-1, 16)))
        graph.replay()
        got = snapshot(out, counts)
        want = snapshot(chain([{}, _out_mesh(mesh)]), counts)
        for k in want:
            assert got[k] == want[k], (counts, sel, k)
        oracle = C.render(v[:counts[0]], f[:counts[1]], s["w2c"][list(sel)], s["K"], s["W"], s["H"], near=s["near"])
        assert got["depth"] == oracle["depth"].tobytes() and got["header"] == oracle["header"].tobytes(), (counts, sel)
        culled = C.cull_faces(v[:counts[0]], None, f[:counts[1]], oracle["face_index"], oracle["depth"], min_pixels=2)
        assert got["cull_header"] == culled["header"].tobytes() and got["faces"] == culled["faces"].tobytes(), (counts, sel)
