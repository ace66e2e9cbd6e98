"""Mesh depth and Depth L1 on the GPU (csrc/map_meshrender.hip; csrc/map_eval.hip's dqo_eval_depth_l1): dqo_eval.mesh_render_depth bit
for bit against tests/mesh_render_oracle.py — depth, face_index, the eight header words — on a mesh that takes every branch;
dqo_eval.depth_l1 bit for bit against tests/depth_l1_oracle.py; dqo_eval.eval_mesh_depth and FusedMapper.evaluate_mesh_depth against
the chain done by hand; the render and the comparison replayed from a captured graph with changed counts and matrices.

Bars.  Everything the render writes: bit for bit (float32 and float64 statements without contraction, an integer min whose result does
not depend on the order).  The Depth L1 table: bit for bit (double sums in the oracle's order); its root is the one operation that
could differ, by the last bit of a double before the rounding to float32."""
import numpy as np
import pytest

import depth_l1_oracle as D
import mesh_render_oracle as R
import test_gpu_mesh_ops as G

pytestmark = pytest.mark.gpu

GUARD, GF, GI = 64, 12345.5, -77


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.asarray(a, dtype), device="cuda")


def _upload(vertices, faces, behind=None, counts=None):
    """A mesh dict on the device with its counts in a device header.  Behind the counts: NaN positions, and `behind`, faces that LOOK
    alive (valid indices, a triangle in front of everything) — a kernel that read a row behind the counts would show it."""
    import torch
    V, F = len(vertices), len(faces)
    v = torch.full((V + G.PAD_V, 3), float("nan"), device="cuda")
    v[:V] = _t(vertices)
    tail = np.zeros((0, 3), np.int32) if behind is None else np.asarray(behind, np.int32)
    f = torch.full((F + len(tail) + G.PAD_F, 3), 1 << 30, dtype=torch.int32, device="cuda")
    f[:F] = _t(faces)
    if len(tail):
        f[F:F + len(tail)] = _t(tail)
    header = torch.tensor(list(counts if counts is not None else (V, F)) + [0] * 6, dtype=torch.int32, device="cuda")
    return dict(vertices=v, faces=f, header=header)


def _views(s, sel=None):
    w2c = s["w2c"] if sel is None else s["w2c"][sel]
    return dict(w2c=_t(w2c.reshape(-1, 16)), K=s["K"], W=s["W"], H=s["H"])


def _assert_render(got, want, what):
    import torch
    torch.cuda.synchronize()
    assert got["header"].cpu().numpy().tolist() == want["header"].tolist(), (what, got["header"].cpu().numpy().tolist(), want["header"].tolist())
    G._same(got["depth"], want["depth"], what + " depth")
    if got.get("face_index") is not None:
        G._same(got["face_index"], want["face_index"], what + " face_index")


# ---- the render against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [(1, 0, 1), None])
def test_mixed_mesh_equals_the_oracle_bit_for_bit(keep):
    """A welded grid, image-sized triangles (the whole-wave path), degenerate, bad-index and near-crossing faces; three views, one
    switched off; the counts on the device with live-looking faces behind them; guard words behind the outputs; twice."""
    import torch
    import dqo_eval
    s = R.mixed_scene()
    v, f = s["vertices"], s["faces"]
    want = R.render(v, f, s["w2c"], s["K"], s["W"], s["H"], view_keep=keep, near=s["near"])
    h = dict(zip(R.HEADER, want["header"].tolist()))
    assert h["pairs_cooperative"] > 0 and h["pairs_near_dropped"] > 0 and h["pairs_degenerate"] > 0 and h["faces_bad_index"] == 3
    V0 = 21 * 17  # (the grid's vertices come first)
    behind = [[V0 + 6, V0 + 7, 356], [V0 + 6, 0, V0 + 7], [0, 336, V0 + 6]]  # valid indices, triangles in front of part of the grid
    assert (R.render(v, np.concatenate([f, behind]), s["w2c"], s["K"], s["W"], s["H"], keep, s["near"])["face_index"] != want["face_index"]).any()
    mesh = _upload(v, f, behind=behind)
    n, H, W = 3, s["H"], s["W"]
    bd = torch.full((n * H * W + GUARD,), GF, device="cuda")
    bi = torch.full((n * H * W + GUARD,), GI, dtype=torch.int32, device="cuda")
    out = dict(depth=bd[:n * H * W].view(n, H, W), face_index=bi[:n * H * W].view(n, H, W))
    kw = dict(_views(s), view_keep=_t(keep, np.uint8), near=s["near"])
    for turn in range(2):
        got = dqo_eval.mesh_render_depth(mesh, want_face_index=True, out=out, **kw)
        assert got is out and out["header_names"] == dqo_eval.MESH_RENDER_HEADER
        _assert_render(got, want, f"mixed mesh keep {keep}, turn {turn}")
        assert (bd[n * H * W:] == GF).all() and (bi[n * H * W:] == GI).all()
    assert torch.isnan(mesh["vertices"][len(v):]).all() and mesh["faces"][len(f):len(f) + 3].cpu().numpy().tolist() == behind
    assert (mesh["faces"][len(f) + 3:] == 1 << 30).all() and mesh["header"].cpu().numpy().tolist()[:2] == [len(v), len(f)]
    counts = dqo_eval.mesh_counts(got)
    assert tuple(counts) == dqo_eval.MESH_RENDER_HEADER and list(counts.values()) == want["header"].tolist()
    if keep is not None:  # the image of the unused view is written as no hit
        assert not got["depth"][1].any() and (got["face_index"][1] == -1).all()
    # a depth truncation, on the module's own buffers
    cut = dqo_eval.mesh_render_depth(mesh, want_face_index=True, depth_trunc=2.4, **kw)
    assert cut is not out
    _assert_render(cut, R.render(v, f, s["w2c"], s["K"], s["W"], s["H"], view_keep=keep, near=s["near"], depth_trunc=2.4), "truncated")


@pytest.mark.parametrize("W, H", [(1, 1), (64, 1), (1, 64)])
def test_smallest_shapes(W, H):
    """One face, one view; exact buffers without counts."""
    import dqo_eval
    v = np.array([[-1.0, -1.2, 2.0], [1.5, -0.8, 2.5], [0.2, 1.4, 3.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    K = (20.0, 21.0, (W - 1) / 2, (H - 1) / 2)
    want = R.render(v, f, np.eye(4, dtype=np.float32)[None], K, W, H)
    assert want["header"].tolist()[:6] == [1, 0, 1, 0, 0, 0] and want["header"][6] > 0
    got = dqo_eval.mesh_render_depth(dict(vertices=_t(v), faces=_t(f)), _t(np.eye(4, dtype=np.float32).reshape(1, 16)), K, W, H, want_face_index=True)
    _assert_render(got, want, f"{W} x {H}")
    # the counts say the mesh is empty: nothing is hit, nothing is counted
    none = dqo_eval.mesh_render_depth(_upload(v, f, counts=(3, 0)), _t(np.eye(4, dtype=np.float32).reshape(1, 16)), K, W, H, want_face_index=True)
    _assert_render(none, R.render(v, f[:0], np.eye(4, dtype=np.float32)[None], K, W, H), f"{W} x {H}, no face")


def test_257_faces_33_views_and_only_the_last_pair_is_visible():
    """More than one block of 256 faces, more than one chunk of 32 views; faces 0 - 255 lie far to the side of every camera, views
    0 - 31 look away from face 256."""
    import dqo_eval
    W, H, K = 40, 30, (35.0, 35.0, 19.5, 14.5)
    rng = np.random.default_rng(3)
    aside = (np.array([500.0, 0.0, 5.0]) + rng.uniform(-0.2, 0.2, size=(256 * 3, 3))).astype(np.float32)
    tri = np.array([[-0.7, -0.6, 2.0], [0.9, -0.5, 2.2], [0.1, 0.8, 2.6]], np.float32)
    v = np.concatenate([aside, tri])
    f = np.arange(257 * 3, dtype=np.int32).reshape(257, 3)
    away = R.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    w2c = np.concatenate([np.repeat(away[None], 32, 0), np.eye(4, dtype=np.float32)[None]])
    want = R.render(v, f, w2c, K, W, H)
    assert want["header"].tolist()[:6] == [33, 0, 1, 0, 0, 1] and set(np.unique(want["face_index"])) == {-1, 256}
    assert not want["depth"][:32].any() and (want["depth"][32] > 0).sum() == want["header"][6] > 100
    mesh, kw = _upload(v, f), dict(w2c=_t(w2c.reshape(-1, 16)), K=K, W=W, H=H)
    _assert_render(dqo_eval.mesh_render_depth(mesh, want_face_index=True, **kw), want, "257 x 33")
    keep = np.zeros(33, np.uint8)
    keep[[3, 32]] = 1
    _assert_render(dqo_eval.mesh_render_depth(mesh, want_face_index=True, view_keep=_t(keep), **kw),
                   R.render(v, f, w2c, K, W, H, view_keep=keep), "257 x 33, two used")


def test_without_face_index_and_with_the_callers_workspace():
    import torch
    import _dqo_native as N
    import dqo_eval
    s = R.mixed_scene()
    want = R.render(s["vertices"], s["faces"], s["w2c"], s["K"], s["W"], s["H"], near=s["near"])
    mesh = _upload(s["vertices"], s["faces"])
    need = N.lib().dqo_mesh_render_depth_workspace_bytes(3, s["W"], s["H"])
    ws = torch.zeros((need + GUARD,), dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5
    for turn in range(2):  # the workspace comes back ready for the next call
        got = dqo_eval.mesh_render_depth(mesh, near=s["near"], workspace_buffer=ws[:need], **_views(s))
        assert got["face_index"] is None
        _assert_render(got, want, f"caller's workspace, turn {turn}")
        assert (ws[need:] == 0xA5).all()
    with pytest.raises(RuntimeError, match="workspace too small"):
        dqo_eval.mesh_render_depth(mesh, workspace_buffer=ws[:need - 256], **_views(s))
    with pytest.raises(RuntimeError, match="bad near"):
        dqo_eval.mesh_render_depth(mesh, near=-1.0, **_views(s))
    with pytest.raises(RuntimeError, match="header must not be the mesh's counts"):
        dqo_eval.mesh_render_depth(mesh, out=dict(header=mesh["header"]), **_views(s))


# ---- depth_l1 -----------------------------------------------------------------------------------------------------------------------------
def _assert_table(got, want, what):
    import torch
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.float32
    same = (g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want))
    assert same.all(), (what, g[~same.all(1)], want[~same.all(1)])


def test_depth_l1_equals_its_oracle_bit_for_bit_on_hand_made_stacks():
    """Views of more than one block (41 x 37 = 1517 pixels), an all-miss view on each side, a view empty on both, a view switched off, a
    truncation that removes part of the truth."""
    import torch
    import dqo_eval
    rng = np.random.default_rng(9)
    n, H, W = 6, 37, 41
    a = rng.uniform(0.5, 4.0, size=(n, H, W)).astype(np.float32)
    b = (a + rng.normal(0.0, 0.05, size=a.shape)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = 0.0
    b[rng.random(b.shape) < 0.25] = 0.0
    a[1], b[2] = 0.0, 0.0
    a[3], b[3] = 0.0, 0.0
    keep = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    for kw, okw in ((dict(), dict()), (dict(view_keep=_t(keep)), dict(view_keep=keep)),
                    (dict(view_keep=_t(keep), depth_trunc=3.0), dict(view_keep=keep, depth_trunc=3.0)),
                    (dict(view_keep=_t(np.zeros(n, np.uint8))), dict(view_keep=np.zeros(n, np.uint8)))):
        want = D.depth_l1(a, b, **okw)
        table = torch.full((n + 1, 8), 7.0, device="cuda")
        got = dqo_eval.depth_l1(_t(a), _t(b), out=table, **kw)
        assert got is table
        _assert_table(got, want, str(okw))
        _assert_table(dqo_eval.depth_l1(_t(a), _t(b), **kw), want, str(okw) + " again")  # (the workspace came back ready)
    d = dqo_eval.depth_l1_dict(dqo_eval.depth_l1(_t(a), _t(b), view_keep=_t(keep)))
    assert d["views"][4] is None and d["views"][1]["both"] == 0 and d["views"][1]["only_b"] > 0 and d["mean"]["both"] > 1000
    assert sum(d["views"][0][k] for k in ("both", "only_a", "only_b", "neither")) == H * W
    with pytest.raises(RuntimeError, match="depth_rec must be"):
        dqo_eval.depth_l1(_t(a), _t(b[:, :-1]))


def test_depth_l1_of_the_rendered_pair_and_eval_mesh_depth_equals_the_chain_by_hand():
    import torch
    import dqo_eval
    s = R.mixed_scene()
    gv, gf = R.grid_mesh(20, 16, (-0.8, -0.6, 2.0), (0.08, 0.0, 0.012), (0.0, 0.075, 0.02))
    rv = (gv.astype(np.float64) + 0.02 * np.stack([np.sin(5 * gv[:, 1]), np.cos(4 * gv[:, 0]), np.sin(3 * gv[:, 0] + 1)], 1)).astype(np.float32)
    rf = gf[:-40]
    keep = np.array([1, 0, 1], np.uint8)
    views = dict(_views(s), view_keep=_t(keep), near=s["near"], depth_trunc=2.6)
    gt, rec = _upload(gv, gf), _upload(rv, rf)
    da = dqo_eval.mesh_render_depth(gt, out={}, **views)["depth"]
    db = dqo_eval.mesh_render_depth(rec, out={}, **views)["depth"]
    hand = dqo_eval.depth_l1(da, db, view_keep=views["view_keep"], depth_trunc=2.6)
    wa = R.render(gv, gf, s["w2c"], s["K"], s["W"], s["H"], keep, s["near"], 2.6)["depth"]
    wb = R.render(rv, rf, s["w2c"], s["K"], s["W"], s["H"], keep, s["near"], 2.6)["depth"]
    G._same(da, wa, "gt depth")
    G._same(db, wb, "rec depth")
    want = D.depth_l1(wa, wb, view_keep=keep, depth_trunc=2.6)
    _assert_table(hand, want, "rendered pair")
    assert want[3, 3] > 500 and 0 < want[3, 0] < 0.05 and want[3, 4] > 0  # (both hit widely, centimetres apart, the missing faces show)
    table = torch.zeros((4, 8), device="cuda")
    got = dqo_eval.eval_mesh_depth(rec, gt, dict(views, eps=0.03, min_corners=3, depth=None), out=table)  # (eval_mesh's dict, its cull keys ignored)
    assert got is table
    _assert_table(got, want, "eval_mesh_depth")
    # a mesh against itself
    same = dqo_eval.eval_mesh_depth(gt, gt, views)
    torch.cuda.synchronize()
    t = same.cpu().numpy()
    assert t[3, 0] == 0 and t[3, 2] == 0 and t[3, 7] == 0 and t[3, 4] == 0 and t[3, 5] == 0 and t[3, 3] == want[3, 3] + want[3, 4]
    with pytest.raises(RuntimeError, match="mesh_render_depth's own"):
        dqo_eval.eval_mesh_depth(rec, gt, dict(views, want_face_index=True))
    # the rendered stack is a depth for the cull's occlusion test
    culled = dqo_eval.mesh_counts(dqo_eval.mesh_cull(gt, depth=da, eps=0.01, **{k: x for k, x in views.items() if k != "depth_trunc"}))
    assert 0 < culled["faces"] <= len(gf) and culled["views_used"] == 2


# ---- FusedMapper.evaluate_mesh_depth ------------------------------------------------------------------------------------------------------
def test_evaluate_mesh_depth_equals_the_chain_with_the_views_gathered_by_hand():
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
    gv, gf = R.grid_mesh(12, 10, (-1.2, -0.9, 2.4), (0.2, 0.0, 0.03), (0.0, 0.18, -0.02))  # in camera 0's space, then to the world
    gv = (gv.astype(np.float64) @ c2w0[:3, :3].T + c2w0[:3, 3]).astype(np.float32)
    rv = (gv + np.float32(0.03) * np.sin(7 * gv[:, ::-1])).astype(np.float32)
    mesh = _upload(rv, gf[:-30])
    frames = [None, settings[1], settings[2]]
    st = settings[0]
    K = (Wd / (2.0 * float(st.tanfovx)), Hd / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
    with pytest.raises(ValueError, match="another image size or other intrinsics"):
        fm.evaluate_mesh_depth(mesh, _t(gv), _t(gf), [None, settings[1]._replace(image_width=Wd + 16)])
    with pytest.raises(ValueError, match="a depth needs cameras"):
        fm.evaluate_mesh_depth(mesh, _t(gv), _t(gf), None)
    assert fm._mesh_eval_views == {}
    table = torch.zeros((4, 8), device=dev)
    got = fm.evaluate_mesh_depth(mesh, _t(gv), _t(gf), frames, depth_trunc=4.0, out=table)
    assert got is table
    views = dict(w2c=w2c, K=K, W=Wd, H=Hd, depth_trunc=4.0)
    hand = dqo_eval.eval_mesh_depth(mesh, dict(vertices=_t(gv), faces=_t(gf)), views)
    torch.cuda.synchronize()
    _assert_table(got, hand.cpu().numpy(), "a mesh")
    t = got.cpu().numpy()
    assert t[3, 3] > 1000 and 0 < t[3, 0] < 0.1 and (t[:3, 3:7].sum(1) == Wd * Hd).all()
    # mesh=None: the map's own render per frame
    own = fm.evaluate_mesh_depth(None, _t(gv), _t(gf), frames, depth_trunc=4.0).clone()
    depth = torch.stack([fm._maintain_render(s_).out[1].reshape(Hd, Wd).clone() for s_ in settings])
    truth = dqo_eval.mesh_render_depth(dict(vertices=_t(gv), faces=_t(gf)), w2c, K, Wd, Hd, depth_trunc=4.0, out={})["depth"]
    by_hand = dqo_eval.depth_l1(truth, depth, depth_trunc=4.0)
    torch.cuda.synchronize()
    assert not fm.maintain_overflowed()
    _assert_table(own, by_hand.cpu().numpy(), "mesh=None")
    assert (own[:3, 3:7].sum(1) == Wd * Hd).all()
    shard = FusedMapper(scene_, settings[0], dev, attach_count_reducer=lambda k: k)
    with pytest.raises(NotImplementedError, match="sharded"):
        shard.evaluate_mesh_depth(None, _t(gv), _t(gf), frames)
    _assert_table(shard.evaluate_mesh_depth(mesh, _t(gv), _t(gf), frames, depth_trunc=4.0), hand.cpu().numpy(), "a sharded mapper, a mesh")


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------
def test_one_capture_replayed_with_changed_counts_and_matrices_equals_the_eager_calls():
    import torch
    import dqo_eval
    s = R.mixed_scene()
    v, f = s["vertices"], s["faces"]
    gv, gf = R.grid_mesh(20, 16, (-0.8, -0.6, 2.0), (0.08, 0.0, 0.012), (0.0, 0.075, 0.02))
    mesh, gt = _upload(v, f), _upload(gv, gf)
    kw = dict(_views(s), near=s["near"])
    outs = [{}, {}]

    def chain(o):
        a = dqo_eval.mesh_render_depth(gt, out=o[0], **kw)
        b = dqo_eval.mesh_render_depth(mesh, want_face_index=True, out=o[1], **kw)
        return dict(a=a["depth"], b=b["depth"], face_index=b["face_index"], header=b["header"], gt_header=a["header"], table=dqo_eval.depth_l1(a["depth"], b["depth"]))

    def snapshot(d):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().tobytes() for k, t in d.items()}

    chain(outs)  # the warm-up: the module's workspaces exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branch)
        out = chain(outs)
    V, F = len(v), len(f)
    for counts, sel in (((V, F), (0, 1, 2)), ((V, F // 2), (2, 0, 1)), ((V - 9, F), (1, 1, 0)), ((V, 0), (0, 1, 2))):
        mesh["header"][:2] = torch.tensor(counts, dtype=torch.int32, device="cuda")
        kw["w2c"].copy_(_t(s["w2c"][list(sel)].reshape(-1, 16)))
        graph.replay()
        got = snapshot(out)
        want = snapshot(chain([{}, {}]))
        for k in want:
            assert got[k] == want[k], (counts, sel, k)
        oracle = R.render(v[:counts[0]], f[:counts[1]], s["w2c"][list(sel)], s["K"], s["W"], s["H"], near=s["near"])
        assert got["b"] == oracle["depth"].tobytes() and got["header"] == oracle["header"].tobytes(), (counts, sel)
