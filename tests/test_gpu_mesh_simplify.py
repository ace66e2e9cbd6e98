"""dqo_mesh_simplify (csrc/map_meshops.hip) on the GPU, bit for bit against tests/mesh_simplify_oracle.py: vertices, colours, faces and
the eight header words, on every mesh and cell size of tests/test_mesh_simplify.py; the chain extract -> components -> simplify ->
smooth -> normals (also replayed from a captured graph) and FusedMapper.make_simplified_mesh against the sequence by
hand.  The meshes reach the device as in tests/test_gpu_mesh_ops.py: buffers larger than the counts, garbage behind them."""
import functools

import numpy as np
import pytest

import mesh_ops_oracle as M
import mesh_simplify_oracle as S
import test_gpu_mesh_ops as G
from test_mesh_simplify import CASES, IDS, L, ORIGIN, mesh_of

pytestmark = pytest.mark.gpu

GUARD, GF, GI = 64, 12345.5, -77


@functools.lru_cache(maxsize=None)
def _want(index, colors=True):
    name, kw = CASES[index]
    m = mesh_of(name)
    return S.simplify(m["vertices"], m["colors"] if colors else None, m["faces"], **kw)


def _assert_simplified(out, want, what):
    import torch
    torch.cuda.synchronize()
    assert out["header"].cpu().numpy().tolist() == want["header"].tolist(), what
    nv, nf = int(want["header"][0]), int(want["header"][1])
    G._same(out["vertices"][:nv], want["vertices"], what + " vertices")
    if want["colors"] is not None:
        G._same(out["colors"][:nv], want["colors"], what + " colors")
    G._same(out["faces"][:nf], want["faces"], what + " faces")


def _guarded(cv, cf):
    """An out mesh inside larger buffers: (out dict, the three whole buffers)."""
    import torch
    dev = G._dev()
    bv = torch.full((cv * 3 + GUARD,), GF, device=dev)
    bc = torch.full((cv * 3 + GUARD,), GF, device=dev)
    bf = torch.full((cf * 3 + GUARD,), GI, dtype=torch.int32, device=dev)
    return dict(vertices=bv[:cv * 3].view(cv, 3), colors=bc[:cv * 3].view(cv, 3), faces=bf[:cf * 3].view(cf, 3)), (bv, bc, bf)


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_simplify_equals_the_oracle(index):
    import dqo_eval
    name, kw = CASES[index]
    m = mesh_of(name)
    V, F = len(m["vertices"]), len(m["faces"])
    want = _want(index)
    mesh = G._upload(m)
    out, (bv, bc, bf) = _guarded(V + G.PAD_V, F + G.PAD_F)
    got = dqo_eval.mesh_simplify(mesh, out=out, **kw)
    assert got is out and out["header_names"] == dqo_eval.MESH_SIMPLIFY_HEADER
    _assert_simplified(out, want, IDS[index])
    # the rows behind the written counts, and what lies behind the buffers, keep their bits; so does the input
    nv, nf = int(want["header"][0]), int(want["header"][1])
    assert (bv[3 * nv:] == GF).all() and (bc[3 * nv:] == GF).all() and (bf[3 * nf:] == GI).all(), IDS[index]
    G._tail_untouched(mesh, V, F, IDS[index])
    assert mesh["vertices"][:V].cpu().numpy().tobytes() == m["vertices"].tobytes() and np.array_equal(mesh["faces"][:F].cpu().numpy(), m["faces"])
    assert mesh["header"].cpu().numpy().tolist()[:2] == [V, F]
    c = dqo_eval.mesh_counts(out)
    assert tuple(c) == dqo_eval.MESH_SIMPLIFY_HEADER and list(c.values()) == want["header"].tolist()
    # a second run, into the module's own buffers: the same bits — neither the tables' races nor the fill's leave a trace
    again = dqo_eval.mesh_simplify(mesh, **kw)
    assert again is not out and again["vertices"].data_ptr() != out["vertices"].data_ptr()
    _assert_simplified(again, want, IDS[index] + " again")


def test_simplify_without_counts_and_without_colours():
    """counts NULL: the capacities are the counts; no colours: none are written."""
    import dqo_eval
    index = IDS.index("archipelago-%.4g" % (2 * L))
    name, kw = CASES[index]
    out = dqo_eval.mesh_simplify(G._upload(mesh_of(name), pad=False, colors=False), **kw)
    assert "colors" not in out
    _assert_simplified(out, _want(index, colors=False), "exact buffers")


def test_simplify_with_the_callers_out_and_workspace():
    import torch
    import _dqo_native as N
    import dqo_eval
    dev = G._dev()
    index = len(CASES) - 1  # cluster_extras: every tier of the member lists' sort
    name, kw = CASES[index]
    m = mesh_of(name)
    V, F = len(m["vertices"]), len(m["faces"])
    mesh = G._upload(m)
    cv, cf = V + G.PAD_V, F + G.PAD_F
    need = N.lib().dqo_mesh_simplify_workspace_bytes(cv, cf)
    ws = torch.zeros((need + GUARD,), dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    # an out mesh LARGER than the input, with a header of its own
    out = dict(vertices=torch.full((cv + 5, 3), GF, device=dev), colors=torch.full((cv + 5, 3), GF, device=dev),
               faces=torch.full((cf + 9, 3), GI, dtype=torch.int32, device=dev), header=torch.full((8,), GI, dtype=torch.int32, device=dev))
    for turn in range(2):  # the workspace comes back ready for the next call
        got = dqo_eval.mesh_simplify(mesh, out=out, workspace_buffer=ws[:need], **kw)
        assert got is out
        _assert_simplified(out, _want(index), f"own workspace, turn {turn}")
        assert (ws[need:] == 0xA5).all()
    nv, nf = int(_want(index)["header"][0]), int(_want(index)["header"][1])
    assert (out["vertices"][nv:] == GF).all() and (out["faces"][nf:] == GI).all()
    # the mesh's own header as the out header would be cleared before its counts are read: refused, as is a short workspace
    own = dict(vertices=torch.empty_like(mesh["vertices"]), colors=torch.empty_like(mesh["colors"]), faces=torch.empty_like(mesh["faces"]),
               header=mesh["header"])
    with pytest.raises(RuntimeError, match="header must not be the input's counts"):
        dqo_eval.mesh_simplify(mesh, out=own, **kw)
    with pytest.raises(RuntimeError, match="workspace too small"):
        dqo_eval.mesh_simplify(mesh, workspace_buffer=ws[:need - 256], **kw)
    assert mesh["header"].cpu().numpy().tolist()[:2] == [V, F]


# ---- the chain on the device --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _chain():
    """The oracles' chain behind test_gpu_mesh_ops's components of the sphere with a floater: simplify at 2 L, ten smoothing steps, normals."""
    origin, length, tsdf, both, weight, color, raw, comp, _, _, _ = G._chain()
    simp = S.simplify(comp["vertices"], comp["colors"], comp["faces"], 2 * float(length), tuple(float(o) for o in origin))
    p, c = M.smooth(simp["vertices"], simp["colors"], simp["faces"], 10, lam=0.5)
    return simp, p, c, M.normals(p, simp["faces"])


def _run_chain(vol, cap_v, cap_f):
    import dqo_eval
    mesh = dqo_eval.mesh_components(vol.extract(cap_v, cap_f), largest_only=True)
    mesh = dqo_eval.mesh_simplify(mesh, 2 * vol.voxel_length, origin=vol.origin)
    dqo_eval.mesh_smooth(mesh, 10, lam=0.5)
    return dqo_eval.mesh_normals(mesh)


def _assert_chain(mesh):
    import torch
    simp, p, c, n = _chain()
    torch.cuda.synchronize()
    h = mesh["header"].cpu().numpy().tolist()
    assert h == simp["header"].tolist() and h[:3] == [238, 474, 238] and h[6] == 5786  # (the sphere at 2 L)
    G._same(mesh["vertices"][:h[0]], p, "chain positions")
    G._same(mesh["colors"][:h[0]], c, "chain colours")
    G._same(mesh["faces"][:h[1]], simp["faces"], "chain faces")
    G._same(mesh["normals"][:h[0]], n, "chain normals")


def test_the_chain_with_simplify_on_the_device_and_replayed_from_a_graph():
    import torch
    import dqo_eval
    dev = G._dev()
    origin, length, tsdf, both, weight, color, raw, comp, _, _, _ = G._chain()
    cap_v, cap_f = len(raw["vertices"]) + 100, len(raw["faces"]) + 100
    vol = dqo_eval.TsdfVolume(origin, float(length), (24, 24, 24), 0.15, dev)
    G._load(vol, both, weight, color)
    _assert_chain(_run_chain(vol, cap_v, cap_f))
    # captured with an EMPTY volume (no surface: nothing to cluster), replayed with the sphere and its floater in it
    G._load(vol, np.ones_like(tsdf), weight, color)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mesh = _run_chain(vol, cap_v, cap_f)
    g.replay()
    torch.cuda.synchronize()
    assert mesh["header"].cpu().numpy().tolist() == [0] * 8
    G._load(vol, both, weight, color)
    g.replay()
    _assert_chain(mesh)


# ---- FusedMapper.make_simplified_mesh -----------------------------------------------------------------------------------------------------
def test_make_simplified_mesh_equals_the_sequence_by_hand():
    """On the small scene of test_gpu_mesh_ops.py's make_clean_mesh test."""
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = G._dev()
    cams = [scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]), (11.0, -6.0, [0.15, -0.05, 0.0]))]
    scene_ = scenes.frustum_cloud(17, 8000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    fm = FusedMapper(scene_, settings[0], dev)
    box = dict(origin=(-1.5, -1.5, 0.2), voxel_length=0.0625, dims=(48, 47, 50), sdf_trunc=0.25, device=dev)
    frames = [None, settings[1], settings[2]]
    CV, CF = 200000, 400000
    kw = dict(depth_trunc=4.0, min_component_faces=20, smooth_iter=3, smooth_lambda=0.5, smooth_mu=-0.53)
    VOX = 2 * 0.0625
    vol = dqo_eval.TsdfVolume(**box)
    mesh = fm.make_simplified_mesh(frames, vol, CV, CF, VOX, **kw)
    cnt = dqo_eval.mesh_counts(mesh)
    assert tuple(cnt) == dqo_eval.MESH_SIMPLIFY_HEADER
    raw = vol.counts()
    assert raw["vertices_dropped"] == 0 and raw["faces_dropped"] == 0 and cnt["faces_bad_index"] == 0 and cnt["vertices_outside"] == 0
    assert 50 < cnt["faces"] < raw["faces"] // 3 and cnt["faces_collapsed"] > cnt["faces"] and 20 < cnt["vertices"] < raw["vertices"] // 3
    got = {k: mesh[k][:cnt["vertices" if k != "faces" else "faces"]].clone() for k in ("vertices", "colors", "faces", "normals")}
    # by hand, in buffers of its own
    hand_vol = dqo_eval.TsdfVolume(**box)
    fm.make_mesh(frames, hand_vol, depth_trunc=4.0)
    own = lambda: dict(vertices=torch.empty((CV, 3), device=dev), colors=torch.empty((CV, 3), device=dev),
                       faces=torch.empty((CF, 3), dtype=torch.int32, device=dev))
    comp = dqo_eval.mesh_components(hand_vol.extract(CV, CF), min_faces=20, out=own())
    hand = dqo_eval.mesh_simplify(comp, 0.125, origin=(-1.5, -1.5, 0.2), out=own())
    dqo_eval.mesh_smooth(hand, 3, lam=0.5, mu=-0.53, scope="all")
    dqo_eval.mesh_normals(hand, out=torch.empty((CV, 3), device=dev))
    torch.cuda.synchronize()
    assert dqo_eval.mesh_counts(hand) == cnt
    for k, t in got.items():
        assert torch.equal(G._as_int(t), G._as_int(hand[k][:len(t)])), k
    # simplify_origin moves the grid: another mesh
    moved = dqo_eval.mesh_counts(fm.make_simplified_mesh(frames, vol, CV, CF, VOX, simplify_origin=(-1.5 - 0.0625, -1.5, 0.2), **kw))
    assert moved["clusters"] != cnt["clusters"] or moved["faces"] != cnt["faces"]
    # a second call: no allocation, no host read, the same bits
    vol.clear()
    fm.make_simplified_mesh(frames, vol, CV, CF, VOX, **kw)
    vol.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = fm.make_simplified_mesh(frames, vol, CV, CF, simplify_voxel=VOX, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert dqo_eval.mesh_counts(again) == cnt
    for k, t in got.items():
        assert torch.equal(G._as_int(t), G._as_int(again[k][:len(t)])), k


def test_a_sharded_mapper_refuses_make_simplified_mesh():
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = G._dev()
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    fm = FusedMapper(scenes.frustum_cloud(17, 8000, cam), mapping.make_settings(cam, dev), dev, attach_count_reducer=lambda n: n)
    vol = dqo_eval.TsdfVolume((-1.0, -1.0, 0.2), 0.25, (8, 8, 8), 0.5, dev)
    with pytest.raises(NotImplementedError, match="sharded"):
        fm.make_simplified_mesh([None], vol, 1000, 1000, 0.5)
