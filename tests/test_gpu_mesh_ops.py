"""csrc/map_meshops.hip on the GPU, bit for bit against tests/mesh_ops_oracle.py: connected components and the filtered mesh, Laplacian
and Taubin smoothing, vertex normals, the chain extract -> components -> smooth -> normals (also replayed from a captured graph) and
FusedMapper.make_clean_mesh against the sequence by hand.  The meshes reach the device in buffers LARGER than their counts, the rows
behind the counts filled with NaN positions and out-of-range indices, the counts in a device header: what lies behind is neither read
nor written."""
import functools

import numpy as np
import pytest

import mesh_ops_oracle as M
import tsdf_oracle as O

pytestmark = pytest.mark.gpu

PAD_V, PAD_F = 37, 53


def _dev():
    import torch
    return torch.device("cuda")


def _upload(m, pad=True, colors=True):
    """The mesh dict on the device: capacities above the counts, garbage behind them, a device header with the counts (pad), or exact
    buffers without a header."""
    import torch
    dev = _dev()
    V, F = len(m["vertices"]), len(m["faces"])
    cv, cf = (V + PAD_V, F + PAD_F) if pad else (V, F)
    v = torch.full((cv, 3), float("nan"), device=dev)
    c = torch.full((cv, 3), float("nan"), device=dev)
    f = torch.full((cf, 3), 1 << 30, dtype=torch.int32, device=dev)
    f[F + 1::2] = -7
    v[:V] = torch.from_numpy(m["vertices"]).to(dev)
    c[:V] = torch.from_numpy(m["colors"]).to(dev)
    f[:F] = torch.from_numpy(m["faces"]).to(dev)
    d = dict(vertices=v, faces=f)
    if colors:
        d["colors"] = c
    if pad:
        d["header"] = torch.tensor([V, F, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
    return d


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same(t, want, what):
    got = t.detach().cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if got.size == 0:
        return
    if got.dtype == np.float32:
        bad = (got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(1)
    else:
        bad = (got != want).reshape(len(got), -1).any(1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:5], got[bad][:3], want[bad][:3])


def _tail_untouched(d, V, F, what):
    """The rows behind the counts still hold _upload's garbage."""
    import torch
    assert torch.isnan(d["vertices"][V:]).all() and ("colors" not in d or torch.isnan(d["colors"][V:]).all()), what
    tail = d["faces"][F:].cpu().numpy()
    assert (tail[0::2] == 1 << 30).all() and (tail[1::2] == -7).all(), what


# ---- components -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_components(min_faces, largest_only):
    a = M.archipelago()
    return M.components(a["vertices"], a["colors"], a["faces"], min_faces=min_faces, largest_only=largest_only)


def _assert_components(out, want, F_in, what):
    import torch
    torch.cuda.synchronize()
    assert out["header"].cpu().numpy().tolist() == want["header"].tolist(), what
    nv, nf = int(want["header"][0]), int(want["header"][1])
    _same(out["vertices"][:nv], want["vertices"], what + " vertices")
    if want["colors"] is not None:
        _same(out["colors"][:nv], want["colors"], what + " colors")
    _same(out["faces"][:nf], want["faces"], what + " faces")
    if "labels" in out:
        _same(out["labels"][:F_in], want["labels"], what + " labels")


@pytest.mark.parametrize("min_faces,largest_only", [(0, False), (1, False), (5, False), (8, False), (9, False), (701, False), (6260, False),
                                                    (6261, False), (0, True)])
def test_components_equal_the_oracle(min_faces, largest_only):
    import torch
    import dqo_eval
    dev = _dev()
    a = M.archipelago()
    V, F = len(a["vertices"]), len(a["faces"])
    want = _want_components(min_faces, largest_only)
    mesh = _upload(a)
    cv, cf = V + PAD_V, F + PAD_F
    # the out buffers sit inside larger ones: the rows behind the written counts, and what lies behind the buffers, keep their bits
    GUARD, gf, gi = 64, 12345.5, -77
    bv = torch.full((cv * 3 + GUARD,), gf, device=dev)
    bc = torch.full((cv * 3 + GUARD,), gf, device=dev)
    bf = torch.full((cf * 3 + GUARD,), gi, dtype=torch.int32, device=dev)
    bl = torch.full((cf + GUARD,), gi, dtype=torch.int32, device=dev)
    out = dict(vertices=bv[:cv * 3].view(cv, 3), colors=bc[:cv * 3].view(cv, 3), faces=bf[:cf * 3].view(cf, 3), labels=bl[:cf])
    got = dqo_eval.mesh_components(mesh, min_faces=min_faces, largest_only=largest_only, out=out, want_labels=True)
    assert got is out
    what = f"min_faces {min_faces} largest_only {largest_only}"
    _assert_components(out, want, F, what)
    nv, nf = int(want["header"][0]), int(want["header"][1])
    assert (bv[3 * nv:] == gf).all() and (bc[3 * nv:] == gf).all() and (bf[3 * nf:] == gi).all() and (bl[F:] == gi).all(), what
    _tail_untouched(mesh, V, F, what)
    c = dqo_eval.mesh_counts(out)
    assert tuple(c) == dqo_eval.MESHOPS_HEADER and list(c.values()) == want["header"].tolist()
    if min_faces == 6261:
        assert c["vertices"] == 0 and c["faces"] == 0 and c["components_kept"] == 0 and c["components"] == 9
    if largest_only:
        assert c["components_kept"] == 1 and c["faces"] == 6260
    # a second run, into the module's own buffers, without labels: the same bits, the header is the next operator's counts
    again = dqo_eval.mesh_components(mesh, min_faces=min_faces, largest_only=largest_only)
    assert again is not out and "labels" not in again
    _assert_components(again, want, F, what + " again")


def test_components_without_counts_and_without_colours():
    """counts NULL: the capacities are the counts; no colours: none are written."""
    import dqo_eval
    a = M.archipelago()
    want = M.components(a["vertices"], None, a["faces"], min_faces=5)
    out = dqo_eval.mesh_components(_upload(a, pad=False, colors=False), min_faces=5, want_labels=True)
    assert "colors" not in out
    _assert_components(out, want, len(a["faces"]), "exact buffers")


def test_components_tied_for_largest_are_all_kept():
    import dqo_eval
    rng = np.random.default_rng(3)
    v = rng.normal(size=(8, 3)).astype(np.float32)
    f = np.concatenate([M.TETRA, M.TETRA + 4]).astype(np.int32)
    m = dict(vertices=v, colors=rng.uniform(size=(8, 3)).astype(np.float32), faces=f)
    want = M.components(v, m["colors"], f, largest_only=True)
    assert want["header"].tolist() == [8, 8, 2, 2, 0, 4, 0, 0]
    out = dqo_eval.mesh_components(_upload(m), largest_only=True, want_labels=True)
    _assert_components(out, want, 8, "two tetrahedra")
    assert out["labels"][:8].cpu().numpy().tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    # the mesh's own header as the out header would be cleared before its counts are read: refused
    import torch
    mesh = _upload(m)
    own = dict(vertices=torch.empty_like(mesh["vertices"]), colors=torch.empty_like(mesh["colors"]), faces=torch.empty_like(mesh["faces"]),
               header=mesh["header"])
    with pytest.raises(RuntimeError, match="header must not be the input's counts"):
        dqo_eval.mesh_components(mesh, out=own)
    assert mesh["header"].cpu().numpy().tolist()[:2] == [8, 8]


# ---- smoothing --------------------------------------------------------------------------------------------------------------------------
MESHES = {"archipelago": M.archipelago, "extras": M.smoothing_extras}
SMOOTH = {"one": (1, 0.5, None, "all"), "three": (3, 0.5, None, "all"), "taubin": (2, 0.5, -0.53, "all"), "positions": (2, 0.5, None, "positions"),
          "colors": (2, 0.5, None, "colors")}


@functools.lru_cache(maxsize=None)
def _want_smooth(which, cfg):
    m = MESHES[which]()
    it, lam, mu, scope = SMOOTH[cfg]
    return M.smooth(m["vertices"], m["colors"], m["faces"], it, lam=lam, mu=mu or 0.0, scope=scope)


@pytest.mark.parametrize("cfg", list(SMOOTH))
@pytest.mark.parametrize("which", list(MESHES))
def test_smooth_equals_the_oracle(which, cfg):
    import torch
    import dqo_eval
    m = MESHES[which]()
    V, F = len(m["vertices"]), len(m["faces"])
    it, lam, mu, scope = SMOOTH[cfg]
    wp, wc = _want_smooth(which, cfg)
    assert (scope == "colors") == (wp.tobytes() == m["vertices"].tobytes()) and (scope == "positions") == (wc.tobytes() == m["colors"].tobytes())
    runs = []
    for _ in range(2):  # the same call on fresh copies: the same bits — the fill's race leaves no trace
        mesh = _upload(m)
        assert dqo_eval.mesh_smooth(mesh, it, lam=lam, mu=mu, scope=scope) is mesh
        torch.cuda.synchronize()
        _same(mesh["vertices"][:V], wp, f"{which} {cfg} positions")
        _same(mesh["colors"][:V], wc, f"{which} {cfg} colors")
        _tail_untouched(mesh, V, F, f"{which} {cfg}")
        assert np.array_equal(mesh["faces"][:F].cpu().numpy(), m["faces"])
        runs.append((_bits(mesh["vertices"][:V]).tobytes(), _bits(mesh["colors"][:V]).tobytes()))
    assert runs[0] == runs[1]
    # vertices without neighbours keep their bits
    deg = np.diff(M.neighbours(V, m["faces"])[0])
    lone = np.nonzero(deg == 0)[0]
    assert len(lone) >= 7
    assert np.array_equal(mesh["vertices"][:V].cpu().numpy()[lone].view(np.uint32), m["vertices"][lone].view(np.uint32))
    assert np.array_equal(mesh["colors"][:V].cpu().numpy()[lone].view(np.uint32), m["colors"][lone].view(np.uint32))


def test_smooth_zero_iterations_and_a_mesh_without_colours():
    import torch
    import dqo_eval
    m = M.smoothing_extras()
    V = len(m["vertices"])
    mesh = _upload(m)
    dqo_eval.mesh_smooth(mesh, 0)
    torch.cuda.synchronize()
    _same(mesh["vertices"][:V], m["vertices"], "zero iterations")
    _same(mesh["colors"][:V], m["colors"], "zero iterations")
    plain = _upload(m, pad=False, colors=False)
    dqo_eval.mesh_smooth(plain, 3)  # scope "all" of a mesh without colours: the positions
    torch.cuda.synchronize()
    _same(plain["vertices"], _want_smooth("extras", "three")[0], "no colours")
    with pytest.raises(RuntimeError, match="without colors"):
        dqo_eval.mesh_smooth(plain, 1, scope="colors")


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(MESHES))
def test_normals_equal_the_oracle(which):
    import torch
    import dqo_eval
    m = MESHES[which]()
    V, F = len(m["vertices"]), len(m["faces"])
    want = M.normals(m["vertices"], m["faces"])
    mesh = _upload(m)
    guard = torch.full((V + PAD_V + 8, 3), 777.0, device=_dev())
    assert dqo_eval.mesh_normals(mesh, out=guard[:V + PAD_V]) is mesh and mesh["normals"].data_ptr() == guard.data_ptr()
    torch.cuda.synchronize()
    _same(mesh["normals"][:V], want, which)
    assert (guard[V:] == 777.0).all()
    _tail_untouched(mesh, V, F, which)
    _same(mesh["vertices"][:V], m["vertices"], which + ": the mesh is only read")
    got = mesh["normals"][:V].cpu().numpy()
    referenced = np.zeros(V, bool)
    referenced[m["faces"][M.valid_faces(V, m["faces"])].ravel()] = True
    assert (~referenced).sum() >= 7 and (got[~referenced] == [0.0, 0.0, 1.0]).all()
    if which == "extras":
        assert (got[m["sliver"]] == [0.0, 0.0, 1.0]).all()  # only a zero-area face
    # the module's own buffer, a second time: the same bits
    dqo_eval.mesh_normals(mesh)
    torch.cuda.synchronize()
    assert mesh["normals"].data_ptr() != guard.data_ptr()
    _same(mesh["normals"][:V], want, which + " again")


# ---- the chain on the device --------------------------------------------------------------------------------------------------------------
FLOATER_C, FLOATER_R = (-0.3, -0.3, -0.3), 0.06


@functools.lru_cache(maxsize=1)
def _chain():
    """The sphere's volume, the same with a small second sphere (a floater) written into it, and the oracle's chain on the second."""
    origin, length, tsdf, weight, color = O.sphere_volume()
    _, _, small, _, _ = O.sphere_volume(r=FLOATER_R, centre=FLOATER_C)
    both = np.minimum(tsdf, small)
    raw = O.extract(both, weight, color, origin, length)
    comp = M.components(raw["vertices"], raw["colors"], raw["faces"], largest_only=True)
    p, c = M.smooth(comp["vertices"], comp["colors"], comp["faces"], 10, lam=0.5)
    n = M.normals(p, comp["faces"])
    return origin, length, tsdf, both, weight, color, raw, comp, p, c, n


def _load(vol, tsdf, weight, color):
    import torch
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    vol.color.copy_(torch.from_numpy(color))


def _run_chain(vol, cap_v, cap_f):
    import dqo_eval
    mesh = dqo_eval.mesh_components(vol.extract(cap_v, cap_f), largest_only=True)
    dqo_eval.mesh_smooth(mesh, 10, lam=0.5)
    return dqo_eval.mesh_normals(mesh)


def _assert_chain(mesh):
    import torch
    origin, length, tsdf, both, weight, color, raw, comp, p, c, n = _chain()
    torch.cuda.synchronize()
    h = mesh["header"].cpu().numpy().tolist()
    assert h == comp["header"].tolist() and h[2] == 2 and h[3] == 1 and h[0] == 3132 and h[1] == 6260 and h[7] == len(raw["faces"]) - 6260
    _same(mesh["vertices"][:h[0]], p, "chain positions")
    _same(mesh["colors"][:h[0]], c, "chain colours")
    _same(mesh["faces"][:h[1]], comp["faces"], "chain faces")
    _same(mesh["normals"][:h[0]], n, "chain normals")


def test_the_chain_on_the_device_and_replayed_from_a_graph():
    import torch
    import dqo_eval
    dev = _dev()
    origin, length, tsdf, both, weight, color, raw, comp, p, c, n = _chain()
    assert len(raw["faces"]) > 6260 and len(raw["vertices"]) > 3132  # the floater is in the raw mesh
    cap_v, cap_f = len(raw["vertices"]) + 100, len(raw["faces"]) + 100
    vol = dqo_eval.TsdfVolume(origin, float(length), (24, 24, 24), 0.15, dev)
    _load(vol, both, weight, color)
    _assert_chain(_run_chain(vol, cap_v, cap_f))
    # captured with the plain sphere in the volume (one component, nothing to remove), replayed with the floater in it
    _load(vol, tsdf, weight, color)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mesh = _run_chain(vol, cap_v, cap_f)
    g.replay()
    torch.cuda.synchronize()
    assert mesh["header"].cpu().numpy().tolist()[:4] == [3132, 6260, 1, 1]
    _load(vol, both, weight, color)
    g.replay()
    _assert_chain(mesh)


# ---- FusedMapper.make_clean_mesh ----------------------------------------------------------------------------------------------------------
def test_make_clean_mesh_equals_the_sequence_by_hand():
    """On the small scene of test_gpu_tsdf.py's make_mesh test."""
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = _dev()
    cams = [scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]), (11.0, -6.0, [0.15, -0.05, 0.0]))]
    scene_ = scenes.frustum_cloud(17, 8000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    fm = FusedMapper(scene_, settings[0], dev)
    box = dict(origin=(-1.5, -1.5, 0.2), voxel_length=0.0625, dims=(48, 47, 50), sdf_trunc=0.25, device=dev)
    frames = [None, settings[1], settings[2]]
    CV, CF = 200000, 400000
    kw = dict(depth_trunc=4.0, min_component_faces=20, smooth_iter=3, smooth_lambda=0.5, smooth_mu=-0.53)
    vol = dqo_eval.TsdfVolume(**box)
    mesh = fm.make_clean_mesh(frames, vol, CV, CF, **kw)
    cnt = dqo_eval.mesh_counts(mesh)
    raw = vol.counts()
    assert raw["vertices_dropped"] == 0 and raw["faces_dropped"] == 0 and cnt["faces_bad_index"] == 0
    assert 100 < cnt["faces"] <= raw["faces"] and cnt["faces"] + cnt["faces_removed"] == raw["faces"] and cnt["components_kept"] >= 1
    got = {k: mesh[k][:cnt["vertices" if k != "faces" else "faces"]].clone() for k in ("vertices", "colors", "faces", "normals")}
    # by hand, in buffers of its own
    hand_vol = dqo_eval.TsdfVolume(**box)
    fm.make_mesh(frames, hand_vol, depth_trunc=4.0)
    own = dict(vertices=torch.empty((CV, 3), device=dev), colors=torch.empty((CV, 3), device=dev), faces=torch.empty((CF, 3), dtype=torch.int32, device=dev))
    hand = dqo_eval.mesh_components(hand_vol.extract(CV, CF), min_faces=20, out=own)
    dqo_eval.mesh_smooth(hand, 3, lam=0.5, mu=-0.53, scope="all")
    dqo_eval.mesh_normals(hand, out=torch.empty((CV, 3), device=dev))
    torch.cuda.synchronize()
    assert dqo_eval.mesh_counts(hand) == cnt
    for k, t in got.items():
        assert torch.equal(_as_int(t), _as_int(hand[k][:len(t)])), k
    nrm = got["normals"].cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-6 and np.isfinite(got["vertices"].cpu().numpy()).all()
    # a second call: no allocation, no host read, the same bits; normals=False leaves them out
    vol.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = fm.make_clean_mesh(frames, vol, CV, CF, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert dqo_eval.mesh_counts(again) == cnt
    for k, t in got.items():
        assert torch.equal(_as_int(t), _as_int(again[k][:len(t)])), k
    assert "normals" not in fm.make_clean_mesh(frames, vol, CV, CF, normals=False, **kw)


def _as_int(t):
    import torch
    return t.contiguous().view(torch.int32)


def test_a_sharded_mapper_refuses_make_clean_mesh():
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = _dev()
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    fm = FusedMapper(scenes.frustum_cloud(17, 8000, cam), mapping.make_settings(cam, dev), dev, attach_count_reducer=lambda n: n)
    vol = dqo_eval.TsdfVolume((-1.0, -1.0, 0.2), 0.25, (8, 8, 8), 0.5, dev)
    with pytest.raises(NotImplementedError, match="sharded"):
        fm.make_clean_mesh([None], vol, 1000, 1000)
