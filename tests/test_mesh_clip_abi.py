"""CPU-side checks of the clipping render's and the face cull's entry points (dqo_mesh_render_depth_clip, csrc/map_meshrender.hip;
dqo_mesh_cull_faces, csrc/map_meshcull.hip): the two symbols are declared, exported and bound, the ABI did not move and no size query
was added, every argument error is reported before anything is launched (-1 for bad arguments, then -2 for a short workspace; no GPU
here), the launch counts are the header's words, and the Python surface is the documented one."""
import ctypes
import inspect
import os
import re

import pytest

import mesh_clip_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_render_depth_clip", "dqo_mesh_cull_faces")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch (the workspace is
# NULL wherever a call is to fail earlier, so a check that let a bad argument through would still end at the workspace check)
BIG = 1 << 44
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def _src(name):
    return open(os.path.join(ROOT, "dqo-map_amd", "csrc", name)).read()


def _entry_body(src, name):
    body = src[src.index(f"DQO_API int {name}("):]
    return body[:body.index("\n}\n")]


def test_symbols_are_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    L = native.lib()
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(L, s).argtypes
    assert L.dqo_mesh_render_depth_clip.argtypes == L.dqo_mesh_render_depth.argtypes  # the same arguments
    a = L.dqo_mesh_cull_faces.argtypes
    assert len(a) == 26 and a[13:15] == [ctypes.c_float] * 2 and a[15] is ctypes.c_int32 and a[24] is ctypes.c_size_t
    for cite in ("homogeneous rasterisation", "that test IS the clip", "P_0 . (P_1 x P_2)", "tests/mesh_clip_oracle.py", "WIN PIXELS",
                 "never used as an index", "dqo_mesh_cull_workspace_bytes(cap_vertices, cap_faces) is this entry's query too",
                 "dqo_mesh_render_depth_clip below is the entry that clips", "Not built: near-plane clipping, back-face culling",
                 "Six launches", "Three launches"):
        assert cite in hdr, cite


def test_the_abi_did_not_move_and_no_size_query_was_added(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = native.lib()
    assert lib.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    queries = set(re.findall(r"size_t (dqo_\w*_bytes\w*)\(", hdr))
    assert not [q for q in queries if "clip" in q or "cull_faces" in q]
    assert not [n for n in native.EXPORTS if n.endswith("_bytes") and ("clip" in n or "cull_faces" in n)]


def test_launch_counts_and_what_the_sources_do_not_use():
    render, cull = _src("map_meshrender.hip"), _src("map_meshcull.hip")
    for name in ("dqo_mesh_render_depth", "dqo_mesh_render_depth_clip"):
        assert _entry_body(render, name).count("DQO_LAUNCH(") == 3, name
    assert "mesh_render_raster_kernel<false>" in _entry_body(render, "dqo_mesh_render_depth")
    assert "mesh_render_raster_kernel<true>" in _entry_body(render, "dqo_mesh_render_depth_clip")
    for name in ("dqo_mesh_cull", "dqo_mesh_cull_faces"):
        assert _entry_body(cull, name).count("DQO_LAUNCH(") == 6, name
    for reused in ("mesh_cull_vcount_kernel", "mesh_cull_vscatter_kernel", "mesh_cull_fscatter_kernel"):
        assert reused in _entry_body(cull, "dqo_mesh_cull_faces")
    code = [l.split("//")[0] for l in render.splitlines()]
    assert sum("__hip_atomic_fetch_min" in l for l in code) == 1  # still one pixel function, one 64-bit key path
    for src in (render, cull):
        assert "hipMemset" not in src and "atomicAdd((float" not in src and "atomicAdd_f" not in src and "hipStreamSynchronize" not in src
        assert "hipMemcpy" not in src and "hipDeviceSynchronize" not in src


def _clip(native, cap_v=100, cap_f=200, vertices=FAKE, faces=FAKE + 64, counts=FAKE + 128, n_views=3, w2c=FAKE + 512, view_keep=None, W=64,
          H=48, K=(40.0, 42.0, 31.5, 23.5), near=0.0, depth_trunc=INF, depth=FAKE + 1024, face_index=None, header=FAKE + 320, ws=None,
          ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_render_depth_clip(vertices, faces, counts, cap_v, cap_f, n_views, w2c, view_keep, W, H, *K, near, depth_trunc, depth,
                                        face_index, header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_clip_validation_before_launch(native):
    for caps in ((0, 8), (8, 0), (1 << 28, 8)):
        rc, err = _clip(native, cap_v=caps[0], cap_f=caps[1])
        assert rc == -1 and "bad capacity" in err, (caps, err)
    for name in ("vertices", "faces", "header"):
        rc, err = _clip(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    for n in (0, 65536):
        rc, err = _clip(native, n_views=n)
        assert rc == -1 and "bad n_views" in err, n
    rc, err = _clip(native, w2c=None)
    assert rc == -1 and "null w2c" in err
    for kw in (dict(W=0), dict(H=-1), dict(W=(1 << 24) + 1, H=1), dict(W=1 << 20, H=1 << 20)):
        rc, err = _clip(native, **kw)
        assert rc == -1 and "bad image size" in err, kw
    rc, err = _clip(native, cap_f=1 << 27, n_views=16)
    assert rc == -1 and "too many pairs" in err
    for bad in (-0.5, NAN, INF):
        rc, err = _clip(native, near=bad)
        assert rc == -1 and "bad near" in err, bad
    for bad in (0.0, -1.0, NAN):
        rc, err = _clip(native, depth_trunc=bad)
        assert rc == -1 and "bad depth_trunc" in err, bad
    rc, err = _clip(native, depth=None)
    assert rc == -1 and "null depth" in err
    rc, err = _clip(native, header=FAKE + 256, counts=FAKE + 256)
    assert rc == -1 and "header must not be the mesh's counts" in err
    need = native.lib().dqo_mesh_render_depth_workspace_bytes(3, 64, 48)  # the plain entry's query is this entry's
    rc, err = _clip(native, ws=FAKE, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh render workspace too small ({need - 1} < {need})"
    for kw in (dict(counts=None), dict(view_keep=FAKE + 2048), dict(face_index=FAKE + 4096), dict(near=0.5), dict(W=1, H=1)):
        rc, err = _clip(native, ws=None, **kw)
        assert rc == -2, (kw, err)


def _faces(native, cap_v=100, cap_f=200, vertices=FAKE, colors=None, faces=FAKE + 64, counts=FAKE + 128, n_views=3, view_keep=None, W=64, H=48,
           face_index=FAKE + 512, rdepth=FAKE + 1024, depth=None, eps=0.03, depth_trunc=INF, min_pixels=1, out_vertices=FAKE + 2048,
           out_colors=None, out_faces=FAKE + 4096, out_cap_v=100, out_cap_f=200, face_pixels=FAKE + 8192, header=FAKE + 320, ws=None,
           ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_cull_faces(vertices, colors, faces, counts, cap_v, cap_f, n_views, view_keep, W, H, face_index, rdepth, depth, eps,
                                 depth_trunc, min_pixels, out_vertices, out_colors, out_faces, out_cap_v, out_cap_f, face_pixels, header, ws,
                                 ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_cull_faces_validation_before_launch(native):
    for caps in ((0, 8), (8, 0), (-3, 8), (1 << 28, 8), (8, 1 << 28)):
        rc, err = _faces(native, cap_v=caps[0], cap_f=caps[1], out_cap_v=1 << 28, out_cap_f=1 << 28)
        assert rc == -1 and "bad capacity" in err and "2^28" in err, (caps, err)
    for name in ("vertices", "faces", "header"):
        rc, err = _faces(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    for n in (0, -1, 65536):
        rc, err = _faces(native, n_views=n)
        assert rc == -1 and "bad n_views" in err, n
    for kw in (dict(W=0), dict(H=0), dict(W=-4), dict(W=1 << 20, H=1 << 20)):
        rc, err = _faces(native, **kw)
        assert rc == -1 and "bad image size" in err and "2^40" in err, kw
    for name in ("face_index", "rdepth"):
        rc, err = _faces(native, **{name: None})
        assert rc == -1 and "null face_index / rdepth" in err, name
    rc, err = _faces(native, face_pixels=None)
    assert rc == -1 and "null face_pixels" in err
    for bad in (-0.5, NAN, INF):
        rc, err = _faces(native, eps=bad)
        assert rc == -1 and "bad eps" in err, bad
    for bad in (0.0, -1.0, NAN):
        rc, err = _faces(native, depth_trunc=bad)
        assert rc == -1 and "bad depth_trunc" in err, bad
    for bad in (0, -1, -(1 << 31)):
        rc, err = _faces(native, min_pixels=bad)
        assert rc == -1 and "bad min_pixels" in err, bad
    for kw in (dict(out_cap_v=99), dict(out_cap_f=199)):
        rc, err = _faces(native, **kw)
        assert rc == -1 and "out capacity" in err, kw
    for kw in (dict(out_vertices=None), dict(out_faces=None), dict(colors=FAKE + 32, out_colors=None)):
        rc, err = _faces(native, **kw)
        assert rc == -1 and "null out mesh buffer" in err, kw
    for kw in (dict(out_vertices=FAKE), dict(out_faces=FAKE + 64), dict(colors=FAKE + 32, out_colors=FAKE + 32)):  # an out buffer that is the input's
        rc, err = _faces(native, **kw)
        assert rc == -1 and "the out mesh must not be the input mesh" in err, kw
    rc, err = _faces(native, header=FAKE + 128)
    assert rc == -1 and "header must not be the input's counts" in err
    for alias in (FAKE + 64, FAKE + 4096, FAKE + 320, FAKE + 128):
        rc, err = _faces(native, face_pixels=alias)
        assert rc == -1 and "face_pixels must be a buffer of its own" in err, alias
    need = native.lib().dqo_mesh_cull_workspace_bytes(100, 200)  # dqo_mesh_cull's query is this entry's
    rc, err = _faces(native, ws=FAKE, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh cull workspace too small ({need - 1} < {need})"
    rc, err = _faces(native, ws=None, ws_bytes=need)
    assert rc == -2
    for kw in (dict(counts=None), dict(view_keep=FAKE + 16), dict(depth=FAKE + 16384), dict(min_pixels=(1 << 31) - 1), dict(eps=0.0),
               dict(depth_trunc=5.0), dict(colors=FAKE + 32, out_colors=FAKE + 48), dict(out_cap_v=101, out_cap_f=1000), dict(W=1, H=1, n_views=1)):
        rc, err = _faces(native, ws=None, **kw)
        assert rc == -2, (kw, err)
    rc, err = _faces(native, cap_v=0, ws=None, ws_bytes=0)  # argument errors come first, whatever the workspace
    assert rc == -1 and "bad capacity" in err


def test_python_surface(native):
    import torch
    import dqo_eval
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.mesh_render_depth_clip) == P(dqo_eval.mesh_render_depth)
    assert P(dqo_eval.mesh_cull_visible) == [("mesh", E), ("w2c", E), ("K", E), ("W", E), ("H", E), ("depth", None), ("view_keep", None),
                                             ("eps", 0.03), ("near", 0.0), ("depth_trunc", INF), ("min_pixels", 1), ("out", None),
                                             ("want_pixels", False)]
    assert P(F.FusedMapper.evaluate_mesh_visible) == [("self", E), ("mesh", E), ("gt_vertices", E), ("gt_faces", E), ("frames", E),
                                                      ("depths", None), ("sample_nums", 1000000), ("seed", 0), ("dist_thres", (0.03,)),
                                                      ("transform", None), ("eps", 0.03), ("min_pixels", 1), ("depth_trunc", INF), ("out", None),
                                                      ("row", 0)]
    assert P(F.FusedMapper.evaluate_mesh_depth_clipped) == P(F.FusedMapper.evaluate_mesh_depth)
    assert dqo_eval.MESH_RENDER_CLIP_HEADER == C.HEADER and dqo_eval.MESH_RENDER_CLIP_HEADER[3] == "pairs_near_clipped"
    assert [a == b for a, b in zip(dqo_eval.MESH_RENDER_CLIP_HEADER, dqo_eval.MESH_RENDER_HEADER)].count(False) == 1
    assert dqo_eval.MESH_CULL_FACES_HEADER == C.CULL_HEADER and len(C.CULL_HEADER) == 8
    for fn in (dqo_eval.eval_mesh, dqo_eval.eval_mesh_depth):  # the opt-in keys of the views
        assert ("visibility" in fn.__doc__) and ("clip_near" in fn.__doc__)
    mesh = dict(vertices=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    views = dict(w2c=torch.zeros((1, 16)), K=(40.0, 42.0, 31.5, 23.5), W=64, H=48)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.mesh_render_depth_clip(mesh, **views)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.mesh_cull_visible(mesh, **views)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh_depth(mesh, mesh, dict(views, clip_near=True, visibility="faces", min_pixels=2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh(mesh, mesh, views=dict(views, visibility="faces", clip_near=True, min_corners=2), sample_nums=10)
    with pytest.raises(RuntimeError, match="'vertices' or 'faces'"):
        dqo_eval.eval_mesh(mesh, mesh, views=dict(views, visibility="corners"), sample_nums=10)
    r = dict(header=torch.tensor([2, 1, 40, 3, 2, 5, 777, 0], dtype=torch.int32), header_names=dqo_eval.MESH_RENDER_CLIP_HEADER)
    assert dqo_eval.mesh_counts(r)["pairs_near_clipped"] == 3
