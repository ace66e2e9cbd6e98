"""CPU-side checks of the mesh evaluation's entry points (dqo_mesh_cull, csrc/map_meshcull.hip; dqo_mesh_sample_counted,
csrc/map_meshsample.hip; their workspace queries): the four symbols are declared, exported and bound, the ABI did not move, the size
queries behave, every argument error is reported before anything is launched (-1 for bad arguments, then -2 for a short workspace; no
GPU here), the launch counts are the header's words, and the Python surface is the documented one."""
import ctypes
import inspect
import os

import pytest

import mesh_cull_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_cull_workspace_bytes", "dqo_mesh_cull", "dqo_mesh_sample_counted_workspace_bytes", "dqo_mesh_sample_counted")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
BIG = 1 << 40
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
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(native.lib(), s).argtypes
    L = native.lib()
    assert L.dqo_mesh_cull_workspace_bytes.restype is ctypes.c_size_t and L.dqo_mesh_sample_counted_workspace_bytes.restype is ctypes.c_size_t
    assert L.dqo_mesh_cull.argtypes[11:15] == [ctypes.c_float] * 4 and L.dqo_mesh_cull.argtypes[16:19] == [ctypes.c_float] * 3
    assert L.dqo_mesh_sample_counted.argtypes[6] is ctypes.c_uint64  # the seed
    for cite in ("pc_z > near", "u_f >= 0.0001f && u_f < (float)W - 0.0001f", "pc_z <= d + eps", "min_corners", "F = [1] + [4] + [5]",
                 "V = [0] + [6]", "tests/mesh_cull_oracle.py", "triangle-frustum intersection", "bit_length(F)"):
        assert cite in hdr, cite
    makefile = _src("Makefile")
    assert "map_meshcull.hip" in makefile and "../build/map_meshcull.o: HIPFLAGS += -ffp-contract=off" in makefile


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = native.lib()
    assert lib.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert lib.dqo_abi_sizeof(13) == 0 and lib.dqo_abi_sizeof(16) == 0  # (no new struct: the entries take plain arguments)


def test_launch_counts_and_what_the_sources_do_not_use():
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    cull, sample = _src("map_meshcull.hip"), _src("map_meshsample.hip")
    assert cull.index("mesh_cull_fscatter_kernel") < cull.index('extern "C"')  # the entry points sit behind their launches
    assert _entry_body(cull, "dqo_mesh_cull").count("DQO_LAUNCH(") == 6 and "Six launches" in hdr and "six launches" in cull
    # both sampler entries go through one launch function: dqo_mesh_sample keeps its four launches, the counted one has the same four
    launch = sample[sample.index("static int dqo_launch_mesh_sample("):]
    launch = launch[:launch.index("return DQO_OK;")]
    assert launch.count("DQO_LAUNCH(") == 4 and "same four launches" in hdr and "Four launches" in hdr
    for name in ("dqo_mesh_sample", "dqo_mesh_sample_counted"):
        body = _entry_body(sample, name)
        assert body.count("dqo_launch_mesh_sample<") == 1 and "DQO_LAUNCH(" not in body
    for src in (cull, sample):
        assert "hipMemset" not in src and "atomicAdd((float" not in src and "atomicAdd_f" not in src and "hipStreamSynchronize" not in src
        assert "hipMemcpy" not in src and "hipDeviceSynchronize" not in src
    assert "float*" not in "".join(l for l in cull.splitlines() if "atomic" in l.split("//")[0])  # integer atomics only


def test_workspace_bytes(native):
    f = native.lib().dqo_mesh_cull_workspace_bytes
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -5), (1 << 28, 8), (8, 1 << 28)):
        assert f(*bad) == 0, bad
    assert f(1, 1) > 0 and f((1 << 28) - 1, (1 << 28) - 1) > 1 << 31  # (size_t: not cut at 32 bits)
    sizes = (1, 2, 255, 256, 257, 2048, 2049, 6498, 100000, 1 << 22)
    for a in sizes:
        row = [f(a, b) for b in sizes]
        col = [f(b, a) for b in sizes]
        assert row == sorted(row) and col == sorted(col), a  # they do not decrease as a capacity grows
        assert all(n % 256 == 0 for n in row)
    assert f(1000, 2000) >= 4 * 1000 + 4 * 1000 + 2000  # a view count and a mark per vertex, a keep byte per face
    g, h = native.lib().dqo_mesh_sample_counted_workspace_bytes, native.lib().dqo_mesh_sample_workspace_bytes
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -5), (1 << 25, 8), (8, 1 << 25)):
        assert g(*bad) == 0, bad
    big = (1 << 25) - 1
    assert g(1, 1) > 0 and g(big, big) >= 8 * big
    fsizes = (1, 2, 1023, 1024, 1025, 2049, 4096, 100000, 1 << 22)
    row = [g(a, 1000) for a in fsizes]
    assert row == sorted(row) and all(n % 256 == 0 for n in row)
    assert all(g(a, c) == h(a, c) for a in fsizes for c in (1, 257, 4099))  # dqo_mesh_sample's of the capacity


def _cull(native, cap_v=100, cap_f=200, vertices=FAKE, colors=FAKE, faces=FAKE, counts=FAKE, n_views=3, w2c=FAKE + 512, view_keep=None, W=64,
          H=48, K=(40.0, 42.0, 31.5, 23.5), depth=FAKE + 1024, near=0.0, eps=0.02, depth_trunc=INF, min_corners=3, out_v=FAKE + 64,
          out_c=FAKE + 128, out_f=FAKE + 192, out_cap_v=None, out_cap_f=None, vertex_views=None, header=FAKE + 320, ws=FAKE, ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_cull(vertices, colors, faces, counts, cap_v, cap_f, n_views, w2c, view_keep, W, H, *K, depth, near, eps, depth_trunc,
                           min_corners, out_v, out_c, out_f, cap_v if out_cap_v is None else out_cap_v,
                           cap_f if out_cap_f is None else out_cap_f, vertex_views, header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_cull_validation_before_launch(native):
    for caps in ((0, 8), (8, 0), (-3, 8), (1 << 28, 8), (8, 1 << 28)):
        rc, err = _cull(native, cap_v=caps[0], cap_f=caps[1])
        assert rc == -1 and "bad capacity" in err and "2^28" in err, (caps, err)
    for name in ("vertices", "faces", "header"):
        rc, err = _cull(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    for n in (0, -1, 65536, 1 << 20):
        rc, err = _cull(native, n_views=n)
        assert rc == -1 and "bad n_views" in err and "65535" in err, n
    rc, err = _cull(native, w2c=None)
    assert rc == -1 and "null w2c" in err
    for kw in (dict(W=0), dict(H=0), dict(W=-4), dict(H=-1), dict(W=1 << 20, H=1 << 20), dict(n_views=65535, W=1 << 14, H=1 << 14),
               dict(n_views=65535, W=(1 << 31) - 1, H=(1 << 31) - 1)):
        rc, err = _cull(native, **kw)
        assert rc == -1 and "bad image size" in err and "2^40" in err, kw
    for name in ("near", "eps"):
        for bad in (-0.5, NAN, INF, -INF):
            rc, err = _cull(native, **{name: bad})
            assert rc == -1 and f"bad {name}" in err, (name, bad)
    for bad in (0.0, -1.0, NAN, -INF):
        rc, err = _cull(native, depth_trunc=bad)
        assert rc == -1 and "bad depth_trunc" in err, bad
    for bad in (0, 4, -1):
        rc, err = _cull(native, min_corners=bad)
        assert rc == -1 and "bad min_corners" in err, bad
    for name in ("out_v", "out_c", "out_f"):
        rc, err = _cull(native, **{name: None})
        assert rc == -1 and "null out mesh buffer" in err, name
    for kw in (dict(out_v=FAKE), dict(out_f=FAKE), dict(out_c=FAKE)):
        rc, err = _cull(native, ws=None, **kw)
        assert rc == -1 and "must not be the input mesh" in err, kw
    rc, err = _cull(native, header=FAKE + 256, counts=FAKE + 256, ws=None)  # the header would be cleared before the counts are read
    assert rc == -1 and "header must not be the input's counts" in err
    for kw in (dict(out_cap_v=99), dict(out_cap_f=199)):
        rc, err = _cull(native, **kw)
        assert rc == -1 and "out capacity" in err and "below the input's" in err, kw
    need = native.lib().dqo_mesh_cull_workspace_bytes(100, 200)
    rc, err = _cull(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh cull workspace too small ({need - 1} < {need})"
    rc, err = _cull(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"mesh cull workspace too small ({need} < {need})"
    # what may be NULL or at its limit gets as far as the workspace
    for kw in (dict(colors=None, out_c=None), dict(counts=None), dict(depth=None), dict(view_keep=FAKE + 2048), dict(vertex_views=FAKE + 4096),
               dict(depth_trunc=5.0), dict(near=0.5, eps=0.0), dict(n_views=1), dict(n_views=65535), dict(min_corners=1), dict(min_corners=2),
               dict(out_cap_v=101, out_cap_f=1000)):
        rc, err = _cull(native, ws=None, **kw)
        assert rc == -2, (kw, err)
    rc, err = _cull(native, cap_v=0, ws=None, ws_bytes=0)  # argument errors come first, whatever the workspace
    assert rc == -1 and "bad capacity" in err


def _sample(native, cap_v=100, cap_f=200, vertices=FAKE, faces=FAKE + 64, counts=FAKE + 128, count=1000, seed=7, points=FAKE + 192,
            face_index=None, keep=FAKE + 256, header=FAKE + 320, ws=FAKE, ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_sample_counted(vertices, faces, counts, cap_v, cap_f, count, seed, points, face_index, keep, header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_sample_counted_validation_before_launch(native):
    for cv in (0, -1, 1 << 28):
        rc, err = _sample(native, cap_v=cv)
        assert rc == -1 and "bad vertex capacity" in err, cv
    for cf in (0, -1, 1 << 25):
        rc, err = _sample(native, cap_f=cf)
        assert rc == -1 and "bad face capacity" in err and "2^25 - 1" in err, cf
    for n in (0, -1, 1 << 25):
        rc, err = _sample(native, count=n)
        assert rc == -1 and "bad sample count" in err and "2^25 - 1" in err, n
    for name in ("vertices", "faces", "points", "keep", "header"):
        rc, err = _sample(native, **{name: None})
        assert rc == -1 and "null pointer" in err, name
    rc, err = _sample(native, header=FAKE + 128, ws=None)
    assert rc == -1 and "header must not be the mesh's counts" in err
    need = native.lib().dqo_mesh_sample_counted_workspace_bytes(200, 1000)
    rc, err = _sample(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh sample workspace too small ({need - 1} < {need})"
    for kw in (dict(counts=None), dict(face_index=FAKE + 512), dict(cap_f=(1 << 25) - 1, ws_bytes=0), dict(count=(1 << 25) - 1)):
        rc, err = _sample(native, ws=None, **kw)
        assert rc == -2, (kw, err)


def test_python_surface(native):
    import torch
    import dqo_eval
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.mesh_cull) == [("mesh", E), ("w2c", E), ("K", E), ("W", E), ("H", E), ("depth", None), ("view_keep", None), ("eps", 0.03),
                                     ("near", 0.0), ("depth_trunc", INF), ("min_corners", 3), ("out", None), ("want_views", False),
                                     ("workspace_buffer", None)]
    assert P(dqo_eval.sample_surface_counted) == [("mesh", E), ("count", E), ("seed", 0), ("want_face_index", False), ("workspace_buffer", None)]
    assert P(dqo_eval.eval_mesh) == [("rec_mesh", E), ("gt_mesh", E), ("sample_nums", 1000000), ("seed", 0), ("rec_seed", None),
                                     ("dist_thres", (0.03,)), ("transform", None), ("views", None), ("out", None), ("row", 0)]
    assert P(F.FusedMapper.evaluate_mesh) == [("self", E), ("mesh", E), ("gt_vertices", E), ("gt_faces", E), ("frames", None), ("depths", None),
                                              ("sample_nums", 1000000), ("seed", 0), ("dist_thres", (0.03,)), ("transform", None), ("eps", 0.03),
                                              ("min_corners", 3), ("depth_trunc", INF), ("out", None), ("row", 0)]
    assert dqo_eval.MESH_CULL_HEADER == C.HEADER and len(C.HEADER) == 8
    mesh = dict(vertices=torch.zeros((4, 3)), colors=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.mesh_cull(mesh, torch.zeros((1, 16)), (40.0, 42.0, 31.5, 23.5), 64, 48)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.sample_surface_counted(mesh, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh(mesh, mesh, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh(mesh, mesh, 10, views=dict(w2c=torch.zeros((1, 16)), K=(40.0, 42.0, 31.5, 23.5), W=64, H=48))
    mesh["header"] = torch.tensor([3, 1, 4, 2, 0, 1, 1, 0], dtype=torch.int32)
    mesh["header_names"] = dqo_eval.MESH_CULL_HEADER
    assert dqo_eval.mesh_counts(mesh) == dict(vertices=3, faces=1, vertices_seen=4, views_used=2, faces_bad_index=0, faces_removed=1,
                                              vertices_removed=1, zero=0)
