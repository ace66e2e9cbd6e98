"""CPU-side checks of the mesh depth render's and Depth L1's entry points (dqo_mesh_render_depth, csrc/map_meshrender.hip;
dqo_eval_depth_l1, csrc/map_eval.hip; their workspace queries): the four symbols are declared, exported and bound, the ABI did not move,
the size queries behave, every argument error is reported before anything is launched (-1 for bad arguments, then -2 for a short
workspace; no GPU here), the launch counts are the header's words, and the Python surface is the documented one."""
import ctypes
import inspect
import os

import pytest

import depth_l1_oracle as D
import mesh_render_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_render_depth_workspace_bytes", "dqo_mesh_render_depth", "dqo_eval_depth_l1_workspace_bytes", "dqo_eval_depth_l1")
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
    assert L.dqo_mesh_render_depth_workspace_bytes.restype is ctypes.c_size_t and L.dqo_eval_depth_l1_workspace_bytes.restype is ctypes.c_size_t
    assert L.dqo_mesh_render_depth.argtypes[10:16] == [ctypes.c_float] * 6 and L.dqo_mesh_render_depth.argtypes[20] is ctypes.c_size_t
    assert L.dqo_eval_depth_l1.argtypes[6] is ctypes.c_float and L.dqo_eval_depth_l1.argtypes[9] is ctypes.c_size_t
    for cite in ("CROSSES\n *       THE NEAR PLANE", "ordered by VERTEX ID", "SMALL_MAX = 64", "MINIMUM key", "tests/mesh_render_oracle.py",
                 "tests/depth_l1_oracle.py", "Not built: near-plane clipping, back-face culling", "the NICE-SLAM form"):
        assert cite in hdr, cite
    assert "Not built: rendering the mesh" not in hdr
    makefile = _src("Makefile")
    assert "map_meshrender.hip" in makefile and "../build/map_meshrender.o: HIPFLAGS += -ffp-contract=off" in makefile


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = native.lib()
    assert lib.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert lib.dqo_abi_sizeof(13) == 0 and lib.dqo_abi_sizeof(16) == 0  # (no new struct: the entries take plain arguments)


def test_launch_counts_and_what_the_sources_do_not_use():
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    render, ev = _src("map_meshrender.hip"), _src("map_eval.hip")
    assert render.index("mesh_render_resolve_kernel") < render.index('extern "C"')  # the entry points sit behind their launches
    assert _entry_body(render, "dqo_mesh_render_depth").count("DQO_LAUNCH(") == 3 and "Three launches" in hdr and "three launches" in render
    assert _entry_body(ev, "dqo_eval_depth_l1").count("DQO_LAUNCH(") == 2 and "Two launches" in hdr
    for src in (render, ev):
        assert "hipMemset" not in src and "atomicAdd((float" not in src and "atomicAdd_f" not in src and "hipStreamSynchronize" not in src
        assert "hipMemcpy" not in src and "hipDeviceSynchronize" not in src
    code = [l.split("//")[0] for l in render.splitlines()]
    assert "float*" not in "".join(l for l in code if "atomic" in l) and "double*" not in "".join(l for l in code if "atomic" in l)
    assert sum("__hip_atomic_fetch_min" in l for l in code) == 1  # one pixel function, one 64-bit key path
    assert "MR_SMALL_MAX = 64" in render and R.SMALL_MAX == 64


def test_workspace_bytes(native):
    f = native.lib().dqo_mesh_render_depth_workspace_bytes
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, (1 << 24) + 1, 1), (1, 1, (1 << 24) + 1),
                (1, 1 << 20, 1 << 20), (65535, 1 << 14, 1 << 14)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1) > 0 and f(1, 1 << 24, 1 << 15) > 8 << 39  # (size_t: not cut at 32 bits)
    sizes = (1, 2, 31, 32, 33, 64, 255, 680, 1200)
    for n in (1, 2, 33, 100):
        for a in sizes:
            row = [f(n, a, b) for b in sizes]
            assert row == sorted(row) and all(x % 256 == 0 for x in row), (n, a)
            assert [f(n, b, a) for b in sizes] == sorted(f(n, b, a) for b in sizes)
        assert [f(m, 64, 48) for m in (1, 2, 33, 100, 65535)] == sorted(f(m, 64, 48) for m in (1, 2, 33, 100, 65535))
    assert f(3, 37, 29) >= 8 * 3 * 37 * 29  # an 8-byte key per pixel
    g = native.lib().dqo_eval_depth_l1_workspace_bytes
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1 << 12, 1 << 12), (1, 1 << 24, 1)):
        assert g(*bad) == 0, bad
    assert g(1, 1, 1) > 0 and g(1, 4095, 4096) > 0
    row = [g(n, 64, 48) for n in (1, 2, 33, 100, 4000)]
    assert row == sorted(row) and all(x % 256 == 0 for x in row)
    row = [g(3, w, 48) for w in sizes]
    assert row == sorted(row) and all(x % 256 == 0 for x in row)


def _render(native, cap_v=100, cap_f=200, vertices=FAKE, faces=FAKE + 64, counts=FAKE + 128, n_views=3, w2c=FAKE + 512, view_keep=None, W=64,
            H=48, K=(40.0, 42.0, 31.5, 23.5), near=0.0, depth_trunc=INF, depth=FAKE + 1024, face_index=None, header=FAKE + 320, ws=None,
            ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_render_depth(vertices, faces, counts, cap_v, cap_f, n_views, w2c, view_keep, W, H, *K, near, depth_trunc, depth, face_index,
                                   header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_render_validation_before_launch(native):
    for caps in ((0, 8), (8, 0), (-3, 8), (1 << 28, 8), (8, 1 << 28)):
        rc, err = _render(native, cap_v=caps[0], cap_f=caps[1])
        assert rc == -1 and "bad capacity" in err and "2^28" in err, (caps, err)
    for name in ("vertices", "faces", "header"):
        rc, err = _render(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    for n in (0, -1, 65536, 1 << 20):
        rc, err = _render(native, n_views=n)
        assert rc == -1 and "bad n_views" in err and "65535" in err, n
    rc, err = _render(native, w2c=None)
    assert rc == -1 and "null w2c" in err
    for kw in (dict(W=0), dict(H=0), dict(W=-4), dict(H=-1), dict(W=1 << 20, H=1 << 20), dict(n_views=65535, W=1 << 14, H=1 << 14, cap_f=8),
               dict(W=(1 << 24) + 1, H=1), dict(W=1, H=(1 << 24) + 1)):
        rc, err = _render(native, **kw)
        assert rc == -1 and "bad image size" in err and "2^40" in err and "2^24" in err, kw
    for kw in (dict(cap_f=1 << 27, n_views=16), dict(cap_f=(1 << 28) - 1, n_views=9), dict(cap_f=32769, n_views=65535, W=8, H=8)):
        rc, err = _render(native, **kw)
        assert rc == -1 and "too many pairs" in err and "2^31" in err, kw
    for bad in (-0.5, NAN, INF, -INF):
        rc, err = _render(native, near=bad)
        assert rc == -1 and "bad near" in err, bad
    for bad in (0.0, -1.0, NAN, -INF):
        rc, err = _render(native, depth_trunc=bad)
        assert rc == -1 and "bad depth_trunc" in err, bad
    rc, err = _render(native, depth=None)
    assert rc == -1 and "null depth" in err
    rc, err = _render(native, header=FAKE + 256, counts=FAKE + 256, ws=None)
    assert rc == -1 and "header must not be the mesh's counts" in err
    need = native.lib().dqo_mesh_render_depth_workspace_bytes(3, 64, 48)
    rc, err = _render(native, ws=FAKE, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh render workspace too small ({need - 1} < {need})"
    rc, err = _render(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"mesh render workspace too small ({need} < {need})"
    # what may be NULL or at its limit gets as far as the workspace
    for kw in (dict(counts=None), dict(view_keep=FAKE + 2048), dict(face_index=FAKE + 4096), dict(depth_trunc=5.0), dict(near=0.5), dict(n_views=1),
               dict(n_views=65535, cap_f=32768, W=8, H=8), dict(W=1, H=1), dict(W=1 << 24, H=1, n_views=1), dict(cap_f=(1 << 28) - 1, n_views=7)):
        rc, err = _render(native, ws=None, **kw)
        assert rc == -2, (kw, err)
    rc, err = _render(native, cap_v=0, ws=None, ws_bytes=0)  # argument errors come first, whatever the workspace
    assert rc == -1 and "bad capacity" in err


def _l1(native, n=3, W=64, H=48, a=FAKE, b=FAKE + 64, view_keep=None, depth_trunc=INF, out=FAKE + 128, ws=None, ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_eval_depth_l1(n, W, H, a, b, view_keep, depth_trunc, out, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_depth_l1_validation_before_launch(native):
    for n in (0, -1, 65536):
        rc, err = _l1(native, n=n)
        assert rc == -1 and "bad n_views" in err, n
    for kw in (dict(W=0), dict(H=-1), dict(W=1 << 12, H=1 << 12), dict(W=1 << 24, H=1)):
        rc, err = _l1(native, **kw)
        assert rc == -1 and "bad image size" in err and "2^24" in err, kw
    for name in ("a", "b", "out"):
        rc, err = _l1(native, **{name: None})
        assert rc == -1 and "null pointer" in err, name
    for bad in (0.0, -1.0, NAN, -INF):
        rc, err = _l1(native, depth_trunc=bad)
        assert rc == -1 and "bad depth_trunc" in err, bad
    need = native.lib().dqo_eval_depth_l1_workspace_bytes(3, 64, 48)
    rc, err = _l1(native, ws=FAKE, ws_bytes=need - 1)
    assert rc == -2 and err == f"depth L1 workspace too small ({need - 1} < {need})"
    for kw in (dict(view_keep=FAKE + 256), dict(depth_trunc=4.0), dict(n=1, W=1, H=1), dict(n=65535, W=4, H=4), dict(W=4095, H=4096, n=1)):
        rc, err = _l1(native, ws=None, **kw)
        assert rc == -2, (kw, err)


def test_python_surface(native):
    import torch
    import dqo_eval
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.mesh_render_depth) == [("mesh", E), ("w2c", E), ("K", E), ("W", E), ("H", E), ("view_keep", None), ("near", 0.0),
                                             ("depth_trunc", INF), ("want_face_index", False), ("out", None), ("workspace_buffer", None)]
    assert P(dqo_eval.depth_l1) == [("depth_gt", E), ("depth_rec", E), ("view_keep", None), ("depth_trunc", INF), ("out", None)]
    assert P(dqo_eval.depth_l1_dict) == [("table", E)]
    assert P(dqo_eval.eval_mesh_depth) == [("rec_mesh", E), ("gt_mesh", E), ("views", E), ("out", None)]
    assert P(F.FusedMapper.evaluate_mesh_depth) == [("self", E), ("mesh", E), ("gt_vertices", E), ("gt_faces", E), ("frames", E),
                                                    ("depth_trunc", INF), ("out", None)]
    assert dqo_eval.MESH_RENDER_HEADER == R.HEADER and len(R.HEADER) == 8 and dqo_eval.DEPTH_L1_ROW == D.ROW and len(D.ROW) == 8
    for fn in (dqo_eval.mesh_cull, F.FusedMapper.evaluate_mesh):  # the rendered stack is a depth for the cull
        assert "mesh_render_depth" in fn.__doc__ and "no sensor depth exists" in fn.__doc__
    mesh = dict(vertices=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    views = dict(w2c=torch.zeros((1, 16)), K=(40.0, 42.0, 31.5, 23.5), W=64, H=48)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.mesh_render_depth(mesh, **views)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.depth_l1(torch.zeros((1, 4, 4)), torch.zeros((1, 4, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh_depth(mesh, mesh, views)
    r = dict(header=torch.tensor([2, 1, 40, 3, 2, 5, 777, 0], dtype=torch.int32), header_names=dqo_eval.MESH_RENDER_HEADER)
    assert dqo_eval.mesh_counts(r) == dict(views_used=2, faces_bad_index=1, pairs_rasterised=40, pairs_near_dropped=3, pairs_degenerate=2,
                                           pairs_cooperative=5, pixels_hit=777, zero=0)
    table = torch.tensor([[0.5, 0.25, 0.75, 10, 2, 3, 1, 1.5], [NAN] * 8, [0.5, 0.25, 0.75, 10, 2, 3, 1, 1.5]])
    d = dqo_eval.depth_l1_dict(table)
    assert d["views"][1] is None and d["views"][0] == d["mean"] == dict(l1_valid=0.5, l1_image=0.25, rmse_valid=0.75, both=10, only_a=2, only_b=3,
                                                                         neither=1, max_abs=1.5)


def test_depth_l1_oracle_on_hand_made_stacks():
    """The oracle alone, against numbers worked out by hand."""
    import numpy as np
    a = np.zeros((3, 2, 4), np.float32)
    b = np.zeros((3, 2, 4), np.float32)
    a[0] = [[1.0, 2.0, 0.0, 3.0], [0.0, 9.0, 1.0, 1.0]]
    b[0] = [[1.5, 0.0, 2.0, 1.0], [0.0, 9.0, 1.0, 0.0]]
    t = D.depth_l1(a, b, view_keep=[1, 1, 0], depth_trunc=5.0)  # (the 9 of a lies beyond the truncation: only b hits there)
    # valid: (1, 1.5), (3, 1), (1, 1): |d| = 0.5, 2, 0; image form adds 2 (only a), 2 (only b), 9 (only b: a truncated), 1 (only a)
    assert t[0].tolist() == [np.float32(2.5 / 3), np.float32(16.5 / 8), np.float32(np.sqrt(4.25 / 3)), 3.0, 2.0, 2.0, 1.0, 2.0]
    assert np.isnan(t[1][:3]).all() and t[1][3:].tolist() == [0.0, 0.0, 0.0, 8.0, 0.0] and np.isnan(t[2]).all()
    assert t[3].tolist() == [t[0][0], t[0][1], t[0][2], 3.0, 2.0, 2.0, 9.0, 2.0]


def test_the_new_size_queries_are_on_the_second_grid_and_equal_their_recorded_table(native):
    """tools/record_workspace_bytes.py's second grid: the size queries added since tests/workspace_bytes_parent.json was recorded have no
    parent to be held to; their table, tests/workspace_bytes_since.json, is the one recorded with this operator, entry by entry."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_workspace_bytes as rec
    assert rec.exports_since() == sorted(n for n in NEW if n.endswith("_bytes"))
    assert not set(rec.exports()) & set(NEW)
    now = rec.table_since(native.LIB_PATH)
    assert sorted({k.split("(")[0] for k in now}) == rec.exports_since()
    recorded = json.load(open(os.path.join(ROOT, "tests", "workspace_bytes_since.json")))
    assert sorted(recorded) == sorted(now)
    wrong = {k: (recorded[k], now[k]) for k in recorded if recorded[k] != now[k]}
    assert not wrong, wrong
    for query in rec.exports_since():
        for args in rec.STACKS_BAD:
            assert now[rec.key(query, args)] == 0, (query, args)
        assert all(now[rec.key(query, args)] > 0 and now[rec.key(query, args)] % 256 == 0 for args in rec.STACKS)
