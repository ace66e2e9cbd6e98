"""CPU-side checks of the exact point-to-triangle distance's entry points (dqo_mesh_nearest, csrc/knn.hip; dqo_eval_pcd_surface,
csrc/map_eval.hip; their workspace queries): the four symbols are declared, exported and bound from the header, the ABI did not move,
the size queries return 0 outside the limits, every argument error is reported before anything is launched (-1 for bad arguments, then
-2 for a short workspace; no GPU here), and the Python surface is the documented one."""
import ctypes
import inspect
import os

import pytest

import mesh_dist_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_nearest_workspace_bytes", "dqo_mesh_nearest", "dqo_eval_pcd_surface_workspace_bytes", "dqo_eval_pcd_surface")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
BIG = 1 << 40
TOP = (1 << 25) - 1


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def _src(name):
    return open(os.path.join(ROOT, "dqo-map_amd", "csrc", name)).read()


def test_symbols_are_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(native.lib(), s).argtypes
    L = native.lib()
    assert L.dqo_mesh_nearest_workspace_bytes.restype is ctypes.c_size_t and L.dqo_eval_pcd_surface_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.dqo_mesh_nearest.argtypes) == 17 and L.dqo_mesh_nearest.argtypes[15] is ctypes.c_size_t
    assert len(L.dqo_eval_pcd_surface.argtypes) == 24
    for cite in ("d1 / (d1 - d3)", "e / (e + g)", "1 / ((va + vb) + vc)", "fmaxf(E(p, f), B(p, aabb(f)))", "faces_bad_index", "faces_degenerate",
                 "tests/mesh_dist_oracle.py", "never contracted", "100 * sqrt(FLT_MAX)"):
        assert cite in hdr, cite
    knn = _src("knn.hip")
    section = knn[knn.index("---- dqo_mesh_nearest"):]
    assert "#pragma clang fp contract(off)" in section and "WHY THE CLAMP MAKES PRUNING EXACT" in section
    for word in ("hipMemset", "hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc", "atomicAdd((float", "atomicAdd_f"):
        assert word not in section, word


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = native.lib()
    assert lib.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert lib.dqo_abi_sizeof(13) == 0  # (no new struct: the entries take plain arguments)


def test_workspace_bytes(native):
    f = native.lib().dqo_mesh_nearest_workspace_bytes
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, -1, 8), (8, 8, -1), (1 << 25, 8, 8), (8, 8, 1 << 25), (8, 1 << 28, 8)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1) > 0 and f(TOP, (1 << 28) - 1, TOP) > 1 << 31  # (size_t: not cut at 32 bits)
    sizes = (1, 2, 63, 64, 65, 1023, 1025, 4097, 70001, 1 << 22)
    for a in sizes:
        row, col = [f(a, 100, b) for b in sizes], [f(b, 100, a) for b in sizes]
        assert row == sorted(row) and col == sorted(col) and all(n % 256 == 0 for n in row), a
    assert f(1000, 50, 2000) >= 16 * 1000 + 48 * 2000 + 12 * 2000  # a sorted query, three float4 and a centroid per face
    g, old = native.lib().dqo_eval_pcd_surface_workspace_bytes, native.lib().dqo_eval_pcd_workspace_bytes
    for bad in ((-1, 0, 0, 8, 0, 0), (8, 0, 0, 1 << 25, 0, 0), (8, 0, 5, 8, 0, 0), (8, 5, 0, 8, 0, 0), (8, 0, 0, 8, 5, 1 << 25), (8, 0, 0, 8, 1 << 28, 5),
                (8, -1, -1, 8, 0, 0)):
        assert g(*bad) == 0, bad
    assert g(0, 0, 0, 0, 0, 0) > 0 and g(100, 0, 0, 200, 0, 0) >= old(100, 200)  # (no mesh on either side: dqo_eval_pcd's searches)
    assert g(100, 50, 60, 200, 0, 0) > 0 and g(100, 0, 0, 200, 50, 60) > 0 and g(100, 50, 60, 200, 70, 80) > 0
    assert g(TOP, (1 << 28) - 1, TOP, TOP, (1 << 28) - 1, TOP) > 1 << 31


def test_the_size_queries_are_on_a_grid_of_their_own_and_equal_their_recorded_table(native):
    """tools/record_workspace_bytes.py's third grid: the two size queries have no parent to be held to; their table,
    tests/workspace_bytes_surface.json, is the one recorded with this operator, entry by entry."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_workspace_bytes as rec
    assert not set(rec.exports()) & set(NEW) and not set(rec.exports_since()) & set(NEW)
    now = rec.table_surface(native.LIB_PATH)
    assert sorted({k.split("(")[0] for k in now}) == sorted(n for n in NEW if n.endswith("_bytes"))
    recorded = json.load(open(os.path.join(ROOT, "tests", "workspace_bytes_surface.json")))
    assert sorted(recorded) == sorted(now)
    wrong = {k: (recorded[k], now[k]) for k in recorded if recorded[k] != now[k]}
    assert not wrong, wrong
    for args in rec.SURFACE_BAD:
        assert now[rec.key(NEW[0], args)] == 0, args
    for bad in rec.SURFACE_SIDES_BAD:
        assert now[rec.key(NEW[2], bad + rec.SURFACE_SIDES[1])] == 0 and now[rec.key(NEW[2], rec.SURFACE_SIDES[1] + bad)] == 0, bad
    assert all(n % 256 == 0 for n in now.values())


def _nearest(native, Q=100, q=FAKE, keep=None, qx=None, v=FAKE + 64, f=FAKE + 128, counts=FAKE + 192, cv=50, cf=60, mx=None, d2=FAKE + 256,
             face=FAKE + 320, closest=None, header=FAKE + 384, ws=FAKE, ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_nearest(Q, q, keep, qx, v, f, counts, cv, cf, mx, d2, face, closest, header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_mesh_nearest_validation_before_launch(native):
    for kw in (dict(Q=0), dict(Q=-1), dict(Q=1 << 25), dict(cf=0), dict(cf=-3), dict(cf=1 << 25), dict(cv=0), dict(cv=-1), dict(cv=1 << 28)):
        rc, err = _nearest(native, **kw)
        assert rc == -1 and "bad size" in err and "2^25 - 1" in err and "2^28" in err, (kw, err)
    for name in ("q", "d2"):
        rc, err = _nearest(native, **{name: None})
        assert rc == -1 and "null query / output" in err, name
    for name in ("v", "f", "header"):
        rc, err = _nearest(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    rc, err = _nearest(native, header=FAKE + 192, ws=None)  # the header would be cleared before the counts are read
    assert rc == -1 and "header must not be the mesh's counts" in err
    need = native.lib().dqo_mesh_nearest_workspace_bytes(100, 50, 60)
    rc, err = _nearest(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh nearest workspace too small ({need - 1} < {need})"
    rc, err = _nearest(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"mesh nearest workspace too small ({need} < {need})"
    # what may be NULL or at its limit gets as far as the workspace
    for kw in (dict(counts=None), dict(keep=FAKE + 512), dict(qx=FAKE + 576, mx=FAKE + 640), dict(face=None), dict(closest=FAKE + 704),
               dict(Q=TOP, ws_bytes=0), dict(cf=TOP, cv=(1 << 28) - 1, ws_bytes=0), dict(Q=1, cv=1, cf=1)):
        rc, err = _nearest(native, ws=None, **kw)
        assert rc == -2, (kw, err)
    rc, err = _nearest(native, Q=0, ws=None, ws_bytes=0)  # argument errors come first, whatever the workspace
    assert rc == -1 and "bad size" in err


def _surface(native, n_gt=100, gt=FAKE, gk=None, gm=(FAKE + 64, FAKE + 128, None, 50, 60), n_rec=200, rec=FAKE + 192, rk=None,
             rm=(FAKE + 256, FAKE + 320, FAKE + 384, 70, 80), xf=None, n_thres=1, out=FAKE + 448, row=0, ws=FAKE, ws_bytes=BIG):
    lib = native.lib()
    th = (ctypes.c_float * 8)(*([0.03] * 8)) if n_thres else None
    rc = lib.dqo_eval_pcd_surface(n_gt, gt, gk, *gm, n_rec, rec, rk, *rm, xf, n_thres, th, out, row, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_eval_pcd_surface_validation_before_launch(native):
    none = (None, None, None, 0, 0)
    for kw in (dict(n_gt=-1), dict(n_rec=1 << 25)):
        rc, err = _surface(native, **kw)
        assert rc == -1 and "bad size" in err, kw
    for bad in ((FAKE, FAKE, None, 0, 5), (FAKE, FAKE, None, 5, 0), (FAKE, FAKE, None, 5, 1 << 25), (FAKE, FAKE, None, 1 << 28, 5),
                (FAKE, None, None, 0, 0), (None, None, FAKE, 0, 0)):
        for side in ("gm", "rm"):
            rc, err = _surface(native, **{side: bad})
            assert rc == -1 and "bad mesh" in err, (side, bad)
    for bad in ((None, FAKE, None, 5, 5), (FAKE, None, None, 5, 5)):
        rc, err = _surface(native, gm=bad)
        assert rc == -1 and "null mesh buffer" in err, bad
    for kw in (dict(gt=None), dict(rec=None), dict(out=None)):
        rc, err = _surface(native, **kw)
        assert rc == -1 and "null pointer" in err, kw
    for n in (-1, 9):
        rc, err = _surface(native, n_thres=n)
        assert rc == -1 and "at most 8 thresholds" in err, n
    rc, err = _surface(native, row=-1)
    assert rc == -1 and "bad row" in err
    need = native.lib().dqo_eval_pcd_surface_workspace_bytes(100, 50, 60, 200, 70, 80)
    rc, err = _surface(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"eval_pcd surface workspace too small ({need - 1} < {need})"
    for kw in (dict(gm=none), dict(rm=none), dict(gm=none, rm=none), dict(n_thres=0), dict(n_thres=8), dict(xf=FAKE + 512), dict(n_gt=0, gt=None),
               dict(gk=FAKE + 576, rk=FAKE + 640)):
        rc, err = _surface(native, ws=None, **kw)
        assert rc == -2, (kw, err)


def test_python_surface(native):
    import torch
    import dqo_eval
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.nearest_on_mesh) == [("points", E), ("mesh", E), ("query_keep", None), ("query_transform", None), ("mesh_transform", None),
                                           ("want_face", True), ("want_closest", False), ("workspace_buffer", None)]
    assert P(dqo_eval.eval_pcd_surface) == [("gt_points", E), ("rec_points", E), ("gt_mesh", None), ("rec_mesh", None), ("dist_thres", (0.03,)),
                                            ("transform", None), ("gt_keep", None), ("rec_keep", None), ("out", None), ("row", 0),
                                            ("workspace_buffer", None)]
    # the surface forms stand beside functions whose signatures other tests pin: the same arguments, a name of their own
    assert P(dqo_eval.eval_mesh_surface) == P(dqo_eval.eval_mesh)
    assert P(F.FusedMapper.evaluate_geometry_mesh_surface) == P(F.FusedMapper.evaluate_geometry_mesh)
    assert P(F.FusedMapper.evaluate_mesh_surface) == P(F.FusedMapper.evaluate_mesh) + [("visibility", "vertices"), ("min_pixels", 1)]
    assert dqo_eval.MESH_NEAREST_HEADER == M.HEADER and len(M.HEADER) == 8
    mesh = dict(vertices=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    pts = torch.zeros((5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.nearest_on_mesh(pts, mesh)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_pcd_surface(pts, pts, gt_mesh=mesh)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_mesh_surface(mesh, mesh, 10)
