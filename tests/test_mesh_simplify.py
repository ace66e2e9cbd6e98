"""CPU-side checks of the mesh simplification (dqo_mesh_simplify and its workspace query; csrc/map_meshops.hip): the symbols are
declared, exported and bound, the size query behaves, every argument error is reported before anything is launched (-1 for bad
arguments, -2 for a short workspace; no GPU here), the Python surface is the documented one — and tests/mesh_simplify_oracle.py held
to facts that do not depend on it: its two restatements of the grouping agree, its output keeps the rule's invariants on every mesh
and cell size the GPU tests use, and the counts of the sphere are the ones worked out when the rule was written."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import mesh_simplify_oracle as S
import tsdf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_simplify_workspace_bytes", "dqo_mesh_simplify")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
BIG = 1 << 40
L = float(O.sphere_volume()[1])  # the sphere volume's voxel length, 1 / 24 as a float32
ORIGIN = (-0.5, -0.5, -0.5)  # the sphere volume's
WHOLE = dict(voxel_size=64.0, origin=(-32.0, -32.0, -32.0))  # one cell over every test mesh
MESHES = {"sphere": S.sphere, "archipelago": S.archipelago, "extras": S.smoothing_extras}
CASES = [(m, dict(voxel_size=k * L, origin=ORIGIN)) for m in MESHES for k in (1, 2, 4)] + [(m, WHOLE) for m in MESHES] + \
        [("cluster_extras", dict(voxel_size=S.EXTRAS_CELL, origin=(0.0, 0.0, 0.0)))]
IDS = [f"{m}-{kw['voxel_size']:.4g}" for m, kw in CASES]


def mesh_of(name):
    return S.cluster_extras() if name == "cluster_extras" else MESHES[name]()


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_symbols_are_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(native.lib(), s).argtypes
    assert native.lib().dqo_mesh_simplify_workspace_bytes.restype is ctypes.c_size_t
    assert native.lib().dqo_mesh_simplify.argtypes[6:10] == [ctypes.c_double] * 4  # voxel_size and the origin travel as doubles
    for cite in ("simplify_vertex_clustering", "SimplificationContraction::Average", "Departure", "ASCENDING", "2^21", "Not built: quadric-error"):
        assert cite in hdr, cite
    assert "mesh simplification" not in hdr  # (it left the "Not built" lists)
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_meshops.hip")).read()
    assert src.index("mesh_simp_scatter_kernel") < src.index('extern "C"')  # the entry points sit behind their launches
    assert "hipMemset" not in src and "atomicAdd((float" not in src and "atomicAdd_f" not in src
    body = src[src.index("DQO_API int dqo_mesh_simplify("):]
    body = body[:body.index("return DQO_OK;")]
    assert body.count("DQO_LAUNCH(") == 12 and "Twelve launches" in hdr and "twelve launches" in src


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = native.lib()
    assert lib.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert lib.dqo_abi_sizeof(13) == 0 and lib.dqo_abi_sizeof(16) == 0  # (no new struct: the entry takes plain arguments)


def test_workspace_bytes(native):
    f = native.lib().dqo_mesh_simplify_workspace_bytes
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -5), (1 << 28, 8), (8, 1 << 28)):
        assert f(*bad) == 0, bad
    assert f(1, 1) > 0 and f((1 << 28) - 1, (1 << 28) - 1) > 1 << 32  # (size_t: not cut at 32 bits)
    sizes = (1, 2, 255, 256, 257, 2048, 2049, 3132, 100000, 1 << 22)
    for a in sizes:
        row = [f(a, b) for b in sizes]
        col = [f(b, a) for b in sizes]
        assert row == sorted(row) and col == sorted(col), a  # they do not decrease as a capacity grows
        assert all(n % 256 == 0 for n in row)
    # two tables of at least twice the entries, a slot index a vertex and a face, a triple a face
    assert f(1000, 2000) >= 4 * (2 * 1000 + 2 * 2000 + 1000 + 2000 + 3 * 2000)


def _simplify(native, cap_v=100, cap_f=200, vertices=FAKE, colors=FAKE, faces=FAKE, counts=FAKE, voxel=0.1, origin=(0.0, 0.0, 0.0), out_v=FAKE + 64,
              out_c=FAKE + 128, out_f=FAKE + 192, out_cap_v=None, out_cap_f=None, header=FAKE + 320, ws=FAKE, ws_bytes=BIG):
    lib = native.lib()
    rc = lib.dqo_mesh_simplify(vertices, colors, faces, counts, cap_v, cap_f, voxel, *origin, out_v, out_c, out_f,
                               cap_v if out_cap_v is None else out_cap_v, cap_f if out_cap_f is None else out_cap_f, header, ws, ws_bytes, None)
    return rc, lib.dqo_last_error().decode()


def test_validation_before_launch(native):
    for caps in ((0, 8), (8, 0), (-3, 8), (1 << 28, 8), (8, 1 << 28)):
        rc, err = _simplify(native, cap_v=caps[0], cap_f=caps[1])
        assert rc == -1 and "bad capacity" in err and "2^28" in err, (caps, err)
    for name in ("vertices", "faces", "header"):
        rc, err = _simplify(native, **{name: None})
        assert rc == -1 and "null mesh buffer / header" in err, name
    for name in ("out_v", "out_c", "out_f"):
        rc, err = _simplify(native, **{name: None})
        assert rc == -1 and "null out mesh buffer" in err, name
    for kw in (dict(out_v=FAKE), dict(out_f=FAKE), dict(out_c=FAKE)):
        rc, err = _simplify(native, ws=None, **kw)
        assert rc == -1 and "must not be the input mesh" in err, kw
    rc, err = _simplify(native, header=FAKE + 256, counts=FAKE + 256, ws=None)  # the header would be cleared before the counts are read
    assert rc == -1 and "header must not be the input's counts" in err
    for kw in (dict(out_cap_v=99), dict(out_cap_f=199)):
        rc, err = _simplify(native, **kw)
        assert rc == -1 and "out capacity" in err and "below the input's" in err, kw
    for voxel in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        rc, err = _simplify(native, voxel=voxel)
        assert rc == -1 and "bad voxel_size" in err, voxel
    for axis in range(3):
        for bad in (float("nan"), float("inf"), -float("inf")):
            origin = [0.0, 0.0, 0.0]
            origin[axis] = bad
            rc, err = _simplify(native, origin=origin)
            assert rc == -1 and "bad origin" in err, origin
    need = native.lib().dqo_mesh_simplify_workspace_bytes(100, 200)
    rc, err = _simplify(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh simplify workspace too small ({need - 1} < {need})"
    rc, err = _simplify(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"mesh simplify workspace too small ({need} < {need})"
    rc, err = _simplify(native, colors=None, out_c=None, ws=None)  # no colours: no out colours needed; it gets as far as the workspace
    assert rc == -2
    rc, err = _simplify(native, counts=None, ws=None)  # no counts: the capacities
    assert rc == -2
    rc, err = _simplify(native, cap_v=0, ws=None, ws_bytes=0)  # argument errors come first, whatever the workspace
    assert rc == -1 and "bad capacity" in err


def test_python_surface(native):
    import torch
    import dqo_eval
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.mesh_simplify) == [("mesh", E), ("voxel_size", E), ("origin", (0.0, 0.0, 0.0)), ("out", None), ("workspace_buffer", None)]
    assert dqo_eval.MESH_SIMPLIFY_HEADER == S.HEADER and len(S.HEADER) == 8
    assert P(F.FusedMapper.make_simplified_mesh) == [("self", E), ("frames", E), ("volume", E), ("cap_vertices", E), ("cap_faces", E), ("simplify_voxel", E),
                                                     ("simplify_origin", None), ("depth_trunc", 30.0), ("min_component_faces", 0), ("largest_only", False),
                                                     ("smooth_iter", 0), ("smooth_lambda", 0.5), ("smooth_mu", None), ("normals", True)]
    # make_clean_mesh keeps its parameters: make_simplified_mesh's are those plus the two of the grid
    assert [n for n, _ in P(F.FusedMapper.make_simplified_mesh) if not n.startswith("simplify_")] == [n for n, _ in P(F.FusedMapper.make_clean_mesh)]
    assert "Not built: mesh simplification" not in F.FusedMapper.make_mesh.__doc__
    mesh = dict(vertices=torch.zeros((4, 3)), colors=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.mesh_simplify(mesh, 0.1)
    mesh["header"] = torch.tensor([3, 1, 2, 1, 0, 0, 1, 0], dtype=torch.int32)
    mesh["header_names"] = dqo_eval.MESH_SIMPLIFY_HEADER
    assert dqo_eval.mesh_counts(mesh) == dict(vertices=3, faces=1, clusters=2, vertices_outside=1, faces_bad_index=0, faces_outside=0,
                                              faces_collapsed=1, faces_duplicate=0)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def test_the_counts_worked_out_with_the_rule():
    """The sphere (3132 vertices, 6260 faces), the grid at its volume's origin: clusters, faces kept, collapsed, duplicates, the most
    members.  smoothing_extras() at L: 777 kept, 1361 collapsed, 1286 duplicates; its 490 clusters and its 4 vertices outside the
    grid (isolated ones below the origin) are the 494 cells that its vertices occupy.  The archipelago: 877 formed, 840 written."""
    s = S.sphere()
    for k, want in ((1, (819, 1634, 4626, 0, 8)), (2, (238, 474, 5786, 0, 34)), (4, (59, 114, 6146, 0, 117))):
        r = S.simplify(s["vertices"], s["colors"], s["faces"], k * L, ORIGIN)
        h = r["header"].tolist()
        assert (h[2], h[1], h[6], h[7], int(r["members"].max())) == want and h[0] == h[2] and h[3] == h[4] == h[5] == 0, (k, h)
    e = S.smoothing_extras()
    h = S.simplify(e["vertices"], e["colors"], e["faces"], L, ORIGIN)["header"].tolist()
    assert (h[1], h[6], h[7]) == (777, 1361, 1286) and h[2] + h[3] == 494 and h[3] == 4, h
    a = S.archipelago()
    h = S.simplify(a["vertices"], a["colors"], a["faces"], L, ORIGIN)["header"].tolist()
    assert (h[2], h[0], h[4]) == (877, 840, 2), h


def test_cluster_extras_is_what_it_says():
    m = S.cluster_extras()
    V, F = len(m["vertices"]), len(m["faces"])
    assert 6500 < V < 7500 and 6500 < F < 7500
    r = S.simplify(m["vertices"], m["colors"], m["faces"], S.EXTRAS_CELL)
    h = r["header"].tolist()
    groups = len(S.GROUPS)
    # a group and its two anchors are three written clusters; the unreferenced vertex forms a cluster that is not written
    assert h == [3 * groups, groups, 3 * groups + 1, 4, 2, 4, 0, sum(S.GROUPS) - groups], h
    assert sorted(r["members"].tolist()) == [1] * (2 * groups + 1) + sorted(S.GROUPS)[1:]
    assert S.GROUPS == (1, 2, 32, 33, 2048, 2049, 2600)  # both sides of the tidy kernel's 32 and 2048
    cell, inside = S.cells(m["vertices"], S.EXTRAS_CELL, (0.0, 0.0, 0.0))
    for g in m["groups"]:
        assert inside[g].all() and (cell[g] == cell[g[0]]).all() and (np.diff(g) > 0).all()
    assert np.isnan(m["vertices"]).any(1).sum() == 1 and (~inside).sum() == 4 and (cell[inside] >= 0).all()


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_the_two_restatements_agree_and_the_invariants_hold(name, kw):
    m = mesh_of(name)
    V, F = len(m["vertices"]), len(m["faces"])
    r = S.simplify(m["vertices"], m["colors"], m["faces"], **kw)
    d = S.simplify(m["vertices"], m["colors"], m["faces"], group=S.group_by_dict, **kw)
    for k in ("vertices", "colors", "faces", "header", "rep", "state"):
        assert r[k].dtype == d[k].dtype and r[k].tobytes() == d[k].tobytes(), k
    h = r["header"].tolist()
    nv, nf = h[0], h[1]
    assert r["vertices"].shape == (nv, 3) and r["colors"].shape == (nv, 3) and r["faces"].shape == (nf, 3)
    assert r["vertices"].dtype == np.float32 and r["faces"].dtype == np.int32
    f = r["faces"].astype(np.int64)
    if nf:
        assert f.min() >= 0 and f.max() < nv
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()  # no kept face repeats an index
        assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()  # rotated: the smallest first
        assert len(np.unique(S.rotate(f), axis=0)) == nf  # no two kept faces are equal after rotation
    assert len(np.unique(f)) == nv  # every written vertex is named by a kept face
    valid = int(S.valid_faces(V, m["faces"]).sum())
    assert valid == h[1] + h[5] + h[6] + h[7] and F - valid == h[4]
    assert h[0] <= h[2] <= V - h[3]
    if kw is WHOLE:
        assert h[:4] == [0, 0, 1, int(np.isnan(m["vertices"]).any(1).sum())] and h[6] == valid - h[5] and h[7] == 0  # everything collapses
    # a cluster of one member is its vertex, bit for bit
    written = np.zeros(V, bool)
    written[r["rep"][np.asarray(m["faces"], np.int64)[r["state"] >= 3].ravel()]] = True
    reps = np.nonzero(written)[0]
    assert len(reps) == nv
    size = np.bincount(r["rep"][r["rep"] >= 0], minlength=V)[reps]
    assert np.array_equal(size, r["members"])
    one = size == 1
    assert r["vertices"][one].tobytes() == m["vertices"][reps[one]].tobytes() and r["colors"][one].tobytes() == m["colors"][reps[one]].tobytes()
    # the average, one cluster by hand in a Python loop over ascending ids
    if nv:
        k = int(np.argmax(size))
        total = np.zeros(3)
        for v in np.nonzero(r["rep"] == reps[k])[0]:
            total = total + m["vertices"][v].astype(np.float64)
        want = m["vertices"][reps[k]] if size[k] == 1 else (total / np.float64(size[k])).astype(np.float32)
        assert r["vertices"][k].tobytes() == want.tobytes()
        lo, hi = m["vertices"][r["rep"] == reps[k]].min(0), m["vertices"][r["rep"] == reps[k]].max(0)
        assert (r["vertices"][k] >= lo).all() and (r["vertices"][k] <= hi).all()


def test_a_mesh_with_every_vertex_in_a_cell_of_its_own_comes_back():
    """The referenced vertices bit for bit and in order, the faces rotated: on the archipelago with a cell far below its shortest
    edge (the test asserts that no two in-grid vertices share a cell)."""
    a = S.archipelago()
    V = len(a["vertices"])
    kw = dict(voxel_size=2.0 ** -17, origin=(-1.0, -1.0, -1.0))
    cell, inside = S.cells(a["vertices"], **kw)
    assert inside.all() and len(np.unique(cell, axis=0)) == V
    r = S.simplify(a["vertices"], a["colors"], a["faces"], **kw)
    ok = S.valid_faces(V, a["faces"])
    fv = a["faces"][ok].astype(np.int64)
    proper = (fv[:, 0] != fv[:, 1]) & (fv[:, 1] != fv[:, 2]) & (fv[:, 0] != fv[:, 2])  # (the strip's repeated-index face collapses)
    used = np.zeros(V, bool)
    used[fv[proper].ravel()] = True
    h = r["header"].tolist()
    assert h == [int(used.sum()), int(proper.sum()), V, 0, 2, 0, int((~proper).sum()), 0] and h[6] == 1
    assert r["vertices"].tobytes() == a["vertices"][used].tobytes() and r["colors"].tobytes() == a["colors"][used].tobytes()
    remap = np.cumsum(used) - used
    assert np.array_equal(r["faces"], S.rotate(remap[fv[proper]]).astype(np.int32))
