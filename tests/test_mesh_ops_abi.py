"""CPU-side checks of the mesh clean-up entry points (dqo_mesh_components, dqo_mesh_smooth, dqo_mesh_normals and their workspace
queries; csrc/map_meshops.hip): the symbols are declared, exported and bound, the size queries behave, every argument error is
reported before anything is launched (-1 for bad arguments, -2 for a short workspace; no GPU here), the Python surface is the
documented one, and dqo_ply.write_mesh_ply_normals writes what read_mesh_ply reads."""
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("components", "smooth", "normals")
NEW = tuple(f"dqo_mesh_{n}_workspace_bytes" for n in OPS) + tuple(f"dqo_mesh_{n}" for n in OPS)
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
BIG = 1 << 40


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
        if s.endswith("_bytes"):
            assert getattr(native.lib(), s).restype is ctypes.c_size_t
    for cite in ("configs/Cube_Diorama_base.yaml:45-46", "cluster_connected_triangles", "remove_triangles_by_mask", "remove_unreferenced_vertices",
                 "filter_smooth_laplacian", "filter_smooth_taubin", "compute_vertex_normals", "pinch"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert " map_meshops.hip" in mk and "../build/map_meshops.o: HIPFLAGS += -ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_meshops.hip")).read()
    assert src.index("__global__") < src.index('extern "C"')  # the entry points sit beside their launches, behind them
    assert "hipMemset" not in src and "__launch_bounds__(256)" in src
    assert "atomicAdd((float" not in src and "atomicAdd_f" not in src  # integer atomics only


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    L = native.lib()
    assert L.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert L.dqo_abi_sizeof(13) == 0 and L.dqo_abi_sizeof(16) == 0  # (no new struct: the entries take plain arguments)


@pytest.mark.parametrize("op", OPS)
def test_workspace_bytes(native, op):
    f = getattr(native.lib(), f"dqo_mesh_{op}_workspace_bytes")
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -5), (1 << 28, 8), (8, 1 << 28)):
        assert f(*bad) == 0, bad
    assert f(1, 1) > 0 and f((1 << 28) - 1, (1 << 28) - 1) > 0
    sizes = (1, 2, 255, 256, 257, 2048, 2049, 3132, 100000, 1 << 22)
    for a in sizes:
        row = [f(a, b) for b in sizes]
        col = [f(b, a) for b in sizes]
        assert row == sorted(row) and col == sorted(col), a  # they do not decrease as a capacity grows
        assert all(n % 256 == 0 for n in row)


def _components(native, cap_v=100, cap_f=200, vertices=FAKE, colors=FAKE, faces=FAKE, counts=FAKE, min_faces=0, out_v=FAKE + 64, out_c=FAKE + 128,
                out_f=FAKE + 192, out_cap_v=None, out_cap_f=None, labels=None, header=FAKE + 320, ws=FAKE, ws_bytes=BIG):
    L = native.lib()
    rc = L.dqo_mesh_components(vertices, colors, faces, counts, cap_v, cap_f, min_faces, 0, out_v, out_c, out_f,
                               cap_v if out_cap_v is None else out_cap_v, cap_f if out_cap_f is None else out_cap_f, labels, header, ws, ws_bytes, None)
    return rc, L.dqo_last_error().decode()


def _smooth(native, cap_v=100, cap_f=200, vertices=FAKE, colors=FAKE, faces=FAKE, counts=FAKE, iterations=1, lam=0.5, mu=0.0, scope=2, ws=FAKE,
            ws_bytes=BIG):
    L = native.lib()
    rc = L.dqo_mesh_smooth(vertices, colors, faces, counts, cap_v, cap_f, iterations, lam, mu, scope, ws, ws_bytes, None)
    return rc, L.dqo_last_error().decode()


def _normals(native, cap_v=100, cap_f=200, vertices=FAKE, faces=FAKE, counts=FAKE, normals=FAKE, ws=FAKE, ws_bytes=BIG):
    L = native.lib()
    rc = L.dqo_mesh_normals(vertices, faces, counts, cap_v, cap_f, normals, ws, ws_bytes, None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("call", [_components, _smooth, _normals], ids=OPS)
def test_mesh_validation_before_launch(native, call):
    for caps in ((0, 8), (8, 0), (-3, 8), (1 << 28, 8), (8, 1 << 28)):
        rc, err = call(native, cap_v=caps[0], cap_f=caps[1])
        assert rc == -1 and "bad capacity" in err and "2^28" in err, (caps, err)
    for name in ("vertices", "faces"):
        rc, err = call(native, **{name: None})
        assert rc == -1 and "null mesh buffer" in err, name
    op = call.__name__[1:]
    need = getattr(native.lib(), f"dqo_mesh_{op}_workspace_bytes")(100, 200)
    rc, err = call(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"mesh {op} workspace too small ({need - 1} < {need})"
    rc, err = call(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"mesh {op} workspace too small ({need} < {need})"
    # argument errors come first, whatever the workspace
    rc, err = call(native, cap_v=0, ws=None, ws_bytes=0)
    assert rc == -1 and "bad capacity" in err


def test_components_validation_before_launch(native):
    rc, err = _components(native, min_faces=-1)
    assert rc == -1 and "bad min_faces" in err
    rc, err = _components(native, header=None)
    assert rc == -1 and "null mesh buffer / header" in err
    for kw in (dict(out_cap_v=99), dict(out_cap_f=199)):
        rc, err = _components(native, **kw)
        assert rc == -1 and "out capacity" in err and "below the input's" in err, kw
    for name in ("out_v", "out_c", "out_f"):
        rc, err = _components(native, **{name: None})
        assert rc == -1 and "null out mesh buffer" in err, name
    rc, err = _components(native, colors=None, out_c=None, ws=None)  # no colours: no out colours needed; it gets as far as the workspace
    assert rc == -2
    for kw in (dict(out_v=FAKE), dict(out_f=FAKE), dict(out_c=FAKE)):
        rc, err = _components(native, ws=None, **kw)
        assert rc == -1 and "must not be the input mesh" in err, kw
    rc, err = _components(native, header=FAKE + 256, counts=FAKE + 256, ws=None)  # the header would be cleared before the counts are read
    assert rc == -1 and "header must not be the input's counts" in err


def test_smooth_validation_before_launch(native):
    rc, err = _smooth(native, iterations=-1)
    assert rc == -1 and "bad iterations" in err
    for kw in (dict(lam=float("nan")), dict(lam=float("inf")), dict(mu=float("nan")), dict(mu=-float("inf"))):
        rc, err = _smooth(native, **kw)
        assert rc == -1 and "bad lambda / mu" in err, kw
    for scope in (-1, 3):
        rc, err = _smooth(native, scope=scope)
        assert rc == -1 and "bad scope" in err
    for scope in (1, 2):
        rc, err = _smooth(native, colors=None, scope=scope)
        assert rc == -1 and "null colors" in err
    rc, err = _smooth(native, colors=None, scope=0, ws=None)  # positions alone need no colours
    assert rc == -2
    need = native.lib().dqo_mesh_smooth_workspace_bytes(100, 200)
    assert _smooth(native, iterations=0, ws_bytes=need)[0] == 0  # nothing to do: nothing is launched (no GPU here)
    assert _smooth(native, iterations=0, ws_bytes=need - 1)[0] == -2


def test_normals_validation_before_launch(native):
    rc, err = _normals(native, normals=None)
    assert rc == -1 and "null mesh buffer / normals" in err


def test_python_surface(native):
    import torch
    import dqo_eval
    import dqo_ply
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_eval.mesh_components) == [("mesh", E), ("min_faces", 0), ("largest_only", False), ("out", None), ("want_labels", False),
                                           ("workspace_buffer", None)]
    assert P(dqo_eval.mesh_smooth) == [("mesh", E), ("iterations", E), ("lam", 0.5), ("mu", None), ("scope", "all"), ("workspace_buffer", None)]
    assert P(dqo_eval.mesh_normals) == [("mesh", E), ("out", None), ("workspace_buffer", None)]
    assert P(dqo_eval.mesh_counts) == [("mesh", E)]
    assert dqo_eval.MESHOPS_HEADER == ("vertices", "faces", "components", "components_kept", "faces_bad_index", "largest_component_faces",
                                       "vertices_removed", "faces_removed")
    assert P(F.FusedMapper.make_clean_mesh) == [("self", E), ("frames", E), ("volume", E), ("cap_vertices", E), ("cap_faces", E), ("depth_trunc", 30.0),
                                                ("min_component_faces", 0), ("largest_only", False), ("smooth_iter", 0), ("smooth_lambda", 0.5),
                                                ("smooth_mu", None), ("normals", True)]
    assert list(inspect.signature(dqo_ply.write_mesh_ply_normals).parameters) == ["path", "vertices", "faces", "normals", "colors"]
    assert "Not built: Laplacian smoothing" not in F.FusedMapper.make_mesh.__doc__
    # what must not change
    assert list(inspect.signature(F.FusedMapper.make_mesh).parameters) == ["self", "frames", "volume", "depth_trunc"]
    assert list(inspect.signature(dqo_ply.write_mesh_ply).parameters) == ["path", "vertices", "faces", "colors"]
    # CPU tensors are refused
    mesh = dict(vertices=torch.zeros((4, 3)), colors=torch.zeros((4, 3)), faces=torch.zeros((2, 3), dtype=torch.int32))
    for call in (lambda: dqo_eval.mesh_components(mesh), lambda: dqo_eval.mesh_smooth(mesh, 1), lambda: dqo_eval.mesh_normals(mesh)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert dqo_eval.mesh_counts(mesh) == dict(vertices=4, faces=2)  # (no header: the capacities)
    mesh["header"] = torch.tensor([3, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
    assert dqo_eval.mesh_counts(mesh) == dict(vertices=3, faces=1, vertices_dropped=0, faces_dropped=0)
    mesh["header_names"] = dqo_eval.MESHOPS_HEADER
    assert dqo_eval.mesh_counts(mesh)["components_kept"] == 0 and len(dqo_eval.mesh_counts(mesh)) == 8


def test_write_mesh_ply_normals_round_trip(tmp_path):
    import dqo_ply
    rng = np.random.default_rng(6)
    v = rng.normal(size=(41, 3)).astype(np.float32)
    v[3] = [np.float32(1e-40), -0.0, np.float32(3.4e38)]  # a denormal, -0 and a huge value keep their bits
    n = rng.normal(size=(41, 3)).astype(np.float32)
    n[5] = [0.0, 0.0, 1.0]
    f = rng.integers(0, 41, size=(77, 3)).astype(np.int32)
    c = rng.uniform(-0.2, 1.2, size=(41, 3)).astype(np.float32)
    c[0] = [0.5, 0.49803922, 1.0 / 510.0 + 1e-4]
    for colors, name in ((None, "plain.ply"), (c, "coloured.ply")):
        path = str(tmp_path / name)
        assert dqo_ply.write_mesh_ply_normals(path, v, f, n, colors) == (41, 77)
        head = open(path, "rb").read(600).split(b"end_header\n")[0].decode("ascii").split("\n")
        props = [h.split()[-1] for h in head if h.startswith("property") and "list" not in h]
        assert props == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors is not None else [])
        assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in head
        stride = 24 + (3 if colors is not None else 0)
        assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 41 * stride + 77 * 13
        v2, f2 = dqo_ply.read_mesh_ply(path)
        assert v2.tobytes() == v.tobytes() and np.array_equal(f2, f)
    raw = open(str(tmp_path / "coloured.ply"), "rb").read()
    body = raw[raw.index(b"end_header\n") + 11:]
    vt = np.frombuffer(body[:41 * 27], dtype=np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))]))
    assert vt["p"].tobytes() == v.tobytes() and vt["n"].tobytes() == n.tobytes()
    # the colour bytes are write_mesh_ply's
    dqo_ply.write_mesh_ply(str(tmp_path / "ref.ply"), v, f, c)
    ref = open(str(tmp_path / "ref.ply"), "rb").read()
    rt = np.frombuffer(ref[ref.index(b"end_header\n") + 11:][:41 * 15], dtype=np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]))
    assert np.array_equal(vt["c"], rt["c"]) and vt["c"][0].tolist() == [128, 127, 1]
    import torch
    path = str(tmp_path / "t.ply")
    dqo_ply.write_mesh_ply_normals(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c))
    assert open(path, "rb").read() == raw
    assert dqo_ply.write_mesh_ply_normals(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)) == (0, 0)
    with pytest.raises(ValueError):
        dqo_ply.write_mesh_ply_normals(path, v, f, n[:5])
    with pytest.raises(ValueError):
        dqo_ply.write_mesh_ply_normals(path, v, f, n, c[:5])
