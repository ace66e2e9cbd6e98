"""CPU-side checks of the TSDF entry points (dqo_tsdf_workspace_bytes, dqo_tsdf_clear, dqo_tsdf_integrate, dqo_tsdf_extract;
csrc/map_tsdf.hip): the symbols are declared, exported and bound, the size query behaves, every argument error is reported before
anything is launched (-1 for bad arguments, -2 for a short workspace; no GPU here), the Python surface is the documented one, and
dqo_ply.write_mesh_ply writes what read_mesh_ply reads."""
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_tsdf_workspace_bytes", "dqo_tsdf_clear", "dqo_tsdf_integrate", "dqo_tsdf_extract")
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
    assert native.lib().dqo_tsdf_workspace_bytes.restype is ctypes.c_size_t
    for cite in ("SLAM/eval.py:299, 316-343", "make_mesh.py", "configs/Cube_Diorama_base.yaml:45-46", "UniformTSDFVolume", "Kuhn"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert " map_tsdf.hip" in mk and "../build/map_tsdf.o: HIPFLAGS += -ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_tsdf.hip")).read()
    assert src.index("__global__") < src.index('extern "C"')  # the entry points sit beside their launches, behind them
    assert "hipMemset" not in src and "atomicAdd(" not in src  # cleared by a launch; no atomics of its own (the tickets are dqo_reduce.h's)


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    L = native.lib()
    assert L.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert L.dqo_abi_sizeof(13) == 0 and L.dqo_abi_sizeof(16) == 0  # (no new struct: the entries take plain arguments)


def test_workspace_bytes(native):
    f = native.lib().dqo_tsdf_workspace_bytes
    head = f(2, 2, 2) - (256 + 256 + 3 * 256 + 256)  # one block of 8 points: every array is one 256-byte line
    assert head > 0 and head % 256 == 0
    for dims in ((40, 36, 28), (24, 24, 24), (256, 256, 256), (2, 2, 3)):
        n = dims[0] * dims[1] * dims[2]
        nb = (n + 2047) // 2048
        up = lambda b: (b + 255) // 256 * 256
        assert f(*dims) == head + up(4 * nb) + up(8 * nb) + 3 * up(n) + up(2 * n), dims  # 5 bytes a voxel, 12 a span of 2048
    assert f(1, 8, 8) == 0 and f(8, 0, 8) == 0 and f(8, 8, -2) == 0
    assert f(1024, 1024, 256) == 0 and f(1024, 1024, 255) > 0 and f(1 << 20, 1 << 20, 1 << 20) == 0  # nx ny nz < 2^28


def _clear(native, dims=(8, 8, 8), tsdf=FAKE, weight=FAKE, color=FAKE, header=FAKE):
    L = native.lib()
    return L.dqo_tsdf_clear(*dims, tsdf, weight, color, header, None), L.dqo_last_error().decode()


def _integrate(native, dims=(8, 8, 8), L_=0.1, trunc=0.3, tsdf=FAKE, weight=FAKE, color=FAKE, header=FAKE, W=64, H=48, depth=FAKE, image=FAKE,
               w2c=FAKE):
    L = native.lib()
    rc = L.dqo_tsdf_integrate(*dims, 0.0, 0.0, 0.0, L_, trunc, tsdf, weight, color, header, W, H, depth, image, 40.0, 40.0, 31.5, 23.5, w2c, 30.0,
                              None, None)
    return rc, L.dqo_last_error().decode()


def _extract(native, dims=(8, 8, 8), tsdf=FAKE, weight=FAKE, color=FAKE, vertices=FAKE, vertex_color=FAKE, faces=FAKE, cap_v=10, cap_f=10,
             header=FAKE, ws=FAKE, ws_bytes=BIG):
    L = native.lib()
    rc = L.dqo_tsdf_extract(*dims, 0.0, 0.0, 0.0, 0.1, tsdf, weight, color, vertices, vertex_color, faces, cap_v, cap_f, header, ws, ws_bytes, None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("call", [_clear, _integrate, _extract], ids=["clear", "integrate", "extract"])
def test_volume_validation_before_launch(native, call):
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8)):
        rc, err = call(native, dims=dims)
        assert rc == -1 and "bad dims" in err and "every side is at least 2" in err, (dims, err)
    for dims in ((1024, 1024, 256), (1 << 27, 2, 2), (1 << 20, 1 << 20, 1 << 20)):
        rc, err = call(native, dims=dims)
        assert rc == -1 and "too many voxels" in err and "2^28" in err, (dims, err)
    for name in ("tsdf", "weight", "color", "header"):
        rc, err = call(native, **{name: None})
        assert rc == -1 and "null volume buffer / header" in err, name


def test_integrate_validation_before_launch(native):
    for kw in (dict(L_=0.0), dict(L_=-1.0), dict(trunc=0.0), dict(L_=float("nan"))):
        rc, err = _integrate(native, **kw)
        assert rc == -1 and "bad voxel_length / sdf_trunc" in err, kw
    for kw in (dict(W=0), dict(H=-1), dict(W=1 << 16, H=1 << 15)):
        rc, err = _integrate(native, **kw)
        assert rc == -1 and "bad image size" in err, kw
    for name in ("depth", "image", "w2c"):
        rc, err = _integrate(native, **{name: None})
        assert rc == -1 and "null depth / color / w2c" in err, name


def test_extract_validation_before_launch(native):
    need = native.lib().dqo_tsdf_workspace_bytes(8, 8, 8)
    for kw in (dict(cap_v=-1), dict(cap_f=-1)):
        rc, err = _extract(native, **kw)
        assert rc == -1 and "bad capacity" in err, kw
    for name in ("vertices", "vertex_color", "faces"):
        rc, err = _extract(native, **{name: None})
        assert rc == -1 and "null mesh buffer" in err, name
    rc, err = _extract(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"tsdf workspace too small ({need - 1} < {need})"
    rc, err = _extract(native, ws=None, ws_bytes=need)
    assert rc == -2 and err == f"tsdf workspace too small ({need} < {need})"
    # argument errors come first, whatever the workspace
    rc, err = _extract(native, cap_v=-1, ws=None, ws_bytes=0)
    assert rc == -1 and "bad capacity" in err


def test_python_surface(native):
    import torch
    import dqo_eval
    import dqo_ply
    from dqo_harness import fused_mapping as F
    assert list(inspect.signature(dqo_eval.TsdfVolume.__init__).parameters) == ["self", "origin", "voxel_length", "dims", "sdf_trunc", "device"]
    sig = inspect.signature(dqo_eval.TsdfVolume.integrate)
    assert list(sig.parameters) == ["self", "depth", "color", "K", "w2c", "depth_trunc", "render_header"]
    assert sig.parameters["depth_trunc"].default == 30.0 and sig.parameters["render_header"].default is None
    sig = inspect.signature(dqo_eval.TsdfVolume.extract)
    assert list(sig.parameters) == ["self", "cap_vertices", "cap_faces", "out"] and sig.parameters["out"].default is None
    assert callable(dqo_eval.TsdfVolume.clear) and callable(dqo_eval.TsdfVolume.counts)
    assert dqo_eval.TSDF_HEADER[:6] == ("vertices", "faces", "vertices_dropped", "faces_dropped", "frames", "frames_skipped")
    sig = inspect.signature(F.FusedMapper.make_mesh)
    assert list(sig.parameters) == ["self", "frames", "volume", "depth_trunc"] and sig.parameters["depth_trunc"].default == 30.0
    assert list(inspect.signature(dqo_ply.write_mesh_ply).parameters) == ["path", "vertices", "faces", "colors"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.TsdfVolume((0, 0, 0), 0.1, (8, 8, 8), 0.3, torch.device("cpu"))


def test_write_mesh_ply_round_trip(tmp_path):
    import dqo_ply
    rng = np.random.default_rng(5)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    v[3] = [np.float32(1e-40), -0.0, np.float32(3.4e38)]  # a denormal, -0 and a huge value keep their bits
    f = rng.integers(0, 37, size=(91, 3)).astype(np.int32)
    c = rng.uniform(-0.2, 1.2, size=(37, 3)).astype(np.float32)
    c[0] = [0.5, 0.49803922, 1.0 / 510.0 + 1e-4]  # 127.5 rounds to even (128), 127.0000011 to 127, just above 0.5 to 1
    for colors, name in ((None, "plain.ply"), (c, "coloured.ply")):
        path = str(tmp_path / name)
        assert dqo_ply.write_mesh_ply(path, v, f, colors) == (37, 91)
        head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in head
        assert ("property uchar red" in head) == (colors is not None)
        assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 37 * (12 + (3 if colors is not None else 0)) + 91 * 13
        v2, f2 = dqo_ply.read_mesh_ply(path)
        assert v2.dtype == np.float32 and f2.dtype == np.int32
        assert v2.tobytes() == v.tobytes() and np.array_equal(f2, f)
    raw = open(str(tmp_path / "coloured.ply"), "rb").read()
    body = raw[raw.index(b"end_header\n") + 11:]
    vt = np.frombuffer(body[:37 * 15], dtype=np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]))
    want = np.rint(255.0 * np.clip(c.astype(np.float64), 0.0, 1.0)).astype(np.uint8)
    assert np.array_equal(vt["c"], want) and vt["c"][0].tolist() == [128, 127, 1] and vt["c"].min() == 0 and vt["c"].max() == 255
    # tensors are taken too, an empty mesh is a valid file, bad shapes are refused
    import torch
    path = str(tmp_path / "t.ply")
    dqo_ply.write_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    assert open(path, "rb").read() == raw
    assert dqo_ply.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) == (0, 0)
    v0, f0 = dqo_ply.read_mesh_ply(path)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    with pytest.raises(ValueError):
        dqo_ply.write_mesh_ply(path, v[:, :2], f)
    with pytest.raises(ValueError):
        dqo_ply.write_mesh_ply(path, v, f, c[:5])
