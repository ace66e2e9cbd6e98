"""CPU-side checks of the ground-truth mesh sampler (dqo_mesh_sample, include/dqo_raster.h; dqo_eval.sample_surface; dqo_ply.read_mesh_ply):
the rule itself (tests/mesh_oracle.py) samples a surface as trimesh.sample.sample_surface does — faces in proportion to their area, points
uniform inside a face — the mesh reader accepts and rejects what it says, both symbols are declared and exported, and every argument error
is reported before anything is launched (no GPU here)."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest

import mesh_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_mesh_sample_workspace_bytes", "dqo_mesh_sample")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch


def normal_mesh(seed, V, F, zero=()):
    """F faces over V normal-distributed vertices (float32 [V,3], int32 [F,3]); the faces `zero` names repeat a vertex: area exactly 0."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (V, 3)).astype(np.float32)
    f = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32) if F <= 4096 else _distinct_triples(rng, V, F)
    for z in zero:
        f[z, 1] = f[z, 0]
    return v, f


def _distinct_triples(rng, V, F):
    a = rng.integers(0, V, F)
    b = (a + rng.integers(1, V // 2, F)) % V
    c = (b + rng.integers(1, V // 2 - 1, F)) % V  # a != b, b != c; c == a only if the two steps add up to V: V // 2 + V // 2 - 1 < V
    return np.stack([a, b, c], 1).astype(np.int32)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 5])
def test_faces_are_drawn_in_proportion_to_their_area(seed):
    from scipy.stats import chi2
    v, f = normal_mesh(3, 200, 64, zero=(0, 17, 63))
    n = 1 << 18
    o = mo.sample_surface_oracle(v, f, n, seed)
    A = o["A"]
    live = A > 0
    assert live.sum() == 61 and o["header"][:4] == [n, 64, 0, 3]
    counts = np.bincount(o["face_index"], minlength=64)
    assert (counts[~live] == 0).all()
    expect = n * A[live] / A[live].sum()
    assert expect.min() > 5  # (the chi-square approximation's usual premise)
    stat = float((((counts[live] - expect) ** 2) / expect).sum())
    dof = int(live.sum()) - 1
    bound = float(chi2.ppf(1 - 1e-6, dof))
    print(f"seed {seed}: chi-square {stat:.1f} at {dof} degrees of freedom, bound {bound:.1f}")
    assert stat <= bound
    # the folded draws: u, v >= 0, u + v <= 1, both with mean 1/3 (variance 1/18)
    u, w = o["u"], o["v"]
    assert (u >= 0).all() and (w >= 0).all() and (u + w <= 1.0).all()
    se = np.sqrt(1 / 18 / n)
    assert abs(u.mean() - 1 / 3) < 5 * se and abs(w.mean() - 1 / 3) < 5 * se


def test_points_are_uniform_inside_a_face():
    v = np.float32([[0.25, -1.0, 2.0], [3.0, 0.5, 1.0], [-1.0, 2.0, 4.5]])
    f = np.int32([[0, 1, 2]])
    n = 1 << 16
    o = mo.sample_surface_oracle(v, f, n, seed=9)
    p = o["points"].astype(np.float64)
    a, b, c = v.astype(np.float64)
    e1, e2 = b - a, c - a
    # p = a + u e1 + v e2 with (u, v) uniform on the unit triangle: E u = E v = 1/3, Var u = Var v = 1/18, Cov(u, v) = -1/36
    var = e1 * e1 / 18 + e2 * e2 / 18 - 2 * e1 * e2 / 36
    se = np.sqrt(var / n)
    centroid = (a + b + c) / 3
    print("mean - centroid in standard errors", (p.mean(axis=0) - centroid) / se)
    assert (np.abs(p.mean(axis=0) - centroid) < 5 * se).all()
    # the second moments too: the sample variance per axis within 5 % of the triangle's
    assert (np.abs(p.var(axis=0) / var - 1) < 0.05).all()
    # every point lies in the triangle's plane and inside it (barycentric coordinates from the float32 points, to float32 accuracy)
    M = np.stack([e1, e2, np.cross(e1, e2)], 1)
    bary = np.linalg.solve(M, (p - a).T).T
    assert (bary[:, :2] > -1e-6).all() and (bary[:, 0] + bary[:, 1] < 1 + 1e-6).all() and (np.abs(bary[:, 2]) < 1e-6).all()
    assert (o["face_index"] == 0).all() and o["keep"].all()


def test_zero_area_faces_get_no_sample():
    zero = (0, 1, 30, 31, 32, 33, 62, 63)  # at the start, in a run, at the end
    v, f = normal_mesh(4, 100, 64, zero=zero)
    o = mo.sample_surface_oracle(v, f, 1 << 14, seed=1)
    assert o["header"][3] == len(zero) and (o["q"][list(zero)] == 0).all() and (np.delete(o["q"], zero) > 0).all()
    counts = np.bincount(o["face_index"], minlength=64)
    assert (counts[list(zero)] == 0).all() and (np.delete(counts, zero) > 0).all()
    # a face with an index out of range takes no part and its vertices are never read; one of NaN coordinates counts as degenerate
    f2 = f.copy()
    f2[5, 2], f2[6, 0] = 100, -1
    v2 = v.copy()
    v2[f[40, 0]] = np.nan
    o2 = mo.sample_surface_oracle(v2, f2, 1 << 12, seed=1)
    nan_faces = (f2 == f[40, 0]).any(axis=1) & ~np.isin(np.arange(64), (5, 6))
    assert o2["header"][2] == 2 and o2["header"][3] == int((nan_faces | np.isin(np.arange(64), zero)).sum())
    assert np.isfinite(o2["points"]).all() and not np.isin(o2["face_index"], [5, 6]).any() and not nan_faces[o2["face_index"]].any()
    # no area at all: nothing is drawn
    o3 = mo.sample_surface_oracle(v, np.int32([[0, 0, 1], [2, 3, 3]]), 10, seed=1)
    assert o3["header"] == [0, 2, 0, 2, 61 - 2, 0, 0, 0] and o3["points"] is None and not o3["keep"].any()


def test_the_total_in_quanta_stays_below_2_to_61():
    F = (1 << 25) - 1
    for A in (1.0, 0.5, np.nextafter(1.0, 0.0), np.nextafter(0.5, 1.0), 3.1e-7, 7.7e11):
        e, m = mo.quantum_exponent(A, F)
        q = int(np.floor(np.ldexp(np.float64(A), e)))
        assert 0.5 <= m < 1 and (1 << 35) <= q < (1 << 36) and q * F < (1 << 61), (A, e, q)
    # and at small F the largest face alone stays below 2^61 / F
    for F in (1, 2, 3, 255, 256):
        e, _ = mo.quantum_exponent(1.75, F)
        q = int(np.floor(np.ldexp(np.float64(1.75), e)))
        assert q * F < (1 << 61) and q >= (1 << (60 - F.bit_length()))


def test_the_key_rule_is_the_growth_samplers():
    import sample_oracle as so
    i = np.arange(1000)
    for seed in (0, 7, (5 << 32) | 11):
        for d in range(4, 8):
            assert (mo.keys(seed, d, i) == so.sample_keys(seed, d, i)).all()


# ---- the mesh reader ------------------------------------------------------------------------------------------------------------------------
_CODES = {"uchar": "B", "uint8": "B", "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d",
          "short": "h"}


def write_mesh(path, v, faces, fmt="binary_little_endian", count_type="uchar", index_type="int", extras=(), coord_type="float",
               index_name="vertex_indices", face_extra=None, elements=("vertex", "face"), cut=0):
    """A mesh file.  faces: a list of index tuples (any sizes); extras: (type, name, value) scalar vertex properties placed between the
    coordinates (after x, after y, then after z); cut: bytes dropped from the end of the file."""
    props = [(coord_type, "x")] + list(extras[:1]) + [(coord_type, "y")] + list(extras[1:2]) + [(coord_type, "z")] + list(extras[2:])
    head = ["ply", f"format {fmt} 1.0", "comment made by the test"]
    if "vertex" in elements:
        head += [f"element vertex {len(v)}"] + [f"property {p[0]} {p[1]}" for p in props]
    if "face" in elements:
        head += [f"element face {len(faces)}", f"property list {count_type} {index_type} {index_name}"]
        if face_extra:
            head += [f"property {face_extra[0]} {face_extra[1]}"]
    if "edge" in elements:
        head += ["element edge 0", "property int vertex1"]
    head += ["end_header"]
    body = bytearray()
    text = []
    for row in v:
        vals, k = [], 0
        for p in props:
            if p[1] in "xyz":
                vals.append((p[0], float(row[k])))
                k += 1
            else:
                vals.append((p[0], p[2]))
        if fmt == "ascii":
            text.append(" ".join(repr(x) if isinstance(x, float) else str(x) for _, x in vals))
        else:
            for t, x in vals:
                body += struct.pack("<" + _CODES[t], x)
    if "face" in elements:
        for fc in faces:
            if fmt == "ascii":
                text.append(" ".join(str(x) for x in [len(fc)] + list(fc)) + (" 7" if face_extra else ""))
            else:
                body += struct.pack("<" + _CODES[count_type], len(fc)) + struct.pack(f"<{len(fc)}" + _CODES[index_type], *fc)
                if face_extra:
                    body += struct.pack("<" + _CODES[face_extra[0]], 7)
    data = ("\n".join(head) + "\n").encode("ascii") + (("\n".join(text) + "\n").encode("ascii") if fmt == "ascii" else bytes(body))
    with open(path, "wb") as fh:
        fh.write(data[:len(data) - cut] if cut else data)


V8 = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1.5], [1, 0, 1.5], [1, 1, 1.5], [0.125, 1, 1.5]]) + np.float32(0.1)
TRIS = [(0, 1, 2), (0, 2, 3), (4, 6, 5), (7, 6, 4), (0, 5, 1)]
QUADS = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 4, 7, 3)]
EXTRAS = (("float", "nx", 0.5), ("uchar", "red", 200), ("uchar", "alpha", 255))


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("count_type", ["uchar", "uint8", "int", "int32", "uint", "uint32"])
@pytest.mark.parametrize("index_type", ["int", "int32", "uint", "uint32"])
def test_read_mesh_ply_accepts_every_list_and_index_type(tmp_path, fmt, count_type, index_type):
    import dqo_ply
    path = str(tmp_path / "m.ply")
    write_mesh(path, V8, TRIS, fmt, count_type, index_type, extras=EXTRAS)
    v, f = dqo_ply.read_mesh_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.flags["C_CONTIGUOUS"] and f.flags["C_CONTIGUOUS"]
    assert v.tobytes() == V8.tobytes() and f.tolist() == [list(t) for t in TRIS]


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_read_mesh_ply_splits_quads_and_skips_other_properties(tmp_path, fmt):
    import dqo_ply
    path = str(tmp_path / "q.ply")
    write_mesh(path, V8, QUADS, fmt, extras=EXTRAS, index_name="vertex_index", coord_type="float32")
    v, f = dqo_ply.read_mesh_ply(path)
    assert v.tobytes() == V8.tobytes()
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [0, 4, 7], [0, 7, 3]]  # (a, b, c), (a, c, d), in file order
    write_mesh(path, V8, TRIS, fmt)  # no extra property at all
    v, f = dqo_ply.read_mesh_ply(path)
    assert v.tobytes() == V8.tobytes() and f.tolist() == [list(t) for t in TRIS]
    # indices are not checked here: a negative one and one past the vertices come back as written; an unsigned one of 2^31 or more wraps
    write_mesh(path, V8, [(0, -1, 2), (0, 8, 3)], fmt)
    assert dqo_ply.read_mesh_ply(path)[1].tolist() == [[0, -1, 2], [0, 8, 3]]
    write_mesh(path, V8, [(0, 4294967295, 2)], fmt, index_type="uint")
    assert dqo_ply.read_mesh_ply(path)[1].tolist() == [[0, -1, 2]]


@pytest.mark.parametrize("case, kw, msg", [
    ("big-endian", dict(fmt="binary_big_endian"), "binary_big_endian is not supported"),
    ("double coordinates", dict(coord_type="double"), "double coordinates are not supported"),
    ("mixed sizes", dict(faces=[(0, 1, 2), (0, 1, 2, 3), (4, 5, 6)]), "mixed sizes"),
    ("mixed sizes, ascii", dict(faces=[(0, 1, 2), (0, 1, 2, 3), (4, 5, 6)], fmt="ascii"), "mixed sizes"),
    ("pentagons", dict(faces=[(0, 1, 2, 3, 4)]), "a face of 5 vertices"),
    ("pentagons, ascii", dict(faces=[(0, 1, 2, 3, 4)], fmt="ascii"), "a face of 5 vertices"),
    ("another face property", dict(face_extra=("uchar", "flags")), "the face element has 2 properties"),
    ("a list of shorts", dict(index_type="short"), "face property 'list uchar short vertex_indices'"),
    ("another list", dict(index_name="texcoord"), "face property 'list uchar int texcoord'"),
    ("no face element", dict(elements=("vertex",)), "no face element"),
    ("no vertex element", dict(elements=("face",)), "no vertex element"),
    ("a third element", dict(elements=("vertex", "face", "edge")), "nothing else"),
    ("truncated faces", dict(cut=5), "truncated face data"),
    ("truncated vertices", dict(cut=5 * 13 + 8 * 12 - 6), "truncated vertex data"),
    ("truncated faces, ascii", dict(fmt="ascii", cut=8), "truncated face data|mixed sizes"),
    ("unknown format", dict(fmt="binary_middle_endian"), "unknown format"),
])
def test_read_mesh_ply_rejections_name_the_file_and_the_reason(tmp_path, case, kw, msg):
    import dqo_ply
    path = str(tmp_path / "bad.ply")
    a = dict(v=V8, faces=TRIS)
    a.update(kw)
    write_mesh(path, a.pop("v"), a.pop("faces"), **a)
    with pytest.raises(RuntimeError, match=msg) as e:
        dqo_ply.read_mesh_ply(path)
    assert "bad.ply" in str(e.value), case


def test_read_mesh_ply_rejects_what_is_not_a_ply(tmp_path):
    import dqo_ply
    path = str(tmp_path / "bad.ply")
    with open(path, "wb") as fh:
        fh.write(b"solid cube\n")
    with pytest.raises(RuntimeError, match="not a PLY file"):
        dqo_ply.read_mesh_ply(path)
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\n")
    with pytest.raises(RuntimeError, match="truncated header"):
        dqo_ply.read_mesh_ply(path)


# ---- the ABI, without a GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_symbols_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
    assert native.lib().dqo_abi_version() == 5 and native.lib().dqo_abi_sizeof(13) == 0
    import dqo_eval
    assert int(re.search(r"#define DQO_MESH_SCAN_BLOCK (\d+)", hdr).group(1)) == dqo_eval.MESH_SCAN_BLOCK
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert "map_meshsample.hip" in mk and re.search(r"map_meshsample\.o: HIPFLAGS \+= -ffp-contract=off", mk)


def _call(native, **kw):
    a = dict(V=100, vertices=FAKE, F=50, faces=FAKE, count=1000, seed=0, points=FAKE, face_index=None, keep=FAKE, header=FAKE, ws=FAKE,
             ws_bytes=1 << 40)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_mesh_sample(a["V"], a["vertices"], a["F"], a["faces"], a["count"], a["seed"], a["points"], a["face_index"], a["keep"],
                           a["header"], a["ws"], a["ws_bytes"], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("null vertices", dict(vertices=None), "null pointer"),
    ("null faces", dict(faces=None), "null pointer"),
    ("null points", dict(points=None), "null pointer"),
    ("null keep", dict(keep=None), "null pointer"),
    ("null header", dict(header=None), "null pointer"),
    ("V 0", dict(V=0), "bad vertex count"),
    ("V negative", dict(V=-3), "bad vertex count"),
    ("F 0", dict(F=0), "bad face count"),
    ("F negative", dict(F=-1), "bad face count"),
    ("F 2^25", dict(F=1 << 25), "bad face count"),
    ("count 0", dict(count=0), "bad sample count"),
    ("count negative", dict(count=-7), "bad sample count"),
    ("count 2^25", dict(count=1 << 25), "bad sample count"),
])
def test_validation_errors_without_a_gpu(native, case, kw, msg):
    rc, err = _call(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)  # DQO_ERR_INVALID_ARG


def test_short_or_missing_workspace(native):
    need = native.lib().dqo_mesh_sample_workspace_bytes(50, 1000)
    assert need > 0
    for kw in (dict(ws_bytes=need - 1), dict(ws=None)):
        rc, err = _call(native, **kw)
        assert rc == -2 and "workspace too small" in err, (rc, err)  # DQO_ERR_WORKSPACE


def test_workspace_bytes(native):
    f = native.lib().dqo_mesh_sample_workspace_bytes
    sizes = [f(F, 1000) for F in (1, 1024, 1025, 100000, 2000000, (1 << 25) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[2] < sizes[3] < sizes[4] < sizes[5]
    assert sizes[5] >= 8 * ((1 << 25) - 1) and f(50, 1) == f(50, (1 << 25) - 1) > 0
    for bad in ((0, 10), (-1, 10), (1 << 25, 10), (10, 0), (10, -1), (10, 1 << 25)):
        assert f(*bad) == 0, bad


def test_python_entry(native):
    import torch
    import dqo_eval
    import dqo_ply
    from dqo_harness.fused_mapping import FusedMapper
    sig = inspect.signature(dqo_eval.sample_surface)
    assert list(sig.parameters) == ["vertices", "faces", "count", "seed", "want_face_index", "workspace_buffer"]
    assert [sig.parameters[k].default for k in ("seed", "want_face_index", "workspace_buffer")] == [0, False, None]
    sig = inspect.signature(FusedMapper.evaluate_geometry_mesh)
    assert list(sig.parameters) == ["self", "vertices", "faces", "sample_nums", "seed", "dist_thres", "transform", "out", "row", "densify"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sample_nums"], d["seed"], d["dist_thres"], d["transform"], d["out"], d["row"], d["densify"]) == (1000000, 0, (0.03,), None,
                                                                                                                None, 0, None)
    assert list(inspect.signature(dqo_ply.read_mesh_ply).parameters) == ["path"]
    assert dqo_eval.MESH_SCAN_BLOCK >= 256 and len(dqo_eval.MESH_HEADER) == 8
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.sample_surface(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), 10)
    # nothing in the documentation still leaves the sampling to the caller
    for word in ("trimesh", "open3d", "sample_surface"):
        assert word in dqo_eval.__doc__, word
    assert "the caller passes the ground truth as points" not in dqo_eval.__doc__
