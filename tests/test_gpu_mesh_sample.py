"""GPU: the ground-truth mesh sampler (dqo_eval.sample_surface, FusedMapper.evaluate_geometry_mesh — csrc/map_meshsample.hip) against
tests/mesh_oracle.py.

Bars, and why.  Quanta: |q_dev - q_oracle| <= 1 for every face — each double statement of an area rounds once on both sides and the file is
compiled without contraction, so the areas can differ only where the device's sqrt differs from numpy's correctly rounded one, by an ulp;
a quantum is at least 2^17 ulps of any area (the largest face has at least 2^35 quanta of its 53 bits), so only the floor can move, by one.
The count of faces that differ at all is printed; the expectation is zero.  The exponent e: exactly — the test asserts that amax's
mantissa is not within 1e-9 of 0.5 or 1, so it cannot depend on a last bit.  Decisions: with the DEVICE's table of quanta fed to the
oracle's scan and draw, face_index, points (bit for bit), keep and the header are equal — integer statements, and double statements
without contraction.  The geometry row: the bars of tests/test_gpu_eval_pcd.py."""
import numpy as np
import pytest

import mesh_oracle as mo
from test_mesh_oracle import normal_mesh, write_mesh

pytestmark = pytest.mark.gpu

THRES = (0.01, 0.03)


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.asarray(a, dtype), device="cuda")


def _B():
    import dqo_eval
    return dqo_eval.MESH_SCAN_BLOCK


def _zero_faces(F, B):
    """Zero-area faces at the start, at the end and in a run — across the boundary of two scan blocks where the mesh has one."""
    if F < 8:
        return ()
    mid = B if F > B + 2 else F // 2
    return tuple(sorted({0, 1, F - 1, mid - 2, mid - 1, mid, mid + 1}))


def _mesh(F, seed=0):
    B = _B()
    V = 200 if F <= 4 * B else 5000
    return normal_mesh(100 + seed + F % 97, V, F, _zero_faces(F, B))


def _sample(v, f, count, seed, vt=None, ws=None):
    """(dict of numpy arrays, cum int64 [F]) of one call."""
    import torch
    import dqo_eval
    F = f.shape[0]
    ws = dqo_eval.mesh_sample_workspace(F, count, "cuda") if ws is None else ws
    d = dqo_eval.sample_surface(_t(v) if vt is None else vt, _t(f), count, seed=seed, want_face_index=True, workspace_buffer=ws)
    torch.cuda.synchronize()
    cum = dqo_eval.mesh_cum_view(ws, F).cpu().numpy().copy()
    return {k: t.cpu().numpy() for k, t in d.items()}, cum


def _check(v, f, count, seed, what, vt=None):
    """One call against the oracle; returns the number of faces whose quanta differ."""
    F = f.shape[0]
    got, cum = _sample(v, f, count, seed, vt)
    o = mo.sample_surface_oracle(v, f, count, seed)
    # the areas: the table's differences are the quanta
    q_dev = np.diff(cum, prepend=np.int64(0))
    q_or = o["q"].astype(np.int64)
    assert (q_dev >= 0).all() and cum[-1] < (1 << 61), what
    _, m = mo.quantum_exponent(o["A"].max(), F)
    assert min(abs(m - 0.5), abs(m - 1.0)) > 1e-9, (what, m)  # (the premise: e cannot depend on amax's last bit)
    hdr = got["header"].tolist()
    assert hdr[4] == o["e"], (what, hdr, o["e"])
    diff = np.abs(q_dev - q_or)
    differing = int((diff != 0).sum())
    print(f"{what}: F {F} count {count} e {hdr[4]} faces whose quanta differ {differing} (largest difference {int(diff.max())})")
    assert diff.max() <= 1, what
    assert ((q_dev == 0) == (q_or == 0)).all(), what  # (a face without area has none on either side: exact zeros)
    # the decisions, from the device's own table
    d = mo.draw(v, f, q_dev.astype(np.uint64), count, seed)
    total = int(cum[-1])
    assert d["total"] == total and total > 0, what
    assert hdr[:4] == o["header"][:4] and hdr[0] == count and hdr[7] == 0, (what, hdr, o["header"])
    assert got["header"][5:7].tobytes() == mo.header_i32([0, 0, 0, 0, 0, total & mo.MASK, total >> 32, 0])[5:7].tobytes(), what
    assert got["face_index"].dtype == np.int32 and (got["face_index"] == d["face_index"]).all(), what
    assert got["points"].dtype == np.float32 and got["points"].view(np.int32).tobytes() == d["points"].view(np.int32).tobytes(), what
    assert got["keep"].dtype == np.uint8 and (got["keep"] == 1).all(), what
    assert (q_dev[got["face_index"]] > 0).all(), what  # (a face without quanta is never picked)
    return differing


def _sizes():
    B = 1024  # (asserted equal to the module's MESH_SCAN_BLOCK in the test: a parametrisation cannot import the product at collection)
    counts = (1, 255, 257, 4099)
    Fs = (1, 255, 256, 257, B - 1, B, B + 1, 2 * B + 1, 256 * B + 777)
    cases = [(F, counts[(i + 2) % 4]) for i, F in enumerate(Fs[:-1])] + [(Fs[-1], 4099)]  # (the widest search gets the most samples)
    cases += [(2 * B + 1, c) for c in counts if (2 * B + 1, c) not in cases]
    return cases


@pytest.mark.parametrize("F, count", _sizes())
def test_table_and_samples_against_the_oracle(F, count):
    assert _B() == 1024
    v, f = _mesh(F)
    _check(v, f, count, seed=F + count, what=f"F={F}")


def test_reproducible_and_seeded():
    v, f = _mesh(2 * _B() + 1)
    a, cum_a = _sample(v, f, 4099, 7)
    b, cum_b = _sample(v, f, 4099, 7)
    c, cum_c = _sample(v, f, 4099, 8)
    for k in ("points", "face_index", "keep", "header"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert cum_a.tobytes() == cum_b.tobytes() == cum_c.tobytes()
    assert a["points"].tobytes() != c["points"].tobytes() and (a["face_index"] != c["face_index"]).mean() > 0.9
    assert a["header"].tobytes() == c["header"].tobytes()
    # a 64-bit seed: the high word counts
    d, _ = _sample(v, f, 4099, 7 | (1 << 40))
    assert a["points"].tobytes() != d["points"].tobytes()


def test_faces_with_indices_out_of_range_are_counted_and_never_read():
    import torch
    B = _B()
    v, f = _mesh(B + 1)
    V = v.shape[0]
    f = f.copy()
    f[3, 0], f[4, 2], f[B - 1, 1], f[B, 0], f[B, 1] = -1, V, V + 1000, -5, V
    # the vertices are a [V,3] slice from the middle of a larger allocation: a face that were read past either end would still read mapped
    # memory (and give a wrong table, which the comparison below sees)
    big = torch.full((3 * V, 3), 1e6, dtype=torch.float32, device="cuda")
    big[V:2 * V] = _t(v)
    vt = big[V:2 * V]
    assert vt.is_contiguous() and vt.data_ptr() == big.data_ptr() + 12 * V
    _check(v, f, 4099, seed=2, what="bad indices", vt=vt)
    got, cum = _sample(v, f, 4099, 2, vt)
    assert got["header"][2] == 4 and not np.isin(got["face_index"], [3, 4, B - 1, B]).any()
    q = np.diff(cum, prepend=np.int64(0))
    assert (q[[3, 4, B - 1, B]] == 0).all() and np.abs(got["points"]).max() < 100


BOX = ((-0.5, -0.4, 1.5), (0.5, 0.35, 2.5))  # a box of 5 m^2 in front of the camera


def _scene():
    """(camera, scene): the frustum cloud of tests/test_gpu_eval_pcd.py's mapper with its 1700 Gaussians moved onto the box's surface,
    1 cm of noise on top — 340 per m^2, so that both thresholds separate."""
    from dqo_harness import scenes
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    scene = dict(scenes.frustum_cloud(17, 1700, cam))
    v, f = box_mesh(*BOX)
    on = mo.sample_surface_oracle(v, f, 1700, seed=99)["points"]
    scene["xyz"] = (on + np.random.default_rng(6).normal(0, 0.01, on.shape)).astype(np.asarray(scene["xyz"]).dtype)
    return cam, scene


def _mapper(stable=False):
    import torch
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam, scene = _scene()
    fm = FusedMapper(scene, mapping.make_settings(cam, dev), dev).reserve(300)
    fm.alive[5:1700:9] = 0
    if stable:
        fm.track_lifecycle(stable_mask=torch.arange(fm.P, device=dev) % 3 != 0)
    return fm, np.asarray(scene["xyz"], np.float32)


def test_a_mesh_without_area_gives_no_sample_and_a_row_of_nan():
    import torch
    v, f = normal_mesh(5, 50, 300, zero=range(300))
    got, cum = _sample(v, f, 257, 0)
    hdr = got["header"].tolist()
    assert hdr == [0, 300, 0, 300, 61 - 9, 0, 0, 0] and (got["keep"] == 0).all() and (cum == 0).all()
    fm, _ = _mapper()
    row = fm.evaluate_geometry_mesh(_t(v), _t(f), sample_nums=257, dist_thres=THRES)
    torch.cuda.synchronize()
    assert tuple(row.shape) == (32,) and np.isnan(row.cpu().numpy()).all()


def test_one_capture_replayed_twice_equals_the_eager_call():
    import torch
    import dqo_eval
    v, f = _mesh(2 * _B() + 1)
    vt, ft = _t(v), _t(f)
    ws = dqo_eval.mesh_sample_workspace(f.shape[0], 4099, "cuda")
    eager = dqo_eval.sample_surface(vt, ft, 4099, seed=11, want_face_index=True, workspace_buffer=ws)
    torch.cuda.synchronize()
    want = {k: t.cpu().numpy().tobytes() for k, t in eager.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branch; the outputs are the capture's own allocations)
        out = dqo_eval.sample_surface(vt, ft, 4099, seed=11, want_face_index=True, workspace_buffer=ws)
    for _ in range(2):
        for t in out.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, t in out.items():
            assert t.cpu().numpy().tobytes() == want[k], k


def box_mesh(lo, hi, n=16):
    """A closed box from lo to hi, every side an n x n grid of quads cut in two: 6 (n + 1)^2 vertices, 12 n^2 triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    g = np.linspace(0.0, 1.0, n + 1)
    s, t = [x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij")]
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.zeros((s.size, 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side, s, t
            i, j = [x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
            a = len(verts) * s.size + i * (n + 1) + j
            b, c, d = a + (n + 1), a + (n + 1) + 1, a + 1
            faces.append(np.stack([a, b, c], 1) if side else np.stack([a, c, b], 1))
            faces.append(np.stack([a, c, d], 1) if side else np.stack([a, d, c], 1))
            verts.append(lo + p * (hi - lo))
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)


@pytest.mark.parametrize("densified", [False, True])
def test_from_a_mesh_file_to_the_geometry_row(tmp_path, densified):
    import torch
    import dqo_eval
    import dqo_ply
    import pcd_oracle as po
    from test_gpu_eval_pcd import _assert_row
    fm, xyz = _mapper(stable=densified)
    v0, f0 = box_mesh(*BOX)
    assert f0.shape == (3072, 3)
    path = str(tmp_path / "gt_mesh.ply")
    write_mesh(path, v0, [tuple(r) for r in f0.tolist()], extras=(("float", "nx", 0.0), ("uchar", "red", 128)))
    v, f = dqo_ply.read_mesh_ply(path)
    assert v.tobytes() == v0.tobytes() and f.tobytes() == f0.tobytes()
    vt, ft = _t(v), _t(f)
    n, seed = 4099, 5
    densify = True if densified else None
    got = fm.evaluate_geometry_mesh(vt, ft, sample_nums=n, seed=seed, dist_thres=THRES, densify=densify).clone()
    s = dqo_eval.sample_surface(vt, ft, n, seed=seed)
    if densified:
        want = fm.evaluate_geometry_densified(s["points"], THRES).clone()
        d = fm.densify(sample_nums=1000000, want_normals=False)
        rec = d["points"][d["keep"].bool()].cpu().numpy()
    else:
        want = fm.evaluate_geometry(s["points"], THRES).clone()
        rec = fm.xyz.detach()[fm.alive.bool()].cpu().numpy()
    torch.cuda.synchronize()
    b = lambda t: t.cpu().numpy().view(np.uint32).tobytes()
    assert b(got) == b(want), (got[:10].tolist(), want[:10].tolist())
    # ... and against the oracles: the oracle's own samples of the mesh, cKDTree's distances, eval.py's statements in float64
    o = mo.sample_surface_oracle(v, f, n, seed)
    assert s["points"].cpu().numpy().view(np.int32).tobytes() == o["points"].view(np.int32).tobytes()
    d_rec64, d_gt64 = po.kdtree_distances(o["points"], rec)
    for d64 in (d_rec64, d_gt64):  # (the premise of exact counts: the float32 distances are within 2e-7 relative of these)
        assert all((np.abs(d64 - th) > 1e-6 * th).all() for th in THRES)
    print("densified" if densified else "live rows", "reconstructed points", rec.shape[0], got[:10].tolist())
    _assert_row(got.cpu().numpy(), n, rec.shape[0], d_rec64, d_gt64, THRES, "mesh")
    assert 0 < got[7].item() < 100 and 0 < got[8].item() < 100  # (a threshold that separates: some points within 3 cm, not all)
