"""The numpy oracle of csrc/map_tsdf.hip (tests/tsdf_oracle.py) held to what does not depend on it: a sphere written straight into the
volume comes out as a closed, outward-oriented manifold of the analytic volume and area; the flip table is the geometric rule; an
unobserved slab opens the mesh without leaving a vertex unreferenced; a corner at exactly 0 is positive; the capacities cut prefixes."""
import functools

import numpy as np

import tsdf_oracle as O


@functools.lru_cache(maxsize=1)
def sphere_mesh():
    origin, L, tsdf, weight, color = O.sphere_volume()
    return origin, L, tsdf, weight, color, O.extract(tsdf, weight, color, origin, L)


def directed_edges(F):
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    return e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]


def geometric_flip(k, case):
    """Whether the triangles of (tetrahedron k, case), taken with their vertices at the edge midpoints of the unit cube, have their
    right-hand normal pointing AWAY from the positive corners."""
    codes = O.path_codes(k)
    P = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in codes], float)
    neg = [i for i in range(4) if (case >> i) & 1]
    pos = [i for i in range(4) if not (case >> i) & 1]
    want = P[pos].mean(0) - P[neg].mean(0)
    out = set()
    for tri in O.case_triangles(case):
        v = [0.5 * (P[a] + P[b]) for a, b in tri]
        d = np.cross(v[1] - v[0], v[2] - v[0]) @ want
        assert abs(d) > 1e-9
        out.add(bool(d < 0))
    assert len(out) == 1, (k, case)  # (both halves of a quad agree)
    return out.pop()


def test_the_flip_table_is_the_geometric_rule():
    """All 84 (tetrahedron, case) pairs: the geometric flip is FLIP[case] XOR parity(p)."""
    assert O.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)) and O.PERM_PARITY == (0, 1, 1, 0, 0, 1)
    mask = 0
    for case in range(1, 15):
        per_k = [geometric_flip(k, case) ^ bool(O.PERM_PARITY[k]) for k in range(6)]
        assert len(set(per_k)) == 1, case
        mask |= int(per_k[0]) << case
    assert mask == O.FLIP_MASK
    assert [c for c in range(16) if (mask >> c) & 1] == [0b0010, 0b0101, 0b1000, 0b1010, 0b1011, 0b1110]
    # the six tetrahedra tile the cube: every one has volume 1/6 and they share the body diagonal
    for k in range(6):
        P = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in O.path_codes(k)], float)
        assert abs(abs(np.linalg.det(P[1:] - P[0])) - 1.0) < 1e-12 and O.path_codes(k)[0] == 0 and O.path_codes(k)[3] == 7


def test_sphere_is_a_closed_oriented_manifold():
    """n = 24, r = 0.31, centre (0.03, -0.02, 0.011), tsdf = clip(dist / 3L, -1, 1), all weights 1.  Measured with this oracle
    (float32): 3132 vertices, 6260 faces, Euler characteristic 2, volume ratio 0.99097, area ratio 0.99535, maximum radial error
    0.0497 L, no degenerate triangle.  Bars: volume within 2 %, area within 1 %, every vertex within 0.1 L of the sphere."""
    origin, L, tsdf, weight, color, m = sphere_mesh()
    V, F = m["vertices"].astype(np.float64), m["faces"]
    assert m["header"].tolist() == [len(V), len(F), 0, 0] and len(V) > 1000 and m["colors"].shape == V.shape
    print("vertices", len(V), "faces", len(F))
    assert F.min() == 0 and F.max() == len(V) - 1 and len(np.unique(F)) == len(V)  # (no vertex is unreferenced)
    fwd, rev = directed_edges(F)
    assert len(np.unique(fwd)) == len(fwd)  # every directed edge once ...
    assert np.array_equal(np.sort(fwd), np.sort(rev))  # ... and its reverse once
    euler = len(V) - len(fwd) // 2 + len(F)
    assert euler == 2
    r, ctr = 0.31, np.array([0.03, -0.02, 0.011])
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(b - a, c - a)
    assert ((n * ((a + b + c) / 3 - ctr)).sum(1) > 0).all()  # normals point outward: to the positive side
    volume = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6
    area = 0.5 * np.linalg.norm(n, axis=1).sum()
    radial = np.abs(np.linalg.norm(V - ctr, axis=1) - r).max() / float(L)
    print("volume ratio", volume / (4 / 3 * np.pi * r ** 3), "area ratio", area / (4 * np.pi * r * r), "max radial error / L", radial)
    assert abs(volume / (4 / 3 * np.pi * r ** 3) - 1) < 0.02
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert radial < 0.1
    # colour was the voxel centre's position + 0.5, a linear field: interpolated the same way it is the vertex position + 0.5
    assert np.abs(m["colors"].astype(np.float64) - (V + 0.5)).max() < 1e-6


def test_an_unobserved_slab_opens_the_mesh_and_leaves_no_unreferenced_vertex():
    origin, L, tsdf, weight, color, full = sphere_mesh()
    w = weight.copy()
    w[:, :, 11:13] = 0.0  # x = 11, 12 never observed: the cubes x = 10, 11, 12 are invalid
    m = O.extract(tsdf, w, color, origin, L)
    V, F = m["vertices"], m["faces"]
    assert 0 < len(F) < len(full["faces"]) and len(V) < len(full["vertices"])
    assert len(np.unique(F)) == len(V) and F.max() == len(V) - 1
    fwd, rev = directed_edges(F)
    assert len(np.unique(fwd)) == len(fwd)
    boundary = np.setdiff1d(fwd, rev)
    assert len(boundary) > 0  # open
    # every face of the cut mesh is a face of the full mesh (same coordinates), none touches the slab
    x = V[:, 0].astype(np.float64)
    lo, hi = float(origin[0]) + 10.5 * float(L), float(origin[0]) + 13.5 * float(L)
    assert not ((x > lo + 1e-6) & (x < hi - 1e-6)).any()
    full_set = {v.tobytes() for v in full["vertices"]}
    assert all(v.tobytes() in full_set for v in V)
    # nothing observed at all: an empty mesh
    e = O.extract(tsdf, np.zeros_like(w), color, origin, L)
    assert e["header"].tolist() == [0, 0, 0, 0] and e["vertices"].shape == (0, 3) and e["faces"].shape == (0, 3)


def test_a_corner_at_exactly_zero_is_positive():
    one = np.ones((2, 2, 2), np.float32)
    col = np.zeros((3, 2, 2, 2), np.float32)
    origin, L = (0.0, 0.0, 0.0), 1.0
    t = one.copy()
    t[0, 0, 0] = 0.0
    assert O.extract(t, one, col, origin, L)["header"].tolist() == [0, 0, 0, 0]
    t[0, 0, 0] = -0.0
    assert O.extract(t, one, col, origin, L)["header"].tolist() == [0, 0, 0, 0]  # (-0 < 0 is false)
    # one negative corner, one neighbour at 0: the vertex of that edge sits on the neighbour (s = 1), the others halfway
    t = one.copy()
    t[0, 0, 0], t[0, 0, 1] = -1.0, 0.0
    m = O.extract(t, one, col, origin, L)
    assert m["header"].tolist() == [7, 6, 0, 0]  # seven edges leave the corner, one triangle per tetrahedron
    assert m["vertices"][0].tolist() == [1.5, 0.5, 0.5]  # edge type 0 (x) of lattice point 0: s = -1 / (-1 - 0) = 1
    assert m["vertices"][1].tolist() == [0.5, 1.0, 0.5]  # type 1 (y): s = -1 / (-1 - 1) = 0.5
    assert m["vertices"][6].tolist() == [1.0, 1.0, 1.0]  # type 6, the body diagonal


def test_capacities_cut_prefixes_and_count_what_they_drop():
    origin, L, tsdf, weight, color, full = sphere_mesh()
    V, F = len(full["vertices"]), len(full["faces"])
    m = O.extract(tsdf, weight, color, origin, L, cap_vertices=V - 500, cap_faces=F)
    nv = V - 500
    keep = (full["faces"] < nv).all(1)
    assert 0 < keep.sum() < F
    assert m["header"].tolist() == [nv, int(keep.sum()), 500, F - int(keep.sum())]
    assert np.array_equal(m["vertices"], full["vertices"][:nv]) and np.array_equal(m["faces"], full["faces"][keep])
    m = O.extract(tsdf, weight, color, origin, L, cap_vertices=V + 5, cap_faces=1000)
    assert m["header"].tolist() == [V, 1000, 0, F - 1000] and np.array_equal(m["faces"], full["faces"][:1000])
    m = O.extract(tsdf, weight, color, origin, L, cap_vertices=0, cap_faces=10)
    assert m["header"].tolist() == [0, 0, V, F]


def test_integrate_of_a_fronto_parallel_plane():
    """A camera at the origin looking along +z at the plane z = 1: the voxels of the central column get tsdf = min(1, (1 - z) / trunc)
    along the ray through the principal point, weight 1 where sdf > -trunc, and the pixel's colour; a second frame averages."""
    dims, L, trunc = (6, 5, 20), np.float32(0.1), np.float32(0.25)
    origin = (np.float32(-0.3), np.float32(-0.25), np.float32(0.0))
    W, H, f = 9, 7, 20.0
    depth = np.ones((H, W), np.float32)
    color = np.stack([np.full((H, W), v, np.float32) for v in (0.25, 0.5, 0.75)])
    vol = O.integrate(O.clear(dims), origin, L, trunc, depth, color, f, f, 4.0, 3.0, np.eye(4, dtype=np.float32), 30.0)
    z = np.float32(0.0) + (np.arange(20, dtype=np.float32) + np.float32(0.5)) * L
    x, y = 3, 2  # the voxel centre (0.05, 0.0): pixel (int(0.05 * 20 / z + 4.5), 3)
    for k in range(20):
        u = int(np.float32(np.float32(0.05) * np.float32(20.0)) / z[k] + 4.5)
        if not 0 <= u < W:
            assert vol["weight"][k, y, x] == 0
            continue
        mult = np.sqrt(1.0 + ((u - 4.0) / 20.0) ** 2)
        sdf = (1.0 - float(z[k])) * mult
        if sdf > -float(trunc):
            assert vol["weight"][k, y, x] == 1 and abs(vol["tsdf"][k, y, x] - min(1.0, sdf / float(trunc))) < 1e-6, k
            assert vol["color"][:, k, y, x].tolist() == [0.25, 0.5, 0.75]
        else:
            assert vol["weight"][k, y, x] == 0 and vol["tsdf"][k, y, x] == 1 and vol["color"][0, k, y, x] == 0, k
    first = {k: v.copy() for k, v in vol.items()}
    O.integrate(vol, origin, L, trunc, depth, 2 * color, f, f, 4.0, 3.0, np.eye(4, dtype=np.float32), 30.0)
    seen = first["weight"] > 0
    assert seen.any() and np.array_equal(vol["weight"][seen], np.full(seen.sum(), 2, np.float32)) and (vol["weight"][~seen] == 0).all()
    assert np.array_equal(vol["tsdf"], first["tsdf"]) and np.allclose(vol["color"][:, seen], 1.5 * first["color"][:, seen])
    # depth_trunc and d = 0
    none = O.integrate(O.clear(dims), origin, L, trunc, depth, color, f, f, 4.0, 3.0, np.eye(4, dtype=np.float32), 0.5)
    assert (none["weight"] == 0).all()
    none = O.integrate(O.clear(dims), origin, L, trunc, 0 * depth, color, f, f, 4.0, 3.0, np.eye(4, dtype=np.float32), 30.0)
    assert (none["weight"] == 0).all() and (none["tsdf"] == 1).all()
