"""Oracle of the exact point-to-triangle distance (dqo_mesh_nearest, dqo_eval_pcd_surface): numpy only.

tri_dist_f32    the rule of include/dqo_raster.h one float32 rounding at a time: every array below is float32 and every numpy operation
                on two float32 arrays rounds once, so a line here is a line of the header.  Vectorised over [Q, F] pairs.
tri_dist_f64    the same walk in float64 (the comparison the float32 rule's error is measured against).
face_validity   the validity rule and the header's counts.
nearest_oracle  the definition: the minimum of D over ALL valid faces (brute force in chunks of faces, or the same minimum from the pairs
                a box test cannot exclude), with the keep mask and the two transforms of the entry.
fixtures        the meshes and queries the tests share (clamp_cases: pairs on which the clamp by the face's box is active); room_meshes / sample_mesh: the evaluation's small room.
"""
import numpy as np

from pcd_oracle import FLT_MAX, transform_f32

HEADER = ("faces", "faces_valid", "faces_bad_index", "faces_degenerate", "queries", "zero5", "zero6", "zero7")


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _tri_dist(p, a, b, c, dtype):
    """p [...,3] against triangles a, b, c [...,3] (broadcastable), every operation in `dtype`.
    Returns (D, E, region int8 (0..6), x [...,3], fallback bool): D = fmax(E, B(p, aabb)), fallback: E was not finite and became ap.ap."""
    p, a, b, c = (np.asarray(t, dtype) for t in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)]
        region = np.select(conds, [np.int8(k) for k in range(6)], default=np.int8(6)).astype(np.int8)
        v2 = (d1 / (d1 - d3))[..., None]
        w4 = (d2 / (d2 - d6))[..., None]
        w5 = (e / (e + g))[..., None]
        den = dtype(1) / ((va + vb) + vc)
        v6, w6 = (vb * den)[..., None], (vc * den)[..., None]
        shape = np.broadcast(p, a).shape
        xs = [a, b, a + v2 * ab, c, a + w4 * ac, b + w5 * (c - b), (a + ab * v6) + ac * w6]
        x = np.zeros(shape, dtype)
        for k, xk in enumerate(xs):
            x = np.where((region == k)[..., None], np.broadcast_to(xk, shape), x)
        r = p - x
        E = _dot(r, r)
        fallback = ~np.isfinite(E)
        E = np.where(fallback, np.broadcast_to(_dot(ap, ap), E.shape), E)
        x = np.where(fallback[..., None], np.broadcast_to(a, shape), x)
        lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        d = np.where((p < lo) | (p > hi), np.fmin(np.abs(p - lo), np.abs(p - hi)), dtype(0))
        B = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # (box_dist_f32's statements, in `dtype`)
        D = np.fmax(E, B)
    assert D.dtype == dtype and x.dtype == dtype
    return D, E, region, x, fallback


def tri_dist_f32(p, a, b, c):
    return _tri_dist(p, a, b, c, np.float32)


def tri_dist_f64(p, a, b, c):
    return _tri_dist(p, a, b, c, np.float64)


def mesh_counts(vertices, faces, counts):
    cap_v, cap_f = vertices.shape[0], faces.shape[0]
    if counts is None:
        return cap_v, cap_f
    return min(max(int(counts[0]), 0), cap_v), min(max(int(counts[1]), 0), cap_f)


def face_validity(vertices, faces, counts=None, xform=None):
    """(valid bool [cap_f], header int32 [8] without the query count, corners (a, b, c) float32 [cap_f,3] — rows of invalid faces are 0)."""
    vertices, faces = transform_f32(np.asarray(vertices, np.float32), xform), np.asarray(faces, np.int64)
    V, F = mesh_counts(vertices, faces, counts)
    below = np.arange(faces.shape[0]) < F
    index_ok = below & ((faces >= 0) & (faces < V)).all(axis=1)
    safe = np.where(index_ok[:, None], faces, 0)
    a, b, c = vertices[safe[:, 0]], vertices[safe[:, 1]], vertices[safe[:, 2]]
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        nn = _dot(n, n)
    assert nn.dtype == np.float32
    valid = index_ok & np.isfinite(nn) & (nn > 0)
    header = np.zeros(8, np.int32)
    header[:4] = F, valid.sum(), (below & ~index_ok).sum(), (index_ok & ~valid).sum()
    zero = np.where(valid[:, None], np.float32(1), np.float32(0))
    return valid, header, (a * zero, b * zero, c * zero)


def box_dist_f32(p, lo, hi):
    """dist_box_point (csrc/knn.hip): the squared distance of p to the box [lo, hi], float32, broadcastable [...,3]."""
    with np.errstate(all="ignore"):
        d = np.where((p < lo) | (p > hi), np.fmin(np.abs(p - lo), np.abs(p - hi)), np.float32(0))
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_oracle(points, mesh, keeps=None, xforms=(None, None), brute=False, chunk=1024):
    """What dqo_mesh_nearest returns: (dist2 float32 [Q], face int32 [Q] — one admissible answer —, closest float32 [Q,3] for that
    face (rows without a face: NaN), header int32 [8]).  mesh = (vertices, faces, counts or None); keeps: the query keep mask;
    xforms = (query_xform, mesh_xform).
    brute: D against ALL valid faces, in chunks — the definition.  Otherwise the same minimum from fewer pairs: an upper bound ub from
    the faces with the 16 nearest centroids, then D on every pair with B(p, aabb(f)) <= ub — D >= B by its own definition, so a pair
    left out has D > ub >= the minimum: no float argument is needed.  tests/test_mesh_dist_oracle.py holds the two against each other."""
    from scipy.spatial import cKDTree
    vertices, faces, counts = mesh
    p = transform_f32(np.asarray(points, np.float32), xforms[0])
    Q = p.shape[0]
    keep = np.ones(Q, bool) if keeps is None else np.asarray(keeps).astype(bool)
    valid, header, (a, b, c) = face_validity(vertices, faces, counts, xforms[1])
    header[4] = keep.sum()
    dist2, face = np.full(Q, FLT_MAX, np.float32), np.full(Q, -1, np.int32)
    closest = np.full((Q, 3), np.nan, np.float32)
    rows, qi = np.nonzero(valid)[0], np.nonzero(keep)[0]
    if rows.size == 0 or qi.size == 0:
        return dist2, face, closest, header
    pq, a, b, c = p[qi], a[rows], b[rows], c[rows]
    best, arg = np.full(qi.size, np.inf, np.float32), np.zeros(qi.size, np.int64)

    def fold(q_of, f_of, D):  # the minimum of D per query over the listed (query, face) pairs
        if D.size == 0:
            return
        order = np.lexsort((D, q_of))
        first = order[np.r_[True, q_of[order][1:] != q_of[order][:-1]]]
        take = D[first] < best[q_of[first]]
        best[q_of[first[take]]], arg[q_of[first[take]]] = D[first[take]], f_of[first[take]]

    if brute:
        every = np.arange(qi.size)
        for s in range(0, rows.size, chunk):
            D = tri_dist_f32(pq[:, None, :], a[None, s:s + chunk], b[None, s:s + chunk], c[None, s:s + chunk])[0]
            k = D.argmin(axis=1)
            fold(every, s + k, D[every, k])
    else:
        k = min(16, rows.size)
        cent = (a.astype(np.float64) + b + c) / 3
        cand = cKDTree(cent).query(np.nan_to_num(pq.astype(np.float64)), k=k)[1].reshape(qi.size, k)
        D = tri_dist_f32(pq[:, None, :], a[cand], b[cand], c[cand])[0]
        fold(np.repeat(np.arange(qi.size), k), cand.reshape(-1), D.reshape(-1))
        lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        for s in range(0, qi.size, chunk):
            B = box_dist_f32(pq[s:s + chunk, None, :], lo[None], hi[None])
            q_of, f_of = np.nonzero(B <= best[s:s + chunk, None])
            fold(s + q_of, f_of, tri_dist_f32(pq[s + q_of], a[f_of], b[f_of], c[f_of])[0])
    dist2[qi], face[qi] = best, rows[arg].astype(np.int32)
    closest[qi] = tri_dist_f32(pq, a[arg], b[arg], c[arg])[3]
    return dist2, face, closest, header


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def grid_mesh(n=40, seed=5, offset=0.0, extent=2.0):
    """A perturbed n x n height field over [0, extent]^2: (vertices float32 [(n+1)^2,3], faces int32 [2 n^2,3])."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0, extent, n + 1), np.linspace(0, extent, n + 1), indexing="ij")
    z = 0.3 * np.sin(3 * u) * np.cos(2 * v) + rng.normal(0, 0.01, u.shape)
    xy = rng.uniform(-0.2, 0.2, (2,) + u.shape) * (extent / n)
    verts = np.stack([u + xy[0], v + xy[1], z], axis=-1).reshape(-1, 3) + offset
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    k = (i * (n + 1) + j).reshape(-1)
    faces = np.concatenate([np.stack([k, k + n + 1, k + 1], 1), np.stack([k + 1, k + n + 1, k + n + 2], 1)])
    return verts.astype(np.float32), faces.astype(np.int32)


def with_walls(verts, faces, factor=50.0):
    """... plus two triangles `factor` times the grid's extent (a floor under it)."""
    lo, hi = verts.min(0), verts.max(0)
    s = factor * float((hi - lo).max())
    c = (lo + hi) / 2
    wall = np.float32([[c[0] - s, c[1] - s, lo[2] - 0.5], [c[0] + s, c[1] - s, lo[2] - 0.5], [c[0] + s, c[1] + s, lo[2] - 0.5],
                       [c[0] - s, c[1] + s, lo[2] - 0.5]])
    n = verts.shape[0]
    return np.concatenate([verts, wall]), np.concatenate([faces, np.int32([[n, n + 1, n + 2], [n, n + 2, n + 3]])])


def with_slivers(verts, faces, count=100, aspect=1e4, seed=9):
    """... plus `count` slivers of that aspect ratio and an exact duplicate of every tenth face."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.2, 1.8, (count, 3)) * np.float32([1, 1, 0.2])
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = np.cross(d, rng.normal(size=(count, 3)))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    tri = np.stack([base, base + 0.5 * d, base + 0.25 * d + (0.5 / aspect) * e], axis=1).reshape(-1, 3)
    n = verts.shape[0]
    idx = (n + np.arange(3 * count)).reshape(count, 3)
    return np.concatenate([verts, tri.astype(np.float32)]), np.concatenate([faces, idx.astype(np.int32), faces[::10]])


def nan_sliver():
    """A valid face with a query for which the edge branch divides 0 by 0: edge ab is 1e-23 long, so ab.ab = 1e-46 underflows to 0 and with
    it d1 = +0 and d3 = -0 for a query over the plane x = 0, while n = ab x ac = (0, 0, 1e-22) keeps n.n = 1e-44 > 0 (a float32
    subnormal).  Region 2 is taken (vc = 0, d1 >= 0, d3 <= 0) and v = 0 / 0.  (vertices, faces, query)."""
    verts = np.float32([[0, 0, 0], [1e-23, 0, 0], [0, 10, 0]])
    return verts, np.int32([[0, 1, 2]]), np.float32([[0, 5, 1]])


def clamp_cases(seed=0, tries=20000):
    """Faces and queries on which the clamp D = fmaxf(E, B) is ACTIVE — B(p, aabb(f)) > E(p, f): random triangles in [-1, 3]^3 with the
    query up to three float32 steps off corner c per axis, where E's rounding error is of the size of E itself (E is often 0 or a
    fraction of the box distance); the pairs with D != E are kept.  (vertices float32 [3 n,3], faces int32 [n,3], queries float32
    [n,3]): query i belongs to face i; the faces are also each other's far candidates."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.uniform(-1, 3, (tries, 3)).astype(np.float32) for _ in range(3))
    p, k = c.copy(), rng.integers(-3, 4, (tries, 3))
    for _ in range(3):
        up, down = np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))
        p, k = np.where(k > 0, up, np.where(k < 0, down, p)), k - np.sign(k)
    D, E = tri_dist_f32(p, a, b, c)[:2]
    rows = np.nonzero((D != E) & face_validity(np.concatenate([a, b, c]), np.arange(3 * tries).reshape(3, tries).T)[0])[0]
    verts = np.stack([a[rows], b[rows], c[rows]], axis=1).reshape(-1, 3)
    return verts, np.arange(3 * rows.size, dtype=np.int32).reshape(-1, 3), p[rows]


def queries(verts, faces, n_random, seed=3, pad=0.25):
    """Random points in the padded box, then points exactly on vertices, edge midpoints and centroids, then points 1e3 extents away."""
    rng = np.random.default_rng(seed)
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    q = [rng.uniform(lo - pad * ext, hi + pad * ext, (n_random, 3))]
    f = faces[rng.integers(0, faces.shape[0], 12)]
    a, b, c = (verts[f[:, k]].astype(np.float32) for k in range(3))
    q += [a, (a + b) * np.float32(0.5), ((a + b) + c) / np.float32(3)]
    q.append((lo + hi) / 2 + 1e3 * ext * np.float64([[1, 0, 0], [0, -1, 0], [0.6, 0.0, 0.8], [-1, -1, -1]]))
    return np.concatenate([np.asarray(t, np.float32) for t in q])


def sample_mesh(verts, faces, n, seed):
    """n points on the mesh, area-weighted, float32 (numpy's own draw: the tests need points on a surface, not dqo_mesh_sample's bytes)."""
    rng = np.random.default_rng(seed)
    a, b, c = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rng.choice(faces.shape[0], n, p=area / area.sum())
    u, v = rng.uniform(size=(2, n))
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    return (a[f] + u[:, None] * (b[f] - a[f]) + v[:, None] * (c[f] - a[f])).astype(np.float32)


def room_meshes(seed=4):
    """The eval fixture: gt = the six walls of a 4 x 3 x 2.5 m room, each a 16 x 16 grid (3072 faces; the floor ALSO as two big triangles
    would hide nothing, so it is not added); rec = the same room on a 13 x 13 grid with N(0, 0.008) noise on the vertices and a 0.3 m
    bump on one wall.  ((gt vertices, gt faces), (rec vertices, rec faces))."""
    rng = np.random.default_rng(seed)
    size = np.array([4.0, 3.0, 2.5])

    def box(n, noise):
        vs, fs, base = [], [], 0
        u, v = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        k = (i * (n + 1) + j).reshape(-1)
        quad = np.concatenate([np.stack([k, k + n + 1, k + 1], 1), np.stack([k + 1, k + n + 1, k + n + 2], 1)])
        for axis in range(3):
            for side in (0.0, 1.0):
                w = np.zeros(u.shape + (3,))
                w[..., axis], w[..., (axis + 1) % 3], w[..., (axis + 2) % 3] = side, u, v
                vs.append((w * size).reshape(-1, 3))
                fs.append(quad + base)
                base += (n + 1) ** 2
        verts = np.concatenate(vs)
        if noise:
            verts = verts + rng.normal(0, noise, verts.shape)
            near = np.linalg.norm(verts - np.array([0.0, 1.5, 1.2]), axis=1) < 0.6
            verts[near, 0] += 0.3
        return verts.astype(np.float32), np.concatenate(fs).astype(np.int32)

    return box(16, 0.0), box(13, 0.008)
