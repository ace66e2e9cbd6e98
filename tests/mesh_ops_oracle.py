"""numpy restatement of csrc/map_meshops.hip — the rules of include/dqo_raster.h for dqo_mesh_components, dqo_mesh_smooth and
dqo_mesh_normals — and the builders of the test meshes.

open3d (cluster_connected_triangles, filter_smooth_laplacian / filter_smooth_taubin, compute_vertex_normals) does not exist on this
platform, so the header's text defines the rules and this file is the oracle.  A face is valid iff its three indices lie in [0, V).
  - components: a min-label union over shared vertex INDICES (open3d clusters by shared edges: the two differ at pinch vertices only);
    a component's label is its smallest vertex id, its size its number of faces;
  - smoothing: in double from the float32 values of the step before, one rounding per operation, sums from 0 over the ascending
    neighbours ONE NEIGHBOUR SLOT AT A TIME (slot k of every vertex that has one is added in one numpy statement, which keeps each
    vertex's own order), the result rounded to float32 after every step;
  - normals: the same, one incident-face slot at a time, ascending face index, a face once per corner that names the vertex.
numpy's double `/` and sqrt are correctly rounded and it never contracts a multiply and an add.
"""
import functools

import numpy as np

import tsdf_oracle

f32, f64 = np.float32, np.float64
HEADER = ("vertices", "faces", "components", "components_kept", "faces_bad_index", "largest_component_faces", "vertices_removed",
          "faces_removed")


def valid_faces(V, faces):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < V)).all(1)


# ---- components -------------------------------------------------------------------------------------------------------------------------
def vertex_labels(V, faces):
    """label[v] = the smallest vertex id of v's set, sets united through the valid faces: every face pulls its three labels down to
    their minimum, labels jump to their label's label, until nothing moves."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = faces[valid_faces(V, faces)]
    label = np.arange(V, dtype=np.int64)
    while True:
        new = label.copy()
        if len(fv):
            m = label[fv].min(1)
            np.minimum.at(new, fv.ravel(), np.repeat(m, 3))
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def components(vertices, colors, faces, min_faces=0, largest_only=False):
    """dict(labels int32 [F] (-1: a bad face), header int32 [8], vertices, colors (or None), faces) — dqo_mesh_components."""
    vertices = np.asarray(vertices, f32)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(vertices), len(faces)
    ok = valid_faces(V, faces)
    vl = vertex_labels(V, faces)
    labels = np.full(F, -1, np.int64)
    labels[ok] = vl[faces[ok, 0].astype(np.int64)]
    size = np.bincount(labels[ok], minlength=V)  # per root
    ncomp = int((size > 0).sum())
    largest = int(size.max()) if V else 0
    thr = max(int(min_faces), largest if largest_only else 0)
    keep = ok.copy()
    keep[ok] = size[labels[ok]] >= thr
    kept_comp = int(((size > 0) & (size >= thr)).sum())
    used = np.zeros(V, bool)
    used[faces[keep].astype(np.int64).ravel()] = True
    remap = np.cumsum(used) - used
    out_faces = remap[faces[keep].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    header = np.array([used.sum(), keep.sum(), ncomp, kept_comp, (~ok).sum(), largest, V - used.sum(), ok.sum() - keep.sum()], np.int32)
    return dict(labels=labels.astype(np.int32), header=header, vertices=vertices[used], colors=None if colors is None else np.asarray(colors, f32)[used],
                faces=np.ascontiguousarray(out_faces))


def bfs_partition(V, faces):
    """The partition of the valid faces by a plain breadth-first search over faces that share a vertex — independent of vertex_labels.
    Returns a list of sorted face-index lists, sorted."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(V, faces)
    at = [[] for _ in range(V)]
    for f in np.nonzero(ok)[0]:
        for v in set(faces[f].tolist()):
            at[v].append(int(f))
    seen, parts = set(), []
    for f0 in np.nonzero(ok)[0]:
        if int(f0) in seen:
            continue
        seen.add(int(f0))
        part, queue = [], [int(f0)]
        while queue:
            f = queue.pop()
            part.append(f)
            for v in faces[f].tolist():
                for g in at[v]:
                    if g not in seen:
                        seen.add(g)
                        queue.append(g)
                at[v] = []
        parts.append(sorted(part))
    return sorted(parts)


# ---- adjacency --------------------------------------------------------------------------------------------------------------------------
def neighbours(V, faces):
    """(indptr [V+1], idx): N(i) ascending, each neighbour once, i itself excluded, over the valid faces."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = faces[valid_faces(V, faces)]
    a = np.concatenate([fv[:, [0, 1]], fv[:, [0, 2]], fv[:, [1, 0]], fv[:, [1, 2]], fv[:, [2, 0]], fv[:, [2, 1]]]) if len(fv) else np.zeros((0, 2), np.int64)
    a = a[a[:, 0] != a[:, 1]]
    key = np.unique(a[:, 0] * V + a[:, 1])
    i, n = key // V, key % V
    indptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=V), out=indptr[1:])
    return indptr, n


def corner_faces(V, faces):
    """(indptr [V+1], idx): the faces of a vertex's corners, ascending face index, a face once per corner that names the vertex."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fid = np.nonzero(valid_faces(V, faces))[0]
    vert, face = faces[fid].ravel(), np.repeat(fid, 3)
    order = np.lexsort((face, vert))
    indptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=indptr[1:])
    return indptr, face[order]


# ---- smoothing --------------------------------------------------------------------------------------------------------------------------
def smooth_step(p32, c32, indptr, idx, lam, pos=True, col=True):
    """One step with factor lam: (positions, colours) float32 after it."""
    p = p32.astype(f64)
    c = None if c32 is None else c32.astype(f64)
    V = len(p)
    deg = np.diff(indptr)
    S, C, T = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    for k in range(int(deg.max()) if V else 0):
        rows = np.nonzero(deg > k)[0]
        nb = idx[indptr[rows] + k]
        d = p[rows] - p[nb]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        w = 1.0 / (dist + 1e-12)
        if pos:
            S[rows] = S[rows] + w[:, None] * p[nb]
        if col:
            C[rows] = C[rows] + w[:, None] * c[nb]
        T[rows] = T[rows] + w
    has = deg > 0
    new_p, new_c = p32, c32
    with np.errstate(all="ignore"):
        if pos:
            new_p = p32.copy()
            new_p[has] = (p[has] + lam * (S[has] / T[has][:, None] - p[has])).astype(f32)
        if col:
            new_c = c32.copy()
            new_c[has] = (c[has] + lam * (C[has] / T[has][:, None] - c[has])).astype(f32)
    return new_p, new_c


def smooth(vertices, colors, faces, iterations, lam=0.5, mu=0.0, scope="all"):
    """(positions, colours) after dqo_mesh_smooth: scope "positions", "colors" or "all" (positions only when colors is None)."""
    p = np.asarray(vertices, f32).copy()
    c = None if colors is None else np.asarray(colors, f32).copy()
    pos, col = scope in ("positions", "all"), scope in ("colors", "all") and c is not None
    indptr, idx = neighbours(len(p), faces)
    for _ in range(int(iterations)):
        p, c = smooth_step(p, c, indptr, idx, f64(lam), pos, col)
        if mu:
            p, c = smooth_step(p, c, indptr, idx, f64(mu), pos, col)
    return p, c


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def normals(vertices, faces):
    """float32 [V,3]: dqo_mesh_normals."""
    p = np.asarray(vertices, f32).astype(f64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(p)
    ok = valid_faces(V, faces)
    fn = np.zeros((len(faces), 3))
    p0, p1, p2 = (p[faces[ok, k]] for k in range(3))
    u, v = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        fn[ok] = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        indptr, idx = corner_faces(V, faces)
        deg = np.diff(indptr)
        s = np.zeros((V, 3))
        for k in range(int(deg.max()) if V else 0):
            rows = np.nonzero(deg > k)[0]
            s[rows] = s[rows] + fn[idx[indptr[rows] + k]]
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = (length > 0) & np.isfinite(length)
        out = np.zeros((V, 3), f32)
        out[:, 2] = 1.0
        out[good] = (s[good] / length[good][:, None]).astype(f32)
    return out


def enclosed_volume(vertices, faces):
    """The signed volume a closed mesh encloses (double; the sum of det(p0, p1, p2) / 6)."""
    p = np.asarray(vertices, f64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


# ---- the test meshes --------------------------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_C = 0.31, np.array([0.03, -0.02, 0.011])


@functools.lru_cache(maxsize=1)
def sphere():
    """The TSDF oracle's sphere as a mesh dict: 3132 vertices, 6260 faces, one closed component."""
    origin, length, tsdf, weight, color = tsdf_oracle.sphere_volume()
    m = tsdf_oracle.extract(tsdf, weight, color, origin, length)
    return dict(vertices=m["vertices"], colors=m["colors"], faces=m["faces"])


TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
OCTA = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
STRIP = 700


@functools.lru_cache(maxsize=1)
def archipelago(seed=11):
    """The sphere plus five closed tetrahedra (4 faces each), an octahedron (8), a lone triangle (1), a strip of 700 triangles whose
    vertex ids DESCEND along the strip with a repeated-index face attached (701 faces), nine unreferenced vertices and two faces with a
    bad index (-1 and V); then the vertex ids are permuted and the faces shuffled.  Returns dict(vertices, colors, faces, sizes)."""
    rng = np.random.default_rng(seed)
    s = sphere()
    verts, faces = [s["vertices"].astype(f64)], [s["faces"].astype(np.int64)]
    n = len(s["vertices"])

    def add(v, f):
        nonlocal n
        verts.append(np.asarray(v, f64))
        faces.append(np.asarray(f, np.int64) + n)
        n += len(v)

    for k in range(5):
        add(rng.normal(size=(4, 3)) * 0.02 + [0.45, -0.4 + 0.2 * k, 0.4], TETRA)
    add(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.03 + [-0.45, 0.4, -0.4], OCTA)
    add(rng.normal(size=(3, 3)) * 0.02 + [-0.45, -0.45, 0.45], [[0, 1, 2]])
    j = np.arange(STRIP + 2)
    strip_v = np.stack([-0.48 + 0.96 * j / (STRIP + 1), 0.46 + 0.01 * (j & 1), np.full(len(j), -0.46)], 1) + rng.normal(size=(STRIP + 2, 3)) * 1e-4
    ids = STRIP + 1 - j  # the vertex at place j along the strip has the id STRIP + 1 - j
    order = np.argsort(ids)
    t = np.arange(STRIP)
    strip_f = np.stack([ids[t], ids[t + 1], ids[t + 2]], 1)
    strip_f[1::2] = strip_f[1::2][:, [0, 2, 1]]
    strip_f = np.concatenate([strip_f, [[ids[0], ids[0], ids[1]]]])
    add(strip_v[order], strip_f)
    verts.append(rng.uniform(-0.5, 0.5, size=(9, 3)))  # unreferenced
    n += 9
    V = n
    verts = np.concatenate(verts)
    faces = np.concatenate(faces + [np.array([[-1, 5, 9], [17, V, 4]])])
    perm = rng.permutation(V)  # old id -> new id
    new_v = np.empty_like(verts)
    new_v[perm] = verts
    inside = (faces >= 0) & (faces < V)
    faces = np.where(inside, perm[np.clip(faces, 0, V - 1)], faces)
    faces = faces[rng.permutation(len(faces))]
    colors = rng.uniform(0.0, 1.0, size=(V, 3))
    return dict(vertices=new_v.astype(f32), colors=colors.astype(f32), faces=np.ascontiguousarray(faces, np.int32),
                sizes=sorted([6260, 4, 4, 4, 4, 4, 8, 1, 701]))


def fan(n, centre, radius, lift=0.0):
    """(vertices [n+1,3] double, faces [n,3]): hub 0 at centre + (0, 0, lift), a regular ring of n vertices around centre."""
    a = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n)], 1) + centre
    k = np.arange(n)
    return np.concatenate([[np.asarray(centre, f64) + [0, 0, lift]], ring]), np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1)


@functools.lru_cache(maxsize=1)
def smoothing_extras(seed=23):
    """What the sphere lacks: a 300-triangle fan around one hub (raw degree 600: above what a thread sorts), a 2600-triangle fan (raw
    degree 5200: above what a block sorts in LDS), a 20 x 15 open grid with a hole (boundary vertices) and duplicated faces, a
    zero-area triangle on three vertices of its own, and seven isolated vertices; faces shuffled.
    Returns dict(vertices, colors, faces, hubs, sliver (its three vertices), isolated)."""
    rng = np.random.default_rng(seed)
    verts, faces, n = [], [], 0

    def add(v, f):
        nonlocal n
        first = n
        verts.append(np.asarray(v, f64))
        faces.append(np.asarray(f, np.int64).reshape(-1, 3) + n)
        n += len(v)
        return first

    fv, ff = fan(300, [0.0, 0.0, 0.0], 0.2, lift=0.05)
    hubs = [add(fv + rng.normal(size=fv.shape) * 1e-3, ff)]
    fv, ff = fan(2600, [1.0, 0.0, 0.0], 0.3, lift=-0.1)
    hubs.append(add(fv + rng.normal(size=fv.shape) * 1e-4, ff))
    gx, gy = 20, 15
    X, Y = np.meshgrid(np.arange(gx), np.arange(gy))
    gv = np.stack([0.05 * X.ravel(), 0.05 * Y.ravel(), 0.01 * np.sin(0.7 * X.ravel()) * np.cos(0.5 * Y.ravel())], 1) + [0, 1.0, 0]
    gf = []
    for y in range(gy - 1):
        for x in range(gx - 1):
            if 7 <= x < 11 and 5 <= y < 8:
                continue  # the hole
            a = y * gx + x
            gf += [[a, a + 1, a + gx], [a + 1, a + gx + 1, a + gx]]
    gf = np.array(gf)
    gf = np.concatenate([gf, gf[3:40:3], gf[10:12]])  # duplicated faces
    add(gv + rng.normal(size=gv.shape) * 1e-3, gf)
    sliver = add([[1.0, 2.0, 0.0], [2.0, 2.0, 0.0], [3.0, 2.0, 0.0]], [[0, 1, 2]])
    isolated = add(rng.uniform(-1, 1, size=(7, 3)), np.zeros((0, 3), np.int64))
    verts, faces = np.concatenate(verts), np.concatenate(faces)
    faces = faces[rng.permutation(len(faces))]
    colors = rng.uniform(0.0, 1.0, size=(n, 3))
    return dict(vertices=verts.astype(f32), colors=colors.astype(f32), faces=np.ascontiguousarray(faces, np.int32), hubs=hubs,
                sliver=[sliver, sliver + 1, sliver + 2], isolated=list(range(isolated, isolated + 7)))
