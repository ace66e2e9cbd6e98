"""numpy restatement of dqo_mesh_simplify (csrc/map_meshops.hip) — the rule of include/dqo_raster.h: vertex clustering on a grid the
caller places, a cluster's position and colour the average of its members, faces renumbered, collapsed faces and duplicates dropped —
and cluster_extras(), the test mesh with long member lists.  It follows open3d's simplify_vertex_clustering with
SimplificationContraction::Average; the library does not exist on this platform, so the header's text defines the rule and this file
is the oracle.

  - cells: t = ((double)p - origin) / voxel_size per axis, one rounding per operation; i = floor(t); a vertex is in the grid iff the
    three t are finite and 0 <= i < 2^21;
  - a cluster is the set of in-grid vertices of a cell, its representative its smallest vertex id;
  - a face is, in this order, bad (an index outside [0, V)), outside (names a vertex outside the grid), collapsed (two corners in one
    cluster) or live; a live face's triple of representatives is rotated so that the smallest comes first; of the live faces with the
    same rotated triple the lowest face index is kept; kept faces keep their order;
  - a cluster is written iff a live face names it; written clusters are numbered densely in ascending representative id;
  - position and colour: S = 0, S = S + (double)p_m over the members in ascending vertex id (np.add.at adds one index after the
    other, in the order given — a pairwise np.sum would not), (float)(S / (double)n); a cluster of one member is copied.

Grouping and deduplication are stated twice, independently: group_by_dict (dictionaries in a Python loop) and group_by_unique (np.unique
on cell triples and rotated triples); simplify() takes either, tests/test_mesh_simplify_oracle.py holds them to each other."""
import functools

import numpy as np

from mesh_ops_oracle import archipelago, smoothing_extras, sphere, valid_faces  # noqa: F401  (the builders the tests share)

f32, f64 = np.float32, np.float64
HEADER = ("vertices", "faces", "clusters", "vertices_outside", "faces_bad_index", "faces_outside", "faces_collapsed", "faces_duplicate")
GRID = 1 << 21


def cells(vertices, voxel_size, origin):
    """(cell int64 [V,3], inside bool [V]); the cell of a vertex outside the grid is meaningless."""
    p = np.asarray(vertices, f32).astype(f64)
    with np.errstate(all="ignore"):
        t = (p - np.asarray(origin, f64)[None, :]) / f64(voxel_size)
        i = np.floor(t)
        inside = (np.isfinite(t) & (i >= 0) & (i < GRID)).all(1)
    cell = np.zeros(p.shape, np.int64)
    cell[inside] = i[inside].astype(np.int64)
    return cell, inside


def rotate(tri):
    """[n,3] triples rotated so that the smallest entry of each comes first (the cyclic order, and so the orientation, stays)."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k = tri.argmin(1)
    rows = np.arange(len(tri))
    return np.stack([tri[rows, k], tri[rows, (k + 1) % 3], tri[rows, (k + 2) % 3]], 1)


def group_by_dict(cell, inside, faces):
    """(rep int64 [V] (-1 outside the grid), state int8 [F]: 0 bad, 1 outside, 2 collapsed, 3 duplicate, 4 kept; tri int64 [F,3] rotated
    representatives of the live faces) — by dictionaries, one vertex and one face after the other."""
    V = len(cell)
    first, rep = {}, np.full(V, -1, np.int64)
    for v in range(V):
        if inside[v]:
            key = (int(cell[v, 0]), int(cell[v, 1]), int(cell[v, 2]))
            rep[v] = first.setdefault(key, v)  # (ascending v: the first of a cell is its smallest id)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    state, tri, seen = np.zeros(len(faces), np.int8), np.zeros((len(faces), 3), np.int64), set()
    for f, (a, b, c) in enumerate(faces.tolist()):
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V):
            state[f] = 0
        elif not (inside[a] and inside[b] and inside[c]):
            state[f] = 1
        elif rep[a] == rep[b] or rep[b] == rep[c] or rep[a] == rep[c]:
            state[f] = 2
        else:
            r = [int(rep[a]), int(rep[b]), int(rep[c])]
            k = r.index(min(r))
            t = (r[k], r[(k + 1) % 3], r[(k + 2) % 3])
            tri[f] = t
            state[f] = 3 if t in seen else 4
            seen.add(t)
    return rep, state, tri


def group_by_unique(cell, inside, faces):
    """The same, by np.unique on the cell triples and on the rotated triples."""
    V = len(cell)
    rep = np.full(V, -1, np.int64)
    ids = np.nonzero(inside)[0]
    if len(ids):
        _, first, inverse = np.unique(cell[ids], axis=0, return_index=True, return_inverse=True)
        rep[ids] = ids[first[inverse.ravel()]]  # (return_index: the first occurrence, ids ascend)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    state, tri = np.zeros(len(faces), np.int8), np.zeros((len(faces), 3), np.int64)
    ok = valid_faces(V, faces)
    fin = ok.copy()
    fin[ok] = inside[faces[ok]].all(1)
    state[ok & ~fin] = 1
    r = np.full((len(faces), 3), -1, np.int64)
    r[fin] = rep[faces[fin]]
    live = fin & (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    state[fin & ~live] = 2
    lid = np.nonzero(live)[0]
    if len(lid):
        t = rotate(r[lid])
        tri[lid] = t
        _, first = np.unique(t, axis=0, return_index=True)
        state[lid] = 3
        state[lid[first]] = 4
    return rep, state, tri


def simplify(vertices, colors, faces, voxel_size, origin=(0.0, 0.0, 0.0), group=group_by_unique):
    """dict(vertices, colors (or None), faces, header int32 [8], members int64 [clusters written]: their sizes) — dqo_mesh_simplify."""
    vertices = np.asarray(vertices, f32)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(vertices)
    cell, inside = cells(vertices, voxel_size, origin)
    rep, state, tri = group(cell, inside, faces)
    kept = tri[state == 4]
    live = tri[state >= 3]
    written = np.zeros(V, bool)
    written[live.ravel()] = True  # (a duplicate names the clusters of the face it repeats)
    number = np.cumsum(written) - written  # the dense id of a written representative
    nw = int(written.sum())
    member = inside & written[np.where(inside, rep, 0)]
    ids = np.nonzero(member)[0]  # ascending vertex id
    cid = number[rep[ids]]
    n = np.bincount(cid, minlength=nw)

    def average(values):
        x = np.asarray(values, f32)
        S = np.zeros((nw, 3), f64)
        with np.errstate(all="ignore"):
            np.add.at(S, cid, x[ids].astype(f64))
            out = (S / n.astype(f64)[:, None]).astype(f32)
        single = n[cid] == 1
        out[cid[single]] = x[ids[single]]  # a cluster of one member: copied, whatever its bits
        return out

    header = np.array([nw, len(kept), len(np.unique(rep[inside])), V - inside.sum(), (state == 0).sum(), (state == 1).sum(), (state == 2).sum(),
                       (state == 3).sum()], np.int32)
    return dict(vertices=average(vertices), colors=None if colors is None else average(colors),
                faces=np.ascontiguousarray(number[kept].astype(np.int32).reshape(-1, 3)), header=header, members=n, rep=rep, state=state)


# ---- the test mesh with long member lists ---------------------------------------------------------------------------------------------
GROUPS = (1, 2, 32, 33, 2048, 2049, 2600)  # members of a cluster: both sides of what a thread sorts (32) and of what a block sorts in LDS (2048)
EXTRAS_CELL = 0.25  # cluster_extras()'s own cell size, its grid at (0, 0, 0)


@functools.lru_cache(maxsize=1)
def cluster_extras(seed=31):
    """Groups of GROUPS vertices, group g inside the cell (4 g, 1, 1) of a grid of EXTRAS_CELL at the origin, every vertex of a group in
    a triangle with the group's two anchor vertices, which sit in two other cells: a group of n gives one kept face and n - 1
    duplicates.  One vertex with a NaN coordinate, three at negative cell indices and a face naming each; two faces with a bad index
    (-1 and V); an unreferenced vertex; vertex ids permuted, faces shuffled.  Returns dict(vertices, colors, faces, groups: the new
    ids of every group's members)."""
    rng = np.random.default_rng(seed)
    L = EXTRAS_CELL
    verts, faces, groups = [], [], []
    n = 0
    for g, size in enumerate(GROUPS):
        base = np.array([4 * g, 1, 1], f64) * L
        verts.append(base + rng.uniform(0.1, 0.9, size=(size, 3)) * L)
        verts.append(np.stack([base + [1.5 * L, 0.5 * L, 0.5 * L], base + [0.5 * L, 1.5 * L, 0.5 * L]]) + rng.uniform(-0.2, 0.2, size=(2, 3)) * L)
        m = np.arange(n, n + size)
        faces.append(np.stack([m, np.full(size, n + size), np.full(size, n + size + 1)], 1))
        groups.append(m)
        n += size + 2
    anchor = n - 2  # (in-grid vertices the faces of the outsiders name as well)
    outsiders = np.array([[np.nan, 0.3, 0.3], [-0.1 * L, 0.4, 0.4], [0.6, -3.0, 0.2], [0.7, 0.7, -1e-6], [0.123, 0.456, 0.789]])  # (the last: unreferenced)
    verts.append(outsiders)
    faces.append(np.stack([np.arange(n, n + 4), np.full(4, anchor), np.full(4, anchor + 1)], 1))
    n += len(outsiders)
    V = n
    verts = np.concatenate(verts)
    faces = np.concatenate(faces + [np.array([[-1, 3, 7], [11, V, 2]])])
    perm = rng.permutation(V)  # old id -> new id
    new_v = np.empty_like(verts)
    new_v[perm] = verts
    good = (faces >= 0) & (faces < V)
    faces = np.where(good, perm[np.clip(faces, 0, V - 1)], faces)
    faces = faces[rng.permutation(len(faces))]
    colors = rng.uniform(0.0, 1.0, size=(V, 3))
    return dict(vertices=new_v.astype(f32), colors=colors.astype(f32), faces=np.ascontiguousarray(faces, np.int32),
                groups=[np.sort(perm[m]) for m in groups])
