"""numpy float32 restatement of csrc/map_tsdf.hip: the integration of one RGB-D frame into a dense uniform TSDF volume and the
extraction of a welded, indexed, coloured triangle mesh from it by marching tetrahedra on the Kuhn decomposition of every cube.

The integration rule follows open3d's UniformTSDFVolume integrate as published; the library does not exist on this platform, so the
text of include/dqo_raster.h defines the rule and this file is the oracle.  Every float statement is float32, one rounding per
operation, left to right, division and square root correctly rounded (numpy's are).

Conventions shared with the kernels:
  - the grid is [nz,ny,nx], x fastest; lattice point (x, y, z) has linear index (z * ny + y) * nx + x and centre
    origin + (index + 0.5) * L;
  - a cube is named by its lowest lattice point o and is valid iff all eight weights are > 0;
  - the corner o + (dx, dy, dz) has code dx + 2 dy + 4 dz; the seven edge types are the offsets EDGE_OFFSETS, in that order (three
    axes, three face diagonals, the body diagonal), an edge is owned by its lower lattice point;
  - tetrahedron k of a cube belongs to the k-th permutation p of (0, 1, 2) in lexicographic order, path corners c0 = o,
    c1 = c0 + e[p0], c2 = c1 + e[p1], c3 = o + (1, 1, 1); bit i of a case is set when path corner i is negative (tsdf < 0; 0 is
    positive);
  - a triangle's last two indices are swapped iff bit `case` of FLIP_MASK differs from the parity of p.
"""
import itertools

import numpy as np

f32 = np.float32

EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
TYPE_OF_CODE = {dx + 2 * dy + 4 * dz: t for t, (dx, dy, dz) in enumerate(EDGE_OFFSETS)}
PERMS = tuple(itertools.permutations((0, 1, 2)))
PERM_PARITY = tuple(sum(1 for i in range(3) for j in range(i + 1, 3) if p[i] > p[j]) & 1 for p in PERMS)
# bit `case` set: an EVEN permutation's triangles of that case have their last two indices swapped (test_tsdf_oracle.py regenerates it
# from the geometric rule: the right-hand normal points to the positive corners)
FLIP_MASK = 0x4D24


def path_codes(k):
    """The corner codes of tetrahedron k's path corners c0..c3."""
    p = PERMS[k]
    return (0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7)


def case_triangles(case):
    """The triangles of a tetrahedron case before the flip: a list of triangles, each three (negative corner, positive corner) pairs of
    path-corner indices."""
    neg = [i for i in range(4) if (case >> i) & 1]
    pos = [i for i in range(4) if not (case >> i) & 1]
    if len(neg) == 1:
        return [[(neg[0], b) for b in pos]]
    if len(neg) == 3:
        return [[(a, pos[0]) for a in neg]]
    if len(neg) == 2:
        q = [(neg[0], pos[0]), (neg[0], pos[1]), (neg[1], pos[1]), (neg[1], pos[0])]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def flipped(k, case):
    return bool(((FLIP_MASK >> case) & 1) ^ PERM_PARITY[k])


# ---- integrate ------------------------------------------------------------------------------------------------------------------------
def clear(dims):
    nx, ny, nz = dims
    return dict(tsdf=np.ones((nz, ny, nx), f32), weight=np.zeros((nz, ny, nx), f32), color=np.zeros((3, nz, ny, nx), f32))


def centres(origin, L, dims):
    """(pw_x [nx], pw_y [ny], pw_z [nz]): origin_a + ((float)i_a + 0.5f) * L."""
    L = f32(L)
    return tuple(f32(origin[a]) + (np.arange(dims[a], dtype=f32) + f32(0.5)) * L for a in range(3))


def integrate(vol, origin, L, sdf_trunc, depth, color, fx, fy, cx, cy, w2c, depth_trunc):
    """One frame into vol (a dict of clear()'s arrays, updated in place).  depth [H,W] metres, color [3,H,W], w2c [4,4] row major."""
    tsdf, weight, col = vol["tsdf"], vol["weight"], vol["color"]
    nz, ny, nx = tsdf.shape
    H, W = depth.shape
    fx, fy, cx, cy, sdf_trunc, depth_trunc = f32(fx), f32(fy), f32(cx), f32(cy), f32(sdf_trunc), f32(depth_trunc)
    m = np.asarray(w2c, f32).reshape(4, 4)
    px, py, pz = centres(origin, L, (nx, ny, nz))
    X = np.broadcast_to(px[None, None, :], (nz, ny, nx))
    Y = np.broadcast_to(py[None, :, None], (nz, ny, nx))
    Z = np.broadcast_to(pz[:, None, None], (nz, ny, nx))
    with np.errstate(all="ignore"):
        pc = [((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3] for r in range(3)]
        ok = pc[2] > 0
        uf = ((pc[0] * fx) / pc[2] + cx) + f32(0.5)
        vf = ((pc[1] * fy) / pc[2] + cy) + f32(0.5)
        eps = f32(0.0001)
        ok &= (uf >= eps) & (uf < f32(W) - eps) & (vf >= eps) & (vf < f32(H) - eps)
        u = np.where(ok, uf, 0).astype(np.int32)
        v = np.where(ok, vf, 0).astype(np.int32)
        d = depth.astype(f32)[v, u]
        ok &= (d > 0) & (d <= depth_trunc)
        a = (u.astype(f32) - cx) / fx
        b = (v.astype(f32) - cy) / fy
        mult = np.sqrt((f32(1.0) + a * a) + b * b)
        sdf = (d - pc[2]) * mult
        ok &= sdf > -sdf_trunc
        t = np.minimum(f32(1.0), sdf / sdf_trunc)
        w = weight.copy()
        w1 = w + f32(1.0)
        tsdf[ok] = ((tsdf * w + t) / w1)[ok]
        for c in range(3):
            col[c][ok] = ((col[c] * w + color[c].astype(f32)[v, u]) / w1)[ok]
        weight[ok] = w1[ok]
    assert tsdf.dtype == f32 and weight.dtype == f32 and col.dtype == f32
    return vol


# ---- extract --------------------------------------------------------------------------------------------------------------------------
def _shift(a, d, fill):
    """b[z,y,x] = a[z+dz, y+dy, x+dx] for d = (dx,dy,dz) with entries in {-1,0,1}; `fill` outside."""
    nz, ny, nx = a.shape
    b = np.full_like(a, fill)
    src = [slice(max(0, s), n + min(0, s)) for s, n in zip((d[2], d[1], d[0]), (nz, ny, nx))]
    dst = [slice(max(0, -s), n + min(0, -s)) for s, n in zip((d[2], d[1], d[0]), (nz, ny, nx))]
    b[tuple(dst)] = a[tuple(src)]
    return b


def extract(tsdf, weight, color, origin, L, cap_vertices=None, cap_faces=None):
    """dict(vertices float32 [V,3], colors float32 [V,3], faces int32 [F,3], header int32 [4]) of the volume: vertices ascending by
    (lattice linear index, edge type), faces ascending by (cube linear index, tetrahedron, triangle).  With caps: the vertex list cut at
    cap_vertices, the faces that name a cut vertex removed, the rest cut at cap_faces; header = written / dropped counts."""
    tsdf, weight = np.asarray(tsdf, f32), np.asarray(weight, f32)
    nz, ny, nx = tsdf.shape
    N = nx * ny * nz
    neg = tsdf < 0
    wpos = weight > 0
    valid = np.ones((nz, ny, nx), bool)
    for code in range(8):
        valid &= _shift(wpos, (code & 1, (code >> 1) & 1, (code >> 2) & 1), False)
    # an edge carries a vertex iff its ends differ in sign and some valid cube contains it (a valid cube's weights are all > 0)
    has = np.zeros((nz, ny, nx, 7), bool)
    for t, d in enumerate(EDGE_OFFSETS):
        anyv = np.zeros((nz, ny, nx), bool)
        for s in itertools.product((0, 1), repeat=3):
            if any(s[a] and d[a] for a in range(3)):
                continue
            anyv |= _shift(valid, (-s[0], -s[1], -s[2]), False)
        has[..., t] = anyv & (neg != _shift(neg, d, False))
    flat = has.reshape(-1)
    vid = (np.cumsum(flat) - flat).astype(np.int64).reshape(nz, ny, nx, 7)  # the id of edge (lattice point, type) where it has one
    V = int(flat.sum())
    # vertices
    zz, yy, xx, tt = np.nonzero(has)  # (row-major: ascending lattice index, then type)
    off = np.asarray(EDGE_OFFSETS)[tt]
    x2, y2, z2 = xx + off[:, 0], yy + off[:, 1], zz + off[:, 2]
    px, py, pz = centres(origin, L, (nx, ny, nz))
    lo_neg = neg[zz, yy, xx]
    ax, ay, az = np.where(lo_neg, xx, x2), np.where(lo_neg, yy, y2), np.where(lo_neg, zz, z2)
    bx, by, bz = np.where(lo_neg, x2, xx), np.where(lo_neg, y2, yy), np.where(lo_neg, z2, zz)
    fa, fb = tsdf[az, ay, ax], tsdf[bz, by, bx]
    s = fa / (fa - fb)
    lerp = lambda pa, pb: pa + s * (pb - pa)
    vertices = np.stack([lerp(px[ax], px[bx]), lerp(py[ay], py[by]), lerp(pz[az], pz[bz])], 1).astype(f32).reshape(-1, 3)
    color = np.asarray(color, f32)
    colors = np.stack([lerp(color[c][az, ay, ax], color[c][bz, by, bx]) for c in range(3)], 1).astype(f32).reshape(-1, 3)
    # faces
    cz, cy_, cx_ = np.nonzero(valid)
    clin = (cz * ny + cy_) * nx + cx_
    recs = []
    for k in range(6):
        codes = path_codes(k)
        corner = [(cx_ + (c & 1), cy_ + ((c >> 1) & 1), cz + ((c >> 2) & 1)) for c in codes]
        case = sum(neg[corner[i][2], corner[i][1], corner[i][0]].astype(np.int64) << i for i in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if sel.size == 0:
                continue
            for j, tri in enumerate(case_triangles(cs)):
                ids = []
                for (a, b) in tri:
                    lo, hi = min(a, b), max(a, b)
                    t = TYPE_OF_CODE[codes[hi] ^ codes[lo]]
                    ids.append(vid[corner[lo][2][sel], corner[lo][1][sel], corner[lo][0][sel], t])
                    assert has[corner[lo][2][sel], corner[lo][1][sel], corner[lo][0][sel], t].all()
                if flipped(k, cs):
                    ids[1], ids[2] = ids[2], ids[1]
                recs.append(np.stack([clin[sel], np.full(sel.size, k), np.full(sel.size, j)] + ids, 1))
    if recs:
        recs = np.concatenate(recs, 0)
        recs = recs[np.lexsort((recs[:, 2], recs[:, 1], recs[:, 0]))]
        faces = recs[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    F = faces.shape[0]
    cap_v = V if cap_vertices is None else int(cap_vertices)
    cap_f = F if cap_faces is None else int(cap_faces)
    nv = min(V, cap_v)
    kept = faces[(faces < nv).all(1)] if nv < V else faces
    nf = min(kept.shape[0], cap_f)
    return dict(vertices=vertices[:nv], colors=colors[:nv], faces=np.ascontiguousarray(kept[:nf]),
                header=np.array([nv, nf, V - nv, F - nf], np.int32))


# ---- the sphere of the tests ------------------------------------------------------------------------------------------------------------
def sphere_volume(n=24, r=0.31, centre=(0.03, -0.02, 0.011)):
    """The unit box [-0.5, 0.5]^3 in n^3 voxels with tsdf = clip(dist / 3L, -1, 1) of a sphere, all weights 1, colour = the voxel
    centre's position + 0.5.  Returns (origin, L, tsdf, weight, color)."""
    L = f32(1.0 / n)
    origin = (f32(-0.5), f32(-0.5), f32(-0.5))
    px, py, pz = [p.astype(np.float64) for p in centres(origin, L, (n, n, n))]
    X, Y, Z = px[None, None, :], py[None, :, None], pz[:, None, None]
    dist = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    tsdf = np.clip(dist / (3.0 * float(L)), -1.0, 1.0).astype(f32)
    weight = np.ones((n, n, n), f32)
    color = np.stack([np.broadcast_to(a + 0.5, (n, n, n)) for a in (X, Y, Z)]).astype(f32)
    return origin, L, tsdf, weight, color
