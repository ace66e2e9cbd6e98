"""dqo_mesh_render_depth (include/dqo_raster.h, csrc/map_meshrender.hip) restated in numpy: a triangle mesh rasterised to depth in K
views.  One numpy operation per statement of the header — float32 arrays for a corner's projection and the box, float64 for the edge
functions and the depth — so every rounding is the kernel's; a pixel keeps the minimum uint64 key.  Also the meshes and cameras the
render's tests share."""
import numpy as np

f32, f64 = np.float32, np.float64
HEADER = ("views_used", "faces_bad_index", "pairs_rasterised", "pairs_near_dropped", "pairs_degenerate", "pairs_cooperative", "pixels_hit",
          "zero")
SMALL_MAX = 64  # pixels of a clipped box that one lane walks alone (header word 5 counts the pairs above it)
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)


def intrinsics(K):
    K = np.asarray(K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.tolist())


def _min3(a, b, c):
    m = a
    m = np.where(b < m, b, m)
    return np.where(c < m, c, m)


def _max3(a, b, c):
    m = a
    m = np.where(b > m, b, m)
    return np.where(c > m, c, m)


def render(vertices, faces, w2c, K, W, H, view_keep=None, near=0.0, depth_trunc=np.inf):
    """dict(depth float32 [n,H,W], face_index int32 [n,H,W], header int32 [8], keys uint64 [n,H,W])."""
    p = np.asarray(vertices, f32).reshape(-1, 3)
    V = len(p)
    fc = np.asarray(faces, np.int32).reshape(-1, 3)
    m = np.asarray(w2c, f32).reshape(-1, 4, 4)
    n = len(m)
    fx, fy, cx, cy = (f32(v) for v in intrinsics(K))
    near, depth_trunc = f32(near), f32(depth_trunc)
    keys = np.full((n, H, W), NO_HIT, np.uint64)
    ok = ((fc >= 0) & (fc < V)).all(1)
    ids = np.nonzero(ok)[0]
    v = fc[ids].astype(np.int64)  # [G,3] vertex ids of the valid faces
    repeated = (v[:, 0] == v[:, 1]) | (v[:, 1] == v[:, 2]) | (v[:, 0] == v[:, 2])
    n_rast = n_near = n_degen = n_coop = 0
    used = [k for k in range(n) if view_keep is None or view_keep[k]]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for k in used:
        with np.errstate(all="ignore"):
            pc = np.stack([((m[k, r, 0] * x + m[k, r, 1] * y) + m[k, r, 2] * z) + m[k, r, 3] for r in range(3)], 1)  # [V,3] float32
            assert pc.dtype == f32
            P = pc[v]  # [G, corner, r]
            front = (P[:, :, 2] > near).sum(1)
            n_near += int(((front > 0) & (front < 3)).sum())
            px = (P[:, :, 0] * fx) / P[:, :, 2] + cx
            py = (P[:, :, 1] * fy) / P[:, :, 2] + cy
            assert px.dtype == f32
            x0 = np.ceil(_min3(px[:, 0], px[:, 1], px[:, 2]))
            x1 = np.floor(_max3(px[:, 0], px[:, 1], px[:, 2]))
            y0 = np.ceil(_min3(py[:, 0], py[:, 1], py[:, 2]))
            y1 = np.floor(_max3(py[:, 0], py[:, 1], py[:, 2]))
            x0, y0 = np.where(x0 < 0, f32(0), x0), np.where(y0 < 0, f32(0), y0)
            x1, y1 = np.where(x1 > f32(W - 1), f32(W - 1), x1), np.where(y1 > f32(H - 1), f32(H - 1), y1)
            boxed = (front == 3) & (x0 <= x1) & (y0 <= y1)
        for g in np.nonzero(boxed)[0]:
            with np.errstate(all="ignore"):
                xd, yd, Pd = px[g].astype(f64), py[g].astype(f64), P[g].astype(f64)

                def edge(i, j, X, Y):
                    first = v[g, i] < v[g, j]
                    a, b = (i, j) if first else (j, i)
                    E = (xd[b] - xd[a]) * (Y - yd[a]) - (yd[b] - yd[a]) * (X - xd[a])
                    return E if first else np.negative(E)

                A = edge(0, 1, xd[2], yd[2])
                if repeated[g] or A == 0.0:
                    n_degen += 1
                    continue
                n_rast += 1
                ix0, ix1, iy0, iy1 = int(x0[g]), int(x1[g]), int(y0[g]), int(y1[g])
                bw, bh = ix1 - ix0 + 1, iy1 - iy0 + 1
                if bw > SMALL_MAX or bh > SMALL_MAX or bw * bh > SMALL_MAX:
                    n_coop += 1
                Y, X = np.meshgrid(np.arange(iy0, iy1 + 1, dtype=f64), np.arange(ix0, ix1 + 1, dtype=f64), indexing="ij")
                e0, e1, e2 = edge(0, 1, X, Y), edge(1, 2, X, Y), edge(2, 0, X, Y)
                covered = ((A > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((A < 0) & (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                a, b = Pd[1] - Pd[0], Pd[2] - Pd[0]
                nx, ny, nz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
                np0 = (nx * Pd[0, 0] + ny * Pd[0, 1]) + nz * Pd[0, 2]
                rx, ry = (X - f64(cx)) / f64(fx), (Y - f64(cy)) / f64(fy)
                nr = (nx * rx + ny * ry) + nz
                zz = np0 / nr
                zmin, zmax = f64(_min3(P[g, 0, 2], P[g, 1, 2], P[g, 2, 2])), f64(_max3(P[g, 0, 2], P[g, 1, 2], P[g, 2, 2]))
                zz = np.where(zz < zmin, zmin, zz)
                zz = np.where(zz > zmax, zmax, zz)
                d = zz.astype(f32)
                hit = covered & (nr != 0.0) & (d > near) & (d <= depth_trunc)
                key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ids[g])
                tile = keys[k, iy0:iy1 + 1, ix0:ix1 + 1]
                tile[...] = np.where(hit & (key < tile), key, tile)
    hitmask = keys != NO_HIT
    depth = np.where(hitmask, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    face_index = np.where(hitmask, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    header = np.array([len(used), (~ok).sum(), n_rast, n_near, n_degen, n_coop, int(hitmask.sum()) & 0xFFFFFFFF, 0], np.int64).astype(np.int32)
    return dict(depth=depth, face_index=face_index, header=header, keys=keys)


# ---- meshes and cameras -------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """float32 [4,4] world-to-camera, row major: the camera at `eye` looks along +z at `target`, x to the right, y down."""
    eye, target, up = (np.asarray(a, f64) for a in (eye, target, up))
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(-up, zc)
    if np.linalg.norm(xc) < 1e-9:
        xc = np.cross(np.array([0.0, 0.0, 1.0]), zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, -R @ eye
    return out.astype(f32)


def grid_mesh(nx, ny, origin, du, dv):
    """A welded grid of nx x ny quads (two triangles each) spanned from `origin` by the steps du, dv: (vertices [.,3], faces [.,3])."""
    origin, du, dv = (np.asarray(a, f64) for a in (origin, du, dv))
    j, i = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    verts = origin + i[..., None] * du + j[..., None] * dv
    vid = lambda a, b: b * (nx + 1) + a
    faces = []
    for b in range(ny):
        for a in range(nx):
            faces += [[vid(a, b), vid(a + 1, b), vid(a + 1, b + 1)], [vid(a, b), vid(a + 1, b + 1), vid(a, b + 1)]]
    return verts.reshape(-1, 3).astype(f32), np.array(faces, np.int32)


CUBE_LO, CUBE_HI = np.array([-0.5, -0.5, -0.5]), np.array([0.5, 0.5, 0.5])


def cube_mesh():
    """The unit cube about the origin: 8 vertices, 12 faces."""
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int32)


def ray_box_depth(w2c, K, W, H, lo=CUBE_LO, hi=CUBE_HI):
    """float64 [H,W]: the camera-space z of the first point of the box [lo, hi] along each pixel centre's ray (slab method); 0 = miss."""
    fx, fy, cx, cy = intrinsics(K)
    m = np.asarray(w2c, f64).reshape(4, 4)
    R, t = m[:3, :3], m[:3, 3]
    eye = -R.T @ t
    Y, X = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    rc = np.stack([(X - cx) / fx, (Y - cy) / fy, np.ones_like(X)], -1)  # camera-space rays with z = 1: the parameter IS the depth
    rw = rc @ R  # (R^T applied to each ray)
    with np.errstate(all="ignore"):
        t0, t1 = (lo - eye) / rw, (hi - eye) / rw
    tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    return np.where((tn <= tf) & (tn > 0), tn, 0.0)


def cube_views(count, seed):
    """`count` seeded cameras on a shell of radius 2 to 3.5 about the unit cube, each looking at a point near its centre."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(look_at(d * rng.uniform(2.0, 3.5), rng.uniform(-0.15, 0.15, size=3)))
    return np.stack(out)


def mixed_scene():
    """The GPU test's mesh and views: a welded 20 x 16 grid tilted against the first camera, four image-sized triangles behind and across
    it, degenerate faces (a repeated index, three collinear vertices), faces with a bad index, and faces that cross the near plane of
    the cameras; three cameras at 37 x 29.  dict(vertices, faces, w2c [3,4,4], K, W, H, near)."""
    W, H, K = 37, 29, (30.0, 31.0, 17.25, 14.5)
    gv, gf = grid_mesh(20, 16, (-0.8, -0.6, 2.0), (0.08, 0.0, 0.012), (0.0, 0.075, 0.02))
    big = np.array([[-3.0, -2.5, 3.0], [3.5, -2.0, 3.2], [0.2, 3.0, 2.9],      # an image-sized triangle behind the grid
                    [-2.0, 2.0, 2.5], [2.5, 2.2, 2.4], [0.0, -2.8, 3.4],       # another, crossing the first
                    [-1.0, -1.0, 1.6], [1.2, -0.9, 1.7], [0.1, 1.1, 4.0],      # a steep one that cuts through the grid
                    [0.0, 0.0, 2.0], [0.5, 0.5, 2.0], [1.0, 1.0, 2.0],         # collinear: A == 0 exactly in the first view
                    [0.3, 0.2, -0.5], [0.4, -0.3, 1.5], [-0.6, 0.1, 2.5]], f32)  # a triangle through the first camera's near plane
    V0 = len(gv)
    verts = np.concatenate([gv, big])
    extra = np.array([[V0, V0 + 1, V0 + 2], [V0 + 3, V0 + 4, V0 + 5], [V0 + 6, V0 + 7, V0 + 8], [V0 + 2, V0 + 1, V0],  # (the first, reversed)
                      [V0 + 9, V0 + 10, V0 + 11], [5, 5, 9], [3, 3, 3], [len(verts), 1, 2], [-1, 2, 3], [1, 2, 1 << 30],
                      [V0 + 12, V0 + 13, V0 + 14], [V0 + 12, 40, 200]], np.int32)
    at = len(gf) // 2
    faces = np.concatenate([gf[:at], extra[:6], gf[at:], extra[6:]])
    w2c = np.stack([look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), look_at((0.9, -0.4, 0.3), (0.0, 0.0, 2.3)), look_at((-0.7, 0.5, 0.6), (0.1, 0.0, 2.2))])
    return dict(vertices=verts, faces=faces, w2c=w2c, K=K, W=W, H=H, near=0.05)
