"""dqo_mesh_render_depth_clip (csrc/map_meshrender.hip) and dqo_mesh_cull_faces (csrc/map_meshcull.hip) restated in numpy, statement by
statement of include/dqo_raster.h.  The render: a pair with all three corners in front goes through mesh_render_oracle's statements; a
pair that CROSSES the near plane takes the homogeneous rule — its coverage is evaluated here over the WHOLE image, never over the box, so
a box that the kernel makes too small shows as missing pixels; the box rule is restated only to count the pair (header words 2 and 5).
Also the wall the clipping tests share and its analytic hit set."""
import numpy as np

from mesh_render_oracle import NO_HIT, SMALL_MAX, _max3, _min3, f32, f64, intrinsics, look_at

HEADER = ("views_used", "faces_bad_index", "pairs_rasterised", "pairs_near_clipped", "pairs_degenerate", "pairs_cooperative", "pixels_hit",
          "zero")
CULL_HEADER = ("vertices", "faces", "faces_with_pixels", "views_used", "faces_bad_index", "faces_removed", "vertices_removed", "pixels_counted")


def cross_box(xd, yd, Pd, fm, near, fx, fy, cx, cy, W, H):
    """(x0, x1, y0, y1) as ints, or None: the box of a crossing pair, in double (mr_cross_box's statements)."""
    near, fx, fy, cx, cy = (f64(a) for a in (near, fx, fy, cx, cy))
    xmin = ymin = f64(np.inf)
    xmax = ymax = f64(-np.inf)

    def take(u, v):
        nonlocal xmin, xmax, ymin, ymax
        if u < xmin: xmin = u
        if u > xmax: xmax = u
        if v < ymin: ymin = v
        if v > ymax: ymax = v

    with np.errstate(all="ignore"):
        for i in range(3):
            if fm[i]:
                take(xd[i], yd[i])
        for i in range(3):
            j = (i + 1) % 3
            if fm[i] == fm[j]:
                continue
            a, b = (i, j) if fm[i] else (j, i)
            t = (near - Pd[a, 2]) / (Pd[b, 2] - Pd[a, 2])
            qx = Pd[a, 0] + t * (Pd[b, 0] - Pd[a, 0])
            qy = Pd[a, 1] + t * (Pd[b, 1] - Pd[a, 1])
            take((qx * fx) / near + cx, (qy * fy) / near + cy)
        x0, x1, y0, y1 = np.ceil(xmin) - 1.0, np.floor(xmax) + 1.0, np.ceil(ymin) - 1.0, np.floor(ymax) + 1.0
    x0, y0 = (0.0 if x0 < 0.0 else x0), (0.0 if y0 < 0.0 else y0)  # (a NaN fails every comparison and stays)
    x1, y1 = (float(W - 1) if x1 > W - 1 else x1), (float(H - 1) if y1 > H - 1 else y1)
    if not (x0 <= x1 and y0 <= y1):
        return None
    return int(x0), int(x1), int(y0), int(y1)


def render(vertices, faces, w2c, K, W, H, view_keep=None, near=0.0, depth_trunc=np.inf):
    """dict(depth float32 [n,H,W], face_index int32 [n,H,W], header int32 [8], keys uint64 [n,H,W], crossing bool [n,F]: the valid
    (face, view) pairs with 1 or 2 corners in front)."""
    p = np.asarray(vertices, f32).reshape(-1, 3)
    V = len(p)
    fc = np.asarray(faces, np.int32).reshape(-1, 3)
    m = np.asarray(w2c, f32).reshape(-1, 4, 4)
    n = len(m)
    fx, fy, cx, cy = (f32(a) for a in intrinsics(K))
    near, depth_trunc = f32(near), f32(depth_trunc)
    keys = np.full((n, H, W), NO_HIT, np.uint64)
    crossing = np.zeros((n, len(fc)), bool)
    ok = ((fc >= 0) & (fc < V)).all(1)
    ids = np.nonzero(ok)[0]
    v = fc[ids].astype(np.int64)
    repeated = (v[:, 0] == v[:, 1]) | (v[:, 1] == v[:, 2]) | (v[:, 0] == v[:, 2])
    n_rast = n_near = n_degen = n_coop = 0
    used = [k for k in range(n) if view_keep is None or view_keep[k]]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    Yall, Xall = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    for k in used:
        with np.errstate(all="ignore"):
            pc = np.stack([((m[k, r, 0] * x + m[k, r, 1] * y) + m[k, r, 2] * z) + m[k, r, 3] for r in range(3)], 1)
            assert pc.dtype == f32
            P = pc[v]
            infront = P[:, :, 2] > near
            front = infront.sum(1)
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
        cross = (front > 0) & (front < 3)
        n_near += int(cross.sum())
        crossing[k, ids[cross]] = True
        for g in np.nonzero(boxed | cross)[0]:
            with np.errstate(all="ignore"):
                xd, yd, Pd = px[g].astype(f64), py[g].astype(f64), P[g].astype(f64)
                fm = infront[g]
                if cross[g]:
                    box = cross_box(xd, yd, Pd, fm, near, fx, fy, cx, cy, W, H)
                    Y, X = Yall, Xall  # (the whole image: the box only counts)
                    iy0, iy1, ix0, ix1 = 0, H - 1, 0, W - 1
                else:
                    box = ix0, ix1, iy0, iy1 = int(x0[g]), int(x1[g]), int(y0[g]), int(y1[g])
                    Y, X = np.meshgrid(np.arange(iy0, iy1 + 1, dtype=f64), np.arange(ix0, ix1 + 1, dtype=f64), indexing="ij")
                rx, ry = (X - f64(cx)) / f64(fx), (Y - f64(cy)) / f64(fy)

                def edge(i, j, X, Y, rx, ry):
                    first = v[g, i] < v[g, j]
                    a, b = (i, j) if first else (j, i)
                    if fm[i] and fm[j]:
                        E = (xd[b] - xd[a]) * (Y - yd[a]) - (yd[b] - yd[a]) * (X - xd[a])
                    else:
                        c0 = Pd[a, 1] * Pd[b, 2] - Pd[a, 2] * Pd[b, 1]
                        c1 = Pd[a, 2] * Pd[b, 0] - Pd[a, 0] * Pd[b, 2]
                        c2 = Pd[a, 0] * Pd[b, 1] - Pd[a, 1] * Pd[b, 0]
                        E = (c0 * rx + c1 * ry) + c2
                    return E if first else np.negative(E)

                if cross[g]:
                    t0 = Pd[1, 1] * Pd[2, 2] - Pd[1, 2] * Pd[2, 1]
                    t1 = Pd[1, 2] * Pd[2, 0] - Pd[1, 0] * Pd[2, 2]
                    t2 = Pd[1, 0] * Pd[2, 1] - Pd[1, 1] * Pd[2, 0]
                    A = (Pd[0, 0] * t0 + Pd[0, 1] * t1) + Pd[0, 2] * t2
                    boxless = box is None
                else:
                    A = edge(0, 1, xd[2], yd[2], None, None)
                    boxless = False
                degenerate = bool(repeated[g] or A == 0.0)
                if not boxless:
                    if degenerate:
                        n_degen += 1
                    else:
                        n_rast += 1
                        bw, bh = box[1] - box[0] + 1, box[3] - box[2] + 1
                        if bw > SMALL_MAX or bh > SMALL_MAX or bw * bh > SMALL_MAX:
                            n_coop += 1
                if degenerate:
                    continue
                e0, e1, e2 = edge(0, 1, X, Y, rx, ry), edge(1, 2, X, Y, rx, ry), edge(2, 0, X, Y, rx, ry)
                covered = ((A > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((A < 0) & (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                a, b = Pd[1] - Pd[0], Pd[2] - Pd[0]
                nx, ny, nz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
                np0 = (nx * Pd[0, 0] + ny * Pd[0, 1]) + nz * Pd[0, 2]
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
    return dict(depth=depth, face_index=face_index, header=header, keys=keys, crossing=crossing)


def cull_faces(vertices, colors, faces, face_index, rdepth, depth=None, view_keep=None, eps=0.03, depth_trunc=np.inf, min_pixels=1):
    """dqo_mesh_cull_faces: dict(vertices, colors (None without), faces, header int32 [8], face_pixels int32 [F])."""
    p = np.asarray(vertices, f32).reshape(-1, 3)
    V = len(p)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    F = len(f)
    fi = np.asarray(face_index, np.int32)
    n = len(fi)
    rd = np.asarray(rdepth, f32)
    eps, depth_trunc = f32(eps), f32(depth_trunc)
    ok = ((f >= 0) & (f < V)).all(1)
    used = np.array([view_keep is None or bool(view_keep[k]) for k in range(n)])
    counts = (fi >= 0) & (fi < F) & used[:, None, None]
    if F:
        counts &= ok[np.clip(fi, 0, F - 1)]
    if depth is not None:
        s = np.asarray(depth, f32)
        with np.errstate(all="ignore"):
            counts &= (s > 0) & (s <= depth_trunc) & (rd <= s + eps)
    pixels = np.bincount(fi[counts].astype(np.int64), minlength=F).astype(np.int64)
    keep = ok & (pixels >= int(min_pixels))
    named = np.zeros(V, bool)
    named[f[keep].astype(np.int64).ravel()] = True
    remap = np.cumsum(named) - named
    out_f = remap[f[keep].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    header = np.array([named.sum(), keep.sum(), (pixels > 0).sum(), used.sum(), (~ok).sum(), (ok & ~keep).sum(), V - named.sum(),
                       int(pixels.sum()) & 0xFFFFFFFF], np.int64).astype(np.uint32).view(np.int32)
    return dict(vertices=p[named], colors=None if colors is None else np.asarray(colors, f32).reshape(-1, 3)[named], faces=out_f, header=header,
                face_pixels=pixels.astype(np.int32))


# ---- the wall ----------------------------------------------------------------------------------------------------------------------------
WALL_VERTICES = np.array([[-50.0, -40.0, 1.0], [60.0, -45.0, 1.0], [55.0, 50.0, 1.0], [-45.0, 48.0, 1.0]], f32)
WALL_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
WALL_K, WALL_W, WALL_H = (30.0, 31.0, 17.25, 14.5), 37, 29


def wall_views():
    """float32 [3,4,4]: cameras that stand in front of the wall (z = 1) and look along it, so both of its triangles cross their near
    planes; the third looks across the diagonal the two triangles share."""
    return np.stack([look_at((0.2, -0.1, 0.4), (3.0, 1.0, 1.0)), look_at((1.0, 1.0, 0.9), (5.0, -3.0, 1.0)),
                     look_at((0.0, 2.0, 0.4), (3.0, 7.0, 1.0))])


def ray_quad_depth(w2c, K, W, H, quad=WALL_VERTICES, near=0.0):
    """float64 [H,W]: the camera-space z at which each pixel centre's ray meets the convex planar quad (corners in order), 0 = miss or
    not beyond near; in double from the float32 matrix."""
    fx, fy, cx, cy = intrinsics(K)
    m = np.asarray(w2c, f64).reshape(4, 4)
    q = np.asarray(quad, f64) @ m[:3, :3].T + m[:3, 3]  # the corners in camera space
    nrm = np.cross(q[1] - q[0], q[2] - q[0])
    Y, X = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    r = np.stack([(X - cx) / fx, (Y - cy) / fy, np.ones_like(X)], -1)
    with np.errstate(all="ignore"):
        t = (nrm @ q[0]) / (r @ nrm)  # r has z = 1: the parameter IS the depth
    hitp = r * t[..., None]
    inside = np.ones_like(t, bool)
    for i in range(4):
        a, b = q[i], q[(i + 1) % 4]
        inside &= np.cross(b - a, hitp - a) @ nrm >= 0
    return np.where(inside & (t > near) & np.isfinite(t), t, 0.0)


def ray_box_exit_depth(w2c, K, W, H, lo, hi):
    """float64 [H,W]: the camera-space z at which each pixel centre's ray LEAVES the box [lo, hi] (slab method) for a camera inside it."""
    fx, fy, cx, cy = intrinsics(K)
    m = np.asarray(w2c, f64).reshape(4, 4)
    R, t = m[:3, :3], m[:3, 3]
    eye = -R.T @ t
    Y, X = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    rw = np.stack([(X - cx) / fx, (Y - cy) / fy, np.ones_like(X)], -1) @ R
    with np.errstate(all="ignore"):
        t0, t1 = (lo - eye) / rw, (hi - eye) / rw
    return np.maximum(t0, t1).min(-1)
