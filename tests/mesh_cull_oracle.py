"""dqo_mesh_cull (include/dqo_raster.h, csrc/map_meshcull.hip) restated in numpy: a mesh restricted to what K views see.  Float32
arrays, one numpy operation per statement of the header, so every rounding is the kernel's; the compaction is dqo_mesh_components'.
Also the scene the cull's tests share: the mesh tests/tsdf_oracle.py extracts from the volume test_gpu_tsdf.scene() integrates, with the
three frames that made it."""
import functools

import numpy as np

f32 = np.float32
HEADER = ("vertices", "faces", "vertices_seen", "views_used", "faces_bad_index", "faces_removed", "vertices_removed", "zero")
# a (vertex, view) pair's way through the statements
NOT_IN_FRONT, OUTSIDE_IMAGE, NO_DEPTH, OCCLUDED, SEEN, VIEW_UNUSED = 0, 1, 2, 3, 4, 5


def intrinsics(K):
    K = np.asarray(K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.tolist())


def classify(vertices, w2c, K, W, H, depth=None, view_keep=None, eps=0.03, near=0.0, depth_trunc=np.inf):
    """int8 [V,n]: where the statements leave vertex v in view k (the constants above)."""
    p = np.asarray(vertices, f32).reshape(-1, 3)
    m = np.asarray(w2c, f32).reshape(-1, 4, 4)
    n = len(m)
    fx, fy, cx, cy = (f32(v) for v in intrinsics(K))
    eps, near, depth_trunc = f32(eps), f32(near), f32(depth_trunc)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    state = np.empty((len(p), n), np.int8)
    small = f32(0.0001)
    for k in range(n):
        if view_keep is not None and not view_keep[k]:
            state[:, k] = VIEW_UNUSED
            continue
        with np.errstate(all="ignore"):
            pc = [((m[k, r, 0] * x + m[k, r, 1] * y) + m[k, r, 2] * z) + m[k, r, 3] for r in range(3)]
            front = pc[2] > near
            uf = ((pc[0] * fx) / pc[2] + cx) + f32(0.5)
            vf = ((pc[1] * fy) / pc[2] + cy) + f32(0.5)
            inside = front & (uf >= small) & (uf < f32(W) - small) & (vf >= small) & (vf < f32(H) - small)
            s = np.where(front, np.where(inside, SEEN, OUTSIDE_IMAGE), NOT_IN_FRONT).astype(np.int8)
            if depth is not None:
                u = np.where(inside, uf, 0).astype(np.int32)
                v = np.where(inside, vf, 0).astype(np.int32)
                d = np.asarray(depth[k], f32)[v, u]
                has = (d > 0) & (d <= depth_trunc)
                near_enough = pc[2] <= d + eps
                s = np.where(inside, np.where(has, np.where(near_enough, SEEN, OCCLUDED), NO_DEPTH), s).astype(np.int8)
            assert pc[2].dtype == f32 and uf.dtype == f32
        state[:, k] = s
    return state


def valid_faces(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def cull(vertices, colors, faces, w2c, K, W, H, depth=None, view_keep=None, eps=0.03, near=0.0, depth_trunc=np.inf, min_corners=3):
    """dict(vertices, colors (None without), faces, header int32 [8], vertex_views int32 [V], state int8 [V,n], corners int32 [F]: a
    valid face's seen corners, -1 for a bad face)."""
    p = np.asarray(vertices, f32).reshape(-1, 3)
    V = len(p)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    state = classify(p, w2c, K, W, H, depth, view_keep, eps, near, depth_trunc)
    views = (state == SEEN).sum(1).astype(np.int32)
    ok = valid_faces(V, f)
    corners = np.full(len(f), -1, np.int32)
    corners[ok] = (views[f[ok].astype(np.int64)] > 0).sum(1)  # (a repeated index counts once per corner)
    keep = ok & (corners >= int(min_corners))
    used = np.zeros(V, bool)
    used[f[keep].astype(np.int64).ravel()] = True
    remap = np.cumsum(used) - used
    out_f = remap[f[keep].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    n_used = len(np.asarray(w2c).reshape(-1, 16)) if view_keep is None else int(np.count_nonzero(np.asarray(view_keep)))
    header = np.array([used.sum(), keep.sum(), (views > 0).sum(), n_used, (~ok).sum(), (ok & ~keep).sum(), V - used.sum(), 0], np.int32)
    return dict(vertices=p[used], colors=None if colors is None else np.asarray(colors, f32).reshape(-1, 3)[used], faces=out_f, header=header,
                vertex_views=views, state=state, corners=corners)


# ---- the scene ----------------------------------------------------------------------------------------------------------------------------
EPS = f32(0.02)
FOURTH_POSE = (0.0, 0.0, (0.6, 0.0, 1.45))  # looks along +z from beside the sphere: the part of the mesh with z < 1.45 lies behind it


@functools.lru_cache(maxsize=1)
def scene():
    """dict(vertices, colors, faces: the mesh tsdf_oracle.extract gives for the third state of test_gpu_tsdf.scene() — 6 498 vertices,
    12 368 faces —, w2c float32 [4,4,4], depth float32 [4,H,W], K, W, H): views 0-2 are the frames that made the mesh, view 3 is a
    fourth camera that has part of the mesh behind it."""
    import test_gpu_tsdf as T
    import tsdf_oracle as O
    frames, states = T.scene()
    s = states[2]
    mesh = O.extract(s["tsdf"], s["weight"], s["color"], T.ORIGIN, T.L)
    fourth = T._frame(*FOURTH_POSE, 3)
    depth = np.stack([fr[0] for fr in frames] + [fourth[0]]).astype(f32)
    w2c = np.stack([fr[2] for fr in frames] + [fourth[2]]).astype(f32)
    return dict(vertices=mesh["vertices"], colors=mesh["colors"], faces=mesh["faces"], w2c=w2c, depth=depth, K=(T.FX, T.FY, T.CX, T.CY), W=T.W,
                H=T.H)


def with_extras(vertices, colors, faces):
    """The mesh with faces that repeat an index and faces with a bad index put among its faces (the same vertices)."""
    V = len(vertices)
    f = np.asarray(faces, np.int32)
    extra = np.array([[0, 0, 5], [3, 3, 3], [V, 1, 2], [-1, 2, 3], [1, 2, 1 << 30], [7, V - 1, 7]], np.int32)
    at = len(f) // 2
    return vertices, colors, np.concatenate([f[:at], extra[:3], f[at:], extra[3:]])
