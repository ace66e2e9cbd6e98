"""Numpy restatement of DQO-MAP's per-frame tracking chain (the checker for dqo_icp's tracker; tests/test_*tracking*.py):

  preprocess     Tracker.map_preprocess's geometry (SLAM/multiprocess/tracker.py:135-156; bilateralFilter_torch, compute_vertex_map,
                 compute_normal_map, compute_confidence_map in SLAM/utils.py:65-142, 607-646)
  pyramid        ImagePyramids("max") + build_vertex_pyramid + build_normal_pyramid (SLAM/icp.py:340-358, SLAM/utils.py:542-558)
  fill           IcpTracker.update_last_status (SLAM/icp.py:403-421)
  predict_pose   IcpTracker.predict_pose (SLAM/icp.py:423-458): coarse-to-fine Gauss-Newton with the normal equations of
                 oracle/map_oracle.icp_normal_equations, solved in double, then the pixel-aligned point-to-plane loss.

Per-pixel work is fp32 in the reference's operation order; sums are fp64.
"""
import math

import numpy as np

from oracle import map_oracle as mo

f32 = np.float32


def fma(a, b, c):
    """fp32 fused multiply-add (the product is exact in fp64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def norm3(v):
    """torch.norm / linalg.vector_norm of 3-vectors on the CPU: sqrt(fma(z, z, fma(y, y, x * x))), keepdim."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.sqrt(fma(z, z, fma(y, y, x * x)))[..., None]


def cross(a, b):
    """torch.cross on the CPU: component i = fma(a_j, b_k, -(a_k * b_j))."""
    c = lambda j, k: fma(a[..., j], b[..., k], -(a[..., k] * b[..., j]))
    return np.stack([c(1, 2), c(2, 0), c(0, 1)], -1)


def bilateral(depth, radius=5, sigma_color=2.0, sigma_space=2.0):
    """bilateralFilter_torch: circular footprint, zero padding, zero taps masked, 0 / 0 -> 0."""
    d = np.asarray(depth, f32)
    H, W = d.shape
    pad = np.pad(d, radius)
    wsum = np.zeros_like(d)
    psum = np.zeros_like(d)
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            if i * i + j * j > radius * radius:
                continue
            nb = pad[radius + i:radius + i + H, radius + j:radius + j + W]
            spatial = f32(-(i * i + j * j) / (2 * sigma_space ** 2))
            diff = d - nb
            color = -(diff * diff) / f32(2 * sigma_color ** 2)
            w = np.exp(spatial + color) * (nb != 0)
            wsum = wsum + w
            psum = psum + w * nb
    with np.errstate(invalid="ignore", divide="ignore"):
        out = psum / wsum
    out[wsum == 0] = 0
    return out.astype(f32)


def vertex_map(depth, fx, fy, cx, cy):
    d = np.asarray(depth, f32)
    H, W = d.shape
    x = ((np.arange(W, dtype=f32) - f32(cx)) / f32(fx))[None, :]
    y = ((np.arange(H, dtype=f32) - f32(cy)) / f32(fy))[:, None]
    return np.stack([x * d, y * d, d * f32(1)], -1).astype(f32)


def normal_map(V):
    """compute_normal_map: Sobel (replicate padding), cross(dy, dx), / (|n| + 1e-8), zero where z <= min z or z >= max z."""
    P = np.pad(np.asarray(V, f32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = V.shape[:2]
    s = lambda a, b: P[1 + a:1 + a + H, 1 + b:1 + b + W]
    # conv2d's tap order (row-major, one tap at a time): bitwise what the reference's feature_gradient computes
    dx = ((((-s(-1, -1) + s(-1, 1)) - f32(2) * s(0, -1)) + f32(2) * s(0, 1)) - s(1, -1)) + s(1, 1)
    dy = ((((-s(-1, -1) - f32(2) * s(-1, 0)) - s(-1, 1)) + s(1, -1)) + f32(2) * s(1, 0)) + s(1, 1)
    n = cross(dy, dx)
    n = n / (norm3(n) + f32(1e-8))
    z = V[..., 2]
    bad = (z <= z.min()) | (z >= z.max())
    n[bad] = 0
    return n.astype(f32)


def cosine_similarity(a, b, eps=1e-8):
    """torch.nn.functional.cosine_similarity along the last axis: each vector over max(|v|, eps), then the dot product."""
    q = (a / np.maximum(norm3(a), f32(eps))) * (b / np.maximum(norm3(b), f32(eps)))
    return (q[..., 0] + q[..., 1]) + q[..., 2]


def confidence_map(normal, fx, fy, cx, cy):
    H, W = normal.shape[:2]
    ray = np.ones((H, W, 3), f32)
    ray[..., 0] = ((np.arange(W, dtype=f32) - f32(cx)) / f32(fx))[None, :]
    ray[..., 1] = ((np.arange(H, dtype=f32) - f32(cy)) / f32(fy))[:, None]
    ray = ray / (norm3(ray) + f32(1e-8))
    return np.abs(cosine_similarity(normal, ray))


def intrinsics(K):
    K = np.asarray(K, f32)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def preprocess(depth, K, min_depth, max_depth, invalid_confidence_thresh, depth_filter=False):
    d = np.asarray(depth, f32).reshape(depth.shape[0], depth.shape[1])
    d = bilateral(d) if depth_filter else d.copy()
    d[~((d > f32(min_depth)) & (d < f32(max_depth)))] = 0
    fx, fy, cx, cy = intrinsics(K)
    V = vertex_map(d, fx, fy, cx, cy)
    N = normal_map(V)
    C = confidence_map(N, fx, fy, cx, cy)
    invalid = (N == 0).all(-1) | (C < f32(invalid_confidence_thresh))
    d[invalid] = 0
    V[invalid] = 0
    N[invalid] = 0
    C[invalid] = 0
    return dict(depth=d, vertex=V, normal=N, conf=C, invalid=invalid)


def maxpool(d, k):
    H, W = d.shape
    h, w = H // k, W // k
    return d[:h * k, :w * k].reshape(h, k, w, k).max(axis=(1, 3))


def pyramid(depth, K, levels=3):
    """[(vertex, normal)] coarsest first: level i pools by 2^(levels-1-i) and scales K by the inverse (K[2,2] = 1)."""
    d = np.asarray(depth, f32).reshape(depth.shape[0], depth.shape[1])
    fx, fy, cx, cy = intrinsics(K)
    out = []
    for i in range(levels):
        k = 1 << (levels - 1 - i)
        s = f32(1.0 / k)
        V = vertex_map(maxpool(d, k), fx * s, fy * s, cx * s, cy * s)
        out.append((V, normal_map(V)))
    return out


def fill(render_depth, frame_depth, render_normal, frame_normal, distance_threshold, normal_threshold):
    r = np.asarray(render_depth, f32).reshape(frame_depth.shape[0], frame_depth.shape[1]).copy()
    fd = np.asarray(frame_depth, f32).reshape(r.shape)
    nmask = (f32(1) - cosine_similarity(np.asarray(render_normal, f32), np.asarray(frame_normal, f32))) > f32(normal_threshold)
    m = ((np.abs(r - fd) > f32(distance_threshold)) | (r == 0) | nmask) & (fd > 0)
    r[m] = fd[m]
    return r


def exp_se3(xi):
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    wh = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    wh2 = wh @ wh
    th = float(np.linalg.norm(w))
    if th <= 1e-8:
        ew, j = np.eye(3), np.eye(3)
    else:
        ew = np.eye(3) + wh * math.sin(th) / th + wh2 * (1.0 - math.cos(th)) / th ** 2
        j = np.eye(3) + (1.0 - math.cos(th)) / th ** 2 * wh + (th - math.sin(th)) / th ** 3 * wh2
    T = np.eye(4)
    T[:3, :3] = ew
    T[:3, 3] = j @ v
    return T


def gauss_newton_step(pose, v0, v1, n0, n1, K, distance_threshold, normal_threshold, damping):
    """One iteration of ICP.icp: normal equations (fp32 results), lev_mar_H in fp32, xi = -H^-1 JtR in double, pose <- exp(xi) pose."""
    JtJ, JtR, valid = mo.icp_normal_equations(v0, v1, n0, n1, pose, K, distance_threshold, normal_threshold)
    JtJ, JtR = JtJ.astype(f32), JtR.astype(f32)
    H = JtJ + np.eye(6, dtype=f32) * (np.trace(JtJ).astype(f32) * f32(damping))
    Hd = H.astype(np.float64)
    inv = np.linalg.pinv(Hd) if np.linalg.det(Hd) == 0 else np.linalg.inv(Hd)
    xi = -inv @ JtR.astype(np.float64)
    return (exp_se3(xi).astype(f32) @ np.asarray(pose, f32)).astype(f32), int(valid.sum())


def p2p_loss(v0, v1, n0, pose):
    """point2plane_loss(v0, v1 @ R^T + t, n0): mean over every pixel of the squared point-to-plane distance (no association)."""
    pose = np.asarray(pose, f32)
    p1 = (v1.reshape(-1, 3) @ pose[:3, :3].T).reshape(v1.shape) + pose[:3, 3]
    r = ((p1 - v0) * n0).sum(-1, dtype=f32)
    return f32((r.astype(np.float64) ** 2).mean())


def predict_pose(pyr_t0, pyr_t1, K, downscales=(0.25, 0.5, 1.0), iters=(5, 5, 5), distance_threshold=0.1, normal_threshold_deg=20,
                 damping=1e-4, fail_threshold=0.02):
    """IcpTracker.predict_pose after the first frame: (pose [4,4] fp32, success, p2p loss, valid ratio of the last level)."""
    nthr = float(np.cos(np.deg2rad(normal_threshold_deg)))
    pose = np.eye(4, dtype=f32)
    cnt, hw = 0, 1
    K = np.asarray(K, f32)
    for level, ds in enumerate(downscales):
        Kl = K * f32(ds)
        Kl[2, 2] = 1
        (vt0, nt0), (vt1, nt1) = pyr_t0[level], pyr_t1[level]
        for _ in range(iters[level]):
            pose, cnt = gauss_newton_step(pose, vt1, vt0, nt1, nt0, Kl, distance_threshold, nthr, damping)
        hw = vt1.shape[:2]
    ratio = f32(f32(cnt) / f32(hw[0])) / f32(hw[1])
    loss = p2p_loss(pyr_t0[-1][0], pyr_t1[-1][0], pyr_t0[-1][1], pose)
    return pose, not (loss > fail_threshold), loss, ratio
