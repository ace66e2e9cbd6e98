"""Order-exact numpy restatement of csrc/icp.hip: the per-pixel fp32 statements of the ICP normal equations one rounding at a time, in
the kernel's order (its head comment, SLAM/icp.py:51-123), exact sums, and the device-side Gauss-Newton step (icp.py:248-337).

Every per-pixel operation is an elementwise np.float32 operation (no matmul, no reductions, no cross product), so a correct kernel
agrees with `probe` bit for bit and with `sums` to the rounding of its own fp64 accumulation."""
import math

import numpy as np

f32 = np.float32
IDX = [(a, b) for a in range(6) for b in range(a, 6)]  # the kernel's order of the 21 upper-triangular sums


def intrinsics(K, k_scale=1.0):
    """(fx, fy, cx, cy) as dqo_load_intrinsics forms them: f32(K) * f32(k_scale), one rounding each."""
    K = np.asarray(K, f32).reshape(3, 3)
    s = f32(k_scale)
    return K[0, 0] * s, K[1, 1] * s, K[0, 2] * s, K[1, 2] * s


def trace_pixels(v0, v1, n0, n1, pose, fx, fy, cx, cy, thr_d, thr_n):
    """Every intermediate of the per-pixel pass as [H, W] fp32 / bool arrays (a dict).  Values of pixels that fail `ok0` are
    whatever the arithmetic gives; only `ok`, `J` and `r` are masked."""
    v0, v1, n0, n1 = (np.ascontiguousarray(a, f32) for a in (v0, v1, n0, n1))
    P = np.asarray(pose, f32).reshape(4, 4)
    fx, fy, cx, cy, thr_d, thr_n = (f32(x) for x in (fx, fy, cx, cy, thr_d, thr_n))
    H, W, _ = v0.shape
    x, y, z = v0[..., 0], v0[..., 1], v0[..., 2]
    a, b, c = n0[..., 0], n0[..., 1], n0[..., 2]
    one, two = f32(1), f32(2)
    wm, hm = f32(W - 1), f32(H - 1)
    with np.errstate(all="ignore"):
        p = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
        n = [(P[i, 0] * a + P[i, 1] * b) + P[i, 2] * c for i in range(3)]
        u = (p[0] / p[2]) * fx + cx
        v = (p[1] / p[2]) * fy + cy
        inview = (u > 0) & (u < wm) & (v > 0) & (v < hm)
        ok0 = (z > 0) & inview
        un, vn = u / (wm / two) - one, v / (hm / two) - one
        gx = np.minimum(wm, np.maximum(((un + one) / two) * wm, f32(0)))
        gy = np.minimum(hm, np.maximum(((vn + one) / two) * hm, f32(0)))
        xi = np.where(ok0, np.rint(gx), 0).astype(np.int64)  # np.rint: round half to even
        yi = np.where(ok0, np.rint(gy), 0).astype(np.int64)
        q = [v1[yi, xi, k] for k in range(3)]
        m = [n1[yi, xi, k] for k in range(3)]
        d = [p[k] - q[k] for k in range(3)]
        ndot = (n[0] * m[0] + n[1] * m[1]) + n[2] * m[2]
        dn = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        ok = ok0 & (q[2] > 0) & (ndot > thr_n) & ~(dn > thr_d)
        r = (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]
        J = [-(m[1] * p[2] - m[2] * p[1]), -(-m[0] * p[2] + m[2] * p[0]), -(m[0] * p[1] - m[1] * p[0]), m[0], m[1], m[2]]
    J = np.where(ok[..., None], np.stack(J, -1), f32(0)).astype(f32)
    r = np.where(ok, r, f32(0)).astype(f32)
    return dict(p=p, n=n, u=u, v=v, inview=inview, ok0=ok0, gx=gx, gy=gy, xi=xi, yi=yi, q=q, m=m, d=d, ndot=ndot, dn=dn, ok=ok, J=J, r=r)


def per_pixel(v0, v1, n0, n1, pose, fx, fy, cx, cy, thr_d, thr_n):
    """(ok [H, W] bool, J [H, W, 6] fp32, r [H, W] fp32); J and r are zero where ok is false."""
    t = trace_pixels(v0, v1, n0, n1, pose, fx, fy, cx, cy, thr_d, thr_n)
    return t["ok"], t["J"], t["r"]


def _exact_sum(terms):
    return math.fsum(terms.tolist()) if np.isfinite(terms).all() else float(np.sum(terms))


def sums(ok, J, r):
    """(JtJ [6, 6] fp32, JtR [6] fp32, count, absJ [6, 6] fp64, absR [6] fp64): the exact sums of the fp64 products (which are exact)
    over the valid pixels, rounded once to fp32, and the sums of the terms' magnitudes."""
    Jv, rv = J[ok].astype(np.float64), r[ok].astype(np.float64)
    JtJ, JtR = np.zeros((6, 6), f32), np.zeros(6, f32)
    absJ, absR = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all="ignore"):
        for a, b in IDX:
            t = Jv[:, a] * Jv[:, b]
            JtJ[a, b] = JtJ[b, a] = f32(_exact_sum(t))
            absJ[a, b] = absJ[b, a] = _exact_sum(np.abs(t))
        for a in range(6):
            t = Jv[:, a] * rv
            JtR[a] = f32(_exact_sum(t))
            absR[a] = _exact_sum(np.abs(t))
    return JtJ, JtR, int(ok.sum()), absJ, absR


def probe(ok, J, r, pixel):
    """The kernel's outputs when only `pixel` = (row, column) has depth in frame 0: each sum is 0.0 plus one exact fp64 product,
    rounded to fp32 (so a product of -0.0 comes out as +0.0)."""
    i, j = pixel
    if not ok[i, j]:
        return np.zeros((6, 6), f32), np.zeros(6, f32), 0
    Jd, rd = J[i, j].astype(np.float64), np.float64(r[i, j])
    with np.errstate(all="ignore"):
        return (0.0 + np.outer(Jd, Jd)).astype(f32), (0.0 + Jd * rd).astype(f32), 1


def chol6_failing_pivot(A):
    """The column at which the kernel's Cholesky of the symmetric fp64 A gives up (pivot not positive or not finite); None if it
    runs through."""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
            if not (d > 0.0) or not math.isfinite(d):
                return j
            L[j, j] = math.sqrt(d)
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    return None


def exp_se3(xi):
    """icp.py:272-312 in float64: rotation first, translation through the left Jacobian."""
    w, v = xi[:3], xi[3:]
    wh = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    wh2 = wh @ wh
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    T = np.eye(4)
    if th > 1e-8:
        T[:3, :3] = np.eye(3) + wh * math.sin(th) / th + wh2 * (1.0 - math.cos(th)) / th ** 2
        j = np.eye(3) + (1.0 - math.cos(th)) / th ** 2 * wh + (th - math.sin(th)) / th ** 3 * wh2
    else:
        j = np.eye(3)
    T[:3, 3] = j @ v
    return T, th


def solve_step(JtJ, JtR, pose, damping):
    """icp_gauss_newton_kernel after the sums: (new pose [4, 4] fp32, info).  info: `pivot` (the failing Cholesky column or None),
    `branch` ("cholesky", "pinv" or "nonfinite"), `xi`, `theta`, `H`."""
    JtJ, JtR = np.asarray(JtJ, f32).reshape(6, 6), np.asarray(JtR, f32).reshape(6)
    P = np.asarray(pose, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        tr = f32(0)
        for a in range(6):
            tr = tr + JtJ[a, a]
        eps = tr * f32(damping)
        Hm = JtJ.copy()
        for a in range(6):
            Hm[a, a] = JtJ[a, a] + eps
        H64, r64 = Hm.astype(np.float64), JtR.astype(np.float64)
        pivot = chol6_failing_pivot(H64)
        if not np.isfinite(H64).all():
            branch, xi = "nonfinite", np.zeros(6)
        elif pivot is None:
            branch, xi = "cholesky", -np.linalg.solve(H64, r64)
        else:
            branch, xi = "pinv", -(np.linalg.pinv(H64) @ r64)
        T64, th = exp_se3(xi)
        T = T64.astype(f32)
        out = np.zeros((4, 4), f32)
        for a in range(4):
            for c in range(4):
                out[a, c] = ((T[a, 0] * P[0, c] + T[a, 1] * P[1, c]) + T[a, 2] * P[2, c]) + T[a, 3] * P[3, c]
    return out, dict(pivot=pivot, branch=branch, xi=xi, theta=th, H=Hm)


def gauss_newton_step(pose, v0, v1, n0, n1, K, k_scale, thr_d, thr_n, damping):
    """One dqo_icp_gauss_newton call: (new pose [4, 4] fp32, the valid count at the incoming pose, info of solve_step)."""
    ok, J, r = per_pixel(v0, v1, n0, n1, pose, *intrinsics(K, k_scale), thr_d, thr_n)
    JtJ, JtR, cnt, _, _ = sums(ok, J, r)
    out, info = solve_step(JtJ, JtR, pose, damping)
    return out, cnt, info
