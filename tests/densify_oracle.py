"""Test-side oracle of dqo_surfel_densify / dqo_eval.densify (include/dqo_raster.h): a float64 numpy restatement of
GaussianPointCloud.densify (SLAM/gaussian_pointcloud.py:67-130, with get_normal :780-791, get_plane :794-812 and build_rotation,
utils/general_utils.py:108-131), and of the subsample that replaces np.random.choice (SLAM/eval.py:244).

Per row i, from the raw parameters (xyz, log scales, quaternion r x y z), M = circle_num * levels * sigma points; column
c = (b * levels + l) * circle_num + k:
    order  = the axes in ascending order of the RAW scales, equal ones lower index first (a stable sort; torch leaves ties unspecified)
    n, p0, p1 = columns order[0], order[1], order[2] of build_rotation(q / |q|), each / (its norm + 1e-8)
    axis0, axis1 = exp(raw[order[1]]), exp(raw[order[2]])
    a  = axis0 * sigma * float32((l + 0.5) / levels) + (axis0 * b if b >= 1),   b_ the same with axis1
    x  = a * cos(theta_k),  z = b_ * sin(theta_k)
    frame "reference": mean + (p0.x x + p0.z z,  n.x x + n.z z,  p1.x x + p1.z z)   (the reference's matmul: p0, n, p1 are matrix ROWS)
    frame "surfel":    mean + x p0 + z p1
    normal = n for every point of the row
The subsample: virtual point v = i * M + c of a kept row gets key = sample_keys(seed, 3, v) (tests/sample_oracle.py: the rule of
csrc/dqo_sample_hash.h; draws 0-2 are the growth sampler's); the n = min(N, cap) smallest keys are chosen, in ascending v."""
import numpy as np

from sample_oracle import fmix32, sample_keys  # noqa: F401  (fmix32: re-exported for the tests)

D = np.float64
DRAW = 3
FRAMES = ("reference", "surfel")


def scale_order(scaling_raw):
    """[P,3] axis indices in ascending order of the raw scales; ties: the lower index first."""
    return np.argsort(np.asarray(scaling_raw), axis=1, kind="stable")


def rotation_matrix(rotation_raw):
    q = np.asarray(rotation_raw, D)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), D)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def surfel_frames(scaling_raw, rotation_raw):
    """(n, p0, p1 [P,3], axis0, axis1 [P]) in float64."""
    raw = np.asarray(scaling_raw)
    order = scale_order(raw)
    R = rotation_matrix(rotation_raw)
    rows = np.arange(raw.shape[0])
    vec = []
    for j in range(3):
        v = R[rows, :, order[:, j]]  # column order[:, j]
        vec.append(v / (np.sqrt((v * v).sum(1)) + 1e-8)[:, None])
    s = np.exp(raw.astype(D))
    return vec[0], vec[1], vec[2], s[rows, order[:, 1]], s[rows, order[:, 2]]


def column_layout(sigma, circle_num, levels):
    """(b, l, k) of every column c < M."""
    c = np.arange(circle_num * levels * sigma)
    ring = circle_num * levels
    return c // ring, (c % ring) // circle_num, c % circle_num


def radii(axis0, axis1, sigma, circle_num, levels):
    """a, b_ [P,M] in float64: the level factor is the float32 the reference multiplies with."""
    b, l, _ = column_layout(sigma, circle_num, levels)
    f = ((l + 0.5) / levels).astype(np.float32).astype(D)
    a = axis0[:, None] * sigma * f[None] + axis0[:, None] * np.where(b >= 1, b, 0)[None]
    b_ = axis1[:, None] * sigma * f[None] + axis1[:, None] * np.where(b >= 1, b, 0)[None]
    return a, b_


def densify_oracle(xyz, scaling_raw, rotation_raw, theta, sigma=1, circle_num=30, levels=5, frame="reference"):
    """dict(points [P,M,3], normals [P,M,3], a_max, b_max [P]) in float64 — every row, no row mask, no subsample."""
    assert frame in FRAMES
    mean = np.asarray(xyz, D)
    n, p0, p1, axis0, axis1 = surfel_frames(scaling_raw, rotation_raw)
    a, b_ = radii(axis0, axis1, sigma, circle_num, levels)
    _, _, k = column_layout(sigma, circle_num, levels)
    th = np.asarray(theta, np.float32).reshape(-1).astype(D)
    assert th.shape[0] == circle_num
    x, z = a * np.cos(th)[k][None], b_ * np.sin(th)[k][None]
    if frame == "reference":
        off = np.stack([p0[:, None, 0] * x + p0[:, None, 2] * z, n[:, None, 0] * x + n[:, None, 2] * z, p1[:, None, 0] * x + p1[:, None, 2] * z], -1)
    else:
        off = x[..., None] * p0[:, None, :] + z[..., None] * p1[:, None, :]
    M = x.shape[1]
    return dict(points=mean[:, None, :] + off, normals=np.repeat(n[:, None, :], M, 1), a_max=np.abs(a).max(1), b_max=np.abs(b_).max(1))


def coordinate_bar(oracle, xyz):
    """[P,1,3]: 2^-23 * (16 * (a_max + b_max) + |mean_c|), the bound on a coordinate's float32 error (tests/test_gpu_densify.py derives it)."""
    return 2.0 ** -23 * (16 * (oracle["a_max"] + oracle["b_max"])[:, None, None] + np.abs(np.asarray(xyz, D))[:, None, :])


NORMAL_BAR = 2.0 ** -23 * 8


def select_oracle(P, M, cap, seed=0, keep=None):
    """(index int64 [n] ascending, header int32-valued list [6]: kept rows, N low, N high, n, M, threshold key as int32) — the virtual
    points dqo_surfel_densify emits for P rows of M columns."""
    rows = np.arange(P) if keep is None else np.nonzero(np.asarray(keep).reshape(-1) != 0)[0]
    v = (rows[:, None].astype(np.int64) * M + np.arange(M)[None]).reshape(-1)
    N = v.shape[0]
    n = min(N, int(cap))
    keys = sample_keys(seed, DRAW, v)
    chosen = np.sort(v[np.argsort(keys, kind="stable")[:n]])
    t = 0xFFFFFFFF if n == N else int(np.sort(keys)[n - 1])
    i32 = lambda w: w - (1 << 32) if w >= (1 << 31) else w  # (the header's words are int32)
    return chosen, [len(rows), i32(N & 0xFFFFFFFF), N >> 32, i32(n), M, i32(t)]
