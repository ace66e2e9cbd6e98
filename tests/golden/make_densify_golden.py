"""Writes tests/golden/densify_golden.npz: the densified cloud of 24 surfels in torch's float32 CPU operators, as the reference forms it
(GaussianPointCloud.densify, SLAM/gaussian_pointcloud.py:67-130, with get_normal / get_plane, :780-812, the activations exp and
normalize, and build_rotation, utils/general_utils.py:108-131).  The rule is restated here as include/dqo_raster.h words it, with
float32 operators of the same kind in the same order: the quaternion normalised twice, the level factor a double rounded into the
float32 product, the sigma blocks joined by concat, a stacked and repeated 3 x 3 row matrix, matmul, the repeated means added last.  The
reference module itself needs open3d, plyfile and a CUDA device, so it cannot be imported where this runs.

torch.argmin / argsort leave the order of equal scales unspecified; rows 22 and 23 have two and three equal raw scales and are recorded
with the rule's order (lower index first: stable=True).  Every other row's raw scales differ by at least 1e-3.

The file holds inputs (xyz, scaling_raw, rotation_raw), the cases and per case theta, points [24, M, 3] and normals [24, 3] (every
point of a row has its row's normal, :122).  Run from the repository root:  python tests/golden/make_densify_golden.py"""
import os

import numpy as np
import torch

CASES = ((1, 30, 5), (2, 3, 2), (3, 7, 1))  # (sigma, circle_num, levels)
P = 24
TIE_ROWS = (22, 23)


def rotation_matrices(rotation_raw):
    """[P,3,3] from raw quaternions (r, x, y, z): the activation normalises them, and the matrix builder divides by the norm once more
    (1 up to rounding) before it forms the nine entries of the usual unit-quaternion rotation."""
    q = torch.nn.functional.normalize(rotation_raw)
    w, x, y, z = q.unbind(dim=1)
    length = torch.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = (q / length[:, None]).unbind(dim=1)
    entries = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
               2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
               2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(entries, dim=1).reshape(-1, 3, 3)


def unit_column(R, axis):
    """Column axis[i] of R[i], divided by (its length + 1e-8)."""
    v = R[torch.arange(R.shape[0]), :, axis]
    return v / (torch.linalg.vector_norm(v, dim=-1, keepdim=True) + 1e-8)


def column_table(sigma, circle_num, levels):
    """(block, level, angle) of every column c < M = circle_num * levels * sigma."""
    c = torch.arange(circle_num * levels * sigma)
    ring = circle_num * levels
    return c // ring, (c % ring) // circle_num, c % circle_num


def radii(axis, sigma, circle_num, levels):
    """[P,M]: (axis * sigma) * float32((l + 0.5) / levels) for the first block, plus axis * b in block b >= 1; blocks joined by concat."""
    _, level, _ = column_table(1, circle_num, levels)
    factor = torch.tensor([(l + 0.5) / levels for l in range(levels)], dtype=torch.float64).to(torch.float32)  # a double, rounded once
    first = (axis * float(sigma)) * factor[level][None, :]
    return torch.concat([first] + [first + axis * float(b) for b in range(1, sigma)], dim=1)


def densify(xyz, scaling_raw, rotation_raw, theta, sigma, circle_num, levels):
    R = rotation_matrices(rotation_raw)
    order = torch.argsort(scaling_raw, dim=1, stable=True)  # (exp is monotone; stable: the rule's tie order)
    normal, plane0, plane1 = (unit_column(R, order[:, j]) for j in range(3))
    scales = torch.exp(scaling_raw)
    rows = torch.arange(scales.shape[0])
    axis0, axis1 = scales[rows, order[:, 1]][:, None], scales[rows, order[:, 2]][:, None]
    _, _, angle = column_table(sigma, circle_num, levels)
    M = angle.shape[0]
    x = radii(axis0, sigma, circle_num, levels) * torch.cos(theta)[angle][None, :]
    z = radii(axis1, sigma, circle_num, levels) * torch.sin(theta)[angle][None, :]
    in_plane = torch.stack([x, torch.zeros_like(x), z], dim=-1)  # [P,M,3]: (x, 0, z)
    # the rule's oddity: the three vectors are the ROWS of the matrix that multiplies (x, 0, z); one copy of it per column
    row_matrix = torch.stack([plane0, normal, plane1], dim=1)[:, None].repeat(1, M, 1, 1)
    offsets = torch.matmul(row_matrix, in_plane[..., None])[..., 0]
    return offsets + xyz[:, None, :].repeat(1, M, 1), normal


def inputs():
    g = torch.Generator(device="cpu")
    g.manual_seed(20241120)
    xyz = (torch.rand(P, 3, generator=g) - 0.5) * 6
    # three well separated log scales per row in a random axis order
    base = torch.tensor([-5.5, -3.5, -2.5])[None] + (torch.rand(P, 3, generator=g) - 0.5) * 0.8
    perm = torch.stack([torch.randperm(3, generator=g) for _ in range(P)])
    scaling_raw = torch.gather(base, 1, perm)
    rotation_raw = torch.randn(P, 4, generator=g) * (0.5 + 2 * torch.rand(P, 1, generator=g))  # (not unit: the rule normalises)
    rotation_raw[0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    scaling_raw[22] = torch.tensor([-3.0, -4.0, -3.0])  # two equal, the smallest in the middle
    scaling_raw[23] = torch.tensor([-3.25, -3.25, -3.25])  # three equal
    return xyz.contiguous(), scaling_raw.contiguous(), rotation_raw.contiguous(), g


def main():
    xyz, scaling_raw, rotation_raw, g = inputs()
    out = dict(xyz=xyz.numpy(), scaling_raw=scaling_raw.numpy(), rotation_raw=rotation_raw.numpy(), cases=np.asarray(CASES, np.int32),
               tie_rows=np.asarray(TIE_ROWS, np.int32))
    for j, (sigma, circle_num, levels) in enumerate(CASES):
        theta = (torch.rand(1, circle_num, generator=g) * torch.pi * 2).reshape(-1)
        pts, nrm = densify(xyz, scaling_raw, rotation_raw, theta, sigma, circle_num, levels)
        out[f"theta_{j}"], out[f"points_{j}"], out[f"normals_{j}"] = theta.numpy(), pts.numpy(), nrm.numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "densify_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
