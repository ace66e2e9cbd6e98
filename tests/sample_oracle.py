"""Test-side oracle of dqo_growth_sample / dqo_mapgrowth.temp_points_init (include/dqo_raster.h, DqoGrowthSample): a numpy restatement of
Mapping.temp_points_init (SLAM/multiprocess/mapper.py:1231-1347), sample_pixels (SLAM/utils.py:145-212) and
GaussianPointCloud.add_empty_points (SLAM/gaussian_pointcloud.py:445-517), one float32 rounding per reference statement, with the CPU
randperm replaced by the key rule below.  tests/test_sample_oracle.py holds it to a literal torch transcription of the reference.

The selection rule (csrc/dqo_sample_hash.h), all arithmetic modulo 2^32:
    fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
    s = fmix32(fmix32(seed_lo ^ 0x9e3779b9) ^ seed_hi);  b = fmix32(s + draw);  key = fmix32(fmix32(pixel ^ b) ^ s) & (2^key_bits - 1)
    chosen = the k smallest (key, pixel) pairs; rows in ascending pixel index.
Orders of the three-term sums, as torch evaluates them on the CPU (held by the test): sum = (0 + 1) + 2, mean = ((0 + 1) + 2) / 3,
norm = sqrt(fma(z, z, fma(y, y, x * x)))."""
import numpy as np

F = np.float32
C0 = 0.28209479177387814
HEADER = ("mask_a", "mask_a_stripped", "mask_b", "mask_b_stripped", "k_a", "k_b", "rows", "overflow")


def fmix32(h):
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def sample_keys(seed, draw, pixels, key_bits=32):
    with np.errstate(over="ignore"):
        seed = int(seed) & (2 ** 64 - 1)
        s = fmix32(fmix32(np.uint32((seed & 0xFFFFFFFF) ^ 0x9E3779B9)) ^ np.uint32(seed >> 32))
        b = fmix32(s + np.uint32(draw))
        key = fmix32(fmix32(np.asarray(pixels, np.uint32) ^ b) ^ s)
    return key & np.uint32(2 ** key_bits - 1)


def choose(seed, draw, pixels, k, key_bits=32):
    """The k smallest (key, pixel) pairs of `pixels`, as ascending pixel indices."""
    pixels = np.asarray(pixels, np.int64)
    order = np.lexsort((pixels, sample_keys(seed, draw, pixels, key_bits)))
    return np.sort(pixels[order[:k]])


def _fma(a, b, c):
    # (a * b is exact in double; the double rounding of the sum before the float one can differ from a true fma once in ~2^29 cases)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def norm3(v):
    return np.sqrt(_fma(v[:, 2], v[:, 2], _fma(v[:, 1], v[:, 1], v[:, 0] * v[:, 0])))


def sum3(v):
    return (v[:, 0] + v[:, 1]) + v[:, 2]


def rotation_arguments(n):
    """compute_rot((0, 0, 1), n) up to the arguments of the three library functions: (unit axis [Q,3], acos argument [Q])."""
    z = np.zeros_like(n)
    z[:, 2] = 1
    axis = np.stack([z[:, 1] * n[:, 2] - z[:, 2] * n[:, 1], z[:, 2] * n[:, 0] - z[:, 0] * n[:, 2], z[:, 0] * n[:, 1] - z[:, 1] * n[:, 0]], 1)
    axis = axis / (norm3(axis) + F(1e-8))[:, None]
    dot = sum3(z * n)
    axis = axis / (norm3(axis) + F(1e-8))[:, None]
    return axis, dot


def rotations(n, double=False):
    """[Q,4] quaternions of compute_rot; acos, sin and cos by torch in float32 — or (double) those three alone in float64 on the same
    float32 arguments, every other statement unchanged."""
    import torch
    axis, dot = rotation_arguments(n)
    if double:
        angle = np.arccos(dot.astype(np.float64)).astype(F)
        half = angle / F(2)
        c, s = np.cos(half.astype(np.float64)).astype(F), np.sin(half.astype(np.float64)).astype(F)
    else:
        half = torch.acos(torch.from_numpy(dot)) / 2
        c, s = torch.cos(half).numpy(), torch.sin(half).numpy()
    return np.concatenate([c[:, None], axis * s[:, None]], 1).astype(F)


def sample_oracle(frame, model=None, *, seed=0, uniform_sample_num, add_transmission_thres=0.5, add_depth_thres=0.1, add_color_thres=0.1,
                  transmission_sample_ratio=1.0, error_sample_ratio=0.05, init_opacity=0.99, xyz_factor=(1.0, 1.0, 0.1), key_bits=32,
                  sh_coeffs=16, capacity=None, select=None):
    """frame: depth_map [H,W,1], vertex_map_w, normal_map_w, color_map [H,W,3], optional instance_img; model (None: first frame):
    render_transmission, render_depth [H,W,1], render_color [H,W,3], render_depth_index.  select(draw, pixels, k) -> the chosen pixels in
    output order (default: the key rule).  Returns dict(header, pixel, xyz, normal, shs, scales, opacity, rotations, obj_id | None)."""
    a = lambda x, c: np.ascontiguousarray(np.asarray(x)).reshape(-1, c)
    depth = a(frame["depth_map"], 1)[:, 0].astype(F)
    vertex, normal, color = (a(frame[k], 3).astype(F) for k in ("vertex_map_w", "normal_map_w", "color_map"))
    inst = None if frame.get("instance_img") is None else a(frame["instance_img"], 3).astype(F)
    HW = depth.shape[0]
    if select is None:
        select = lambda draw, pixels, k: choose(seed, draw, pixels, k, key_bits)
    keep = sum3(normal) != 0  # utils.py:169-170
    if inst is not None:
        keep &= sum3(inst) != 0  # :172-174
    dpos = depth > 0
    draws = []
    if model is None:
        mask_a = dpos
        k_a = int(uniform_sample_num)
        mask_b, k_b, n_b = np.zeros(HW, bool), 0, 0
        draws.append((0, mask_a & keep, k_a))
    else:
        T, rd = a(model["render_transmission"], 1)[:, 0].astype(F), a(model["render_depth"], 1)[:, 0].astype(F)
        rc, di = a(model["render_color"], 3).astype(F), a(model["render_depth_index"], 1)[:, 0]
        mask_a = (T > F(add_transmission_thres)) & dpos
        k_a = int((F(transmission_sample_ratio) * (F(mask_a.sum()) / F(HW))) * F(uniform_sample_num))  # mapper.py:1254-1262
        trans = mask_a & keep if k_a > 0 else mask_a  # the in-place strip of the call at :1269 (none when it returns early, utils.py:155)
        depth_mask = (np.abs(depth - rd) > F(add_depth_thres)) & dpos & (di > -1)
        color_mask = (sum3(np.abs(color - rc)) / F(3) > F(add_color_thres)) & dpos & (T < F(add_transmission_thres))
        mask_b = (color_mask | depth_mask) & ~trans
        k_b = int(F(mask_b.sum()) * F(error_sample_ratio))  # :1327
        draws += [(1, mask_a & keep, k_a), (2, mask_b & keep, k_b)]
    header, pixels = [int(mask_a.sum()), int((mask_a & keep).sum()), int(mask_b.sum()), int((mask_b & keep).sum())], []
    for draw, mask, k in draws:
        k = min(k, int(mask.sum()))  # utils.py:176-177
        header.append(k)
        pixels.append(np.asarray(select(draw, np.nonzero(mask)[0], k), np.int64))
    if model is None:
        header.append(0)
    px = np.concatenate(pixels)
    n = normal[px] / (norm3(normal[px]) + F(1e-8))[:, None]  # gaussian_pointcloud.py:455-456
    stays = sum3(n) != 0  # :457
    px, n = px[stays], n[stays]
    Q = px.shape[0]
    cap = Q if capacity is None else capacity
    header += [min(Q, cap), int(Q > cap)]
    px, n = px[:cap], n[:cap]
    Q = px.shape[0]
    shs = np.zeros((Q, sh_coeffs, 3), F)
    shs[:, 0] = (color[px] - F(0.5)) / F(C0)
    if tuple(float(x) for x in xyz_factor) == (1.0, 1.0, 1.0):
        rot = np.zeros((Q, 4), F)
        rot[:, 0] = 1
    else:
        rot = rotations(n)
    return dict(header=dict(zip(HEADER, header)), pixel=px.astype(np.int32), xyz=vertex[px], normal=n, shs=shs,
                scales=np.full((Q, 3), 1e-6, F), opacity=np.full((Q, 1), init_opacity, F), rotations=rot,
                obj_id=None if inst is None else (inst[px, 0] * F(255)).astype(np.int32))
