"""CPU: the oracle of the growth sampler (tests/sample_oracle.py) against torch's own evaluation of the reference's statements, and the
selection rule's distribution.  No GPU, no library: only the test-side oracle."""
import numpy as np
import pytest
import torch

import sample_cases as sc
from sample_oracle import HEADER, choose, rotations, sample_keys, sample_oracle


# ---- the reference's statements, evaluated by torch on the CPU ------------------------------------------------------------------------------
def _sample_pixels(vertex_map, normal_map, color_map, k, select_mask, instance_img, randperm):
    """SLAM/utils.py:145-212 statement by statement (semantics are None on every live path); select_mask is edited IN PLACE."""
    if k == 0:  # :155-156 — before the mask is touched
        return None
    select_mask[torch.where(normal_map.sum(dim=-1) == 0)] = False  # :169-170
    if instance_img is not None:
        select_mask[torch.where(instance_img.sum(dim=-1) == 0)] = False  # :172-174
    if k > select_mask.sum():  # :176-177
        k = int(select_mask.sum())
    flat = select_mask.flatten()
    vertexs, colors, normals = vertex_map.view(-1, 3)[flat], color_map.view(-1, 3)[flat], normal_map.view(-1, 3)[flat]
    samples = randperm(vertexs.shape[0])[:k]  # :185
    pixels = torch.arange(flat.numel())[flat][samples]  # (not a reference statement: which pixels the rows came from)
    inst = None if instance_img is None else instance_img.view(-1, 3)[flat][samples]
    return vertexs[samples], normals[samples], colors[samples], inst, pixels


def _add_empty_points(rows, xyz_factor, init_opacity, sh_coeffs=16):
    """SLAM/gaussian_pointcloud.py:445-517 up to the parameters it hands to cat() (activated scale and opacity)."""
    if rows is None or rows[0].shape[0] < 1:  # :453-454
        return None
    xyz, normal, color, inst, pixels = rows
    normal = normal / (torch.norm(normal, p=2, dim=-1, keepdim=True) + 1e-8)  # :455-456
    valid = normal.sum(dim=-1) != 0  # :457
    xyz, normal, color, pixels = xyz[valid], normal[valid], color[valid], pixels[valid]
    Q = xyz.shape[0]
    shs = torch.zeros((Q, sh_coeffs, 3))
    shs[:, 0] = (color - 0.5) / 0.28209479177387814  # RGB2SH
    if tuple(xyz_factor) == (1, 1, 1):
        rot = torch.zeros((Q, 4))
        rot[:, 0] = 1
    else:  # compute_rot, utils.py:246-251, and quaternion_from_axis_angle, utils/general_utils.py:185-191
        z = torch.tensor([0.0, 0.0, 1.0]).repeat(Q, 1)
        axis = torch.linalg.cross(z, normal)
        axis = axis / (torch.norm(axis, p=2, dim=-1, keepdim=True) + 1e-8)
        angle = torch.acos(torch.sum(z * normal, dim=1)).unsqueeze(-1)
        axis = axis / (torch.norm(axis, p=2, dim=-1, keepdim=True) + 1e-8)
        half = angle / 2
        rot = torch.cat([torch.cos(half), axis * torch.sin(half)], dim=1)
    obj = None if inst is None or inst.numel() <= 1 else (inst[valid][:, 0] * 255).int()  # :495-497
    return dict(pixel=pixels, xyz=xyz, normal=normal, shs=shs, rotations=rot, obj_id=obj,
                scales=torch.ones(Q, 3) * 1e-6, opacity=init_opacity * torch.ones((Q, 1)))


def reference_temp_points_init(frame, model, cfg, randperm):
    """SLAM/multiprocess/mapper.py:1231-1347.  Returns (counts, [rows of each add_empty_points call])."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    fm = {k: t(v) for k, v in frame.items()}
    args = (fm["vertex_map_w"], fm["normal_map_w"], fm["color_map"])
    add = lambda rows: _add_empty_points(rows, cfg["xyz_factor"], cfg["init_opacity"])
    if model is None:
        mask = fm["depth_map"] > 0  # :1235
        n_pre = int(mask.sum())
        rows = _sample_pixels(*args, cfg["uniform_sample_num"], mask, fm["instance_img"], randperm)
        return dict(mask_a=n_pre, mask_a_stripped=int(mask.sum()), mask_b=0, mask_b_stripped=0), [add(rows)]
    # get_render_output hands the renderer's [C,H,W] images over as permuted views (:1677-1686)
    mm = {k: t(np.moveaxis(v, -1, 0)).permute(1, 2, 0) for k, v in model.items()}
    pixel_num = fm["depth_map"].shape[0] * fm["depth_map"].shape[1]
    trans = (mm["render_transmission"] > cfg["add_transmission_thres"]) & (fm["depth_map"] > 0)  # :1251-1253
    n_a = int(trans.sum())
    ratio = trans.sum() / pixel_num  # :1254-1256
    k_trans = int((cfg["transmission_sample_ratio"] * ratio * cfg["uniform_sample_num"]).to(torch.int32))  # :1258-1262
    _sample_pixels(*args, k_trans, trans, fm["instance_img"], randperm)  # :1269, the redundant call
    rows_trans = _sample_pixels(*args, k_trans, trans, fm["instance_img"], randperm)  # :1279
    depth_error = torch.abs(fm["depth_map"] - mm["render_depth"])
    color_error = torch.abs(fm["color_map"] - mm["render_color"]).mean(dim=-1, keepdim=True)
    depth_mask = (depth_error > cfg["add_depth_thres"]) & (fm["depth_map"] > 0) & (mm["render_depth_index"] > -1)
    color_mask = (color_error > cfg["add_color_thres"]) & (fm["depth_map"] > 0) & (mm["render_transmission"] < cfg["add_transmission_thres"])
    sample_mask = (color_mask | depth_mask) & (~trans)  # :1321-1326
    n_b, quirk = int(sample_mask.sum()), bool(sample_mask.flatten()[sc.QUIRK_PIXEL])  # (before the last call strips this mask too)
    k_err = int((sample_mask.sum() * cfg["error_sample_ratio"]).to(torch.int32))  # :1327
    rows_err = _sample_pixels(*args, k_err, sample_mask, fm["instance_img"], randperm)
    counts = dict(mask_a=n_a, mask_a_stripped=int((trans & _strip(fm)).sum()), mask_b=n_b, mask_b_stripped=int((sample_mask & _strip(fm)).sum()),
                  k_unclamped=(k_trans, k_err), quirk=quirk)
    return counts, [add(rows_trans), add(rows_err)]


def _strip(fm):
    keep = fm["normal_map_w"].sum(dim=-1, keepdim=True) != 0
    return keep if fm["instance_img"] is None else keep & (fm["instance_img"].sum(dim=-1, keepdim=True) != 0)


class _Perms:
    """torch.randperm with a fixed generator, every permutation kept in call order."""

    def __init__(self, seed):
        self.g, self.calls = torch.Generator().manual_seed(seed), []

    def __call__(self, n):
        self.calls.append(torch.randperm(n, generator=self.g))
        return self.calls[-1]


CASES = {
    "later_instance_rot": dict(first=False, instance=True, cfg=sc.SMALL),
    "later_plain_identity": dict(first=False, instance=False, cfg=dict(sc.SMALL, xyz_factor=(1, 1, 1))),
    "later_k_trans_zero": dict(first=False, instance=True, cfg=dict(sc.SMALL, transmission_sample_ratio=1e-4)),
    "later_both_k_zero": dict(first=False, instance=True, cfg=dict(sc.SMALL, transmission_sample_ratio=1e-4, error_sample_ratio=1e-4)),
    "later_k_clamped": dict(first=False, instance=True, cfg=dict(sc.SMALL, uniform_sample_num=10 ** 6, error_sample_ratio=1.0)),
    "first_instance": dict(first=True, instance=True, cfg=sc.SMALL),
    "first_plain_clamped": dict(first=True, instance=False, cfg=dict(sc.SMALL, uniform_sample_num=5000)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_torch_on_the_reference_statements(name):
    """(a) With the selection replaced by the reference's own permutations: the counts, both k and every row are EQUAL (rotations included:
    the oracle takes acos / sin / cos from torch)."""
    case = CASES[name]
    frame, model = sc.make_frame(instance=case["instance"])
    model = None if case["first"] else model
    perms = _Perms(5)
    counts, parts = reference_temp_points_init({k: None if v is None else v.copy() for k, v in frame.items()}, model, case["cfg"], perms)
    # the permutations in call order: the first frame's only call; otherwise the calls at :1269 and :1279 (none when k == 0), then :1336
    def select(draw, pixels, k):
        if case["first"]:
            return pixels[perms.calls[0][:k].numpy()]
        k_trans, k_err = counts["k_unclamped"]
        if (k_trans if draw == 1 else k_err) == 0:
            return pixels[:0]
        return pixels[perms.calls[1 if draw == 1 else (2 if k_trans > 0 else 0)][:k].numpy()]

    want = sample_oracle(frame, model, select=select, **case["cfg"])
    for key in ("mask_a", "mask_a_stripped", "mask_b", "mask_b_stripped"):
        assert want["header"][key] == counts[key], key
    got = [p for p in parts if p is not None]
    ks = [want["header"]["k_a"], want["header"]["k_b"]]
    if not case["first"]:
        un = counts["k_unclamped"]
        assert ks == [min(un[0], counts["mask_a_stripped"]), min(un[1], counts["mask_b_stripped"])]
    assert want["header"]["rows"] == sum(p["xyz"].shape[0] for p in got) and want["header"]["overflow"] == 0
    for key in ("pixel", "xyz", "normal", "shs", "scales", "opacity", "rotations", "obj_id"):
        if want[key] is None:
            assert all(p[key] is None for p in got), key
            continue
        ref = torch.cat([p[key] for p in got]).numpy() if got else want[key][:0]
        bits = lambda x: np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x.astype(np.int64)  # (-0.0 is not +0.0)
        assert ref.shape == want[key].shape and np.array_equal(bits(ref), bits(want[key])), (name, key)
    if name == "later_instance_rot":
        assert want["header"]["k_a"] > 0 and want["header"]["k_b"] > 0 and want["header"]["rows"] < sum(ks)  # (a dropped normal was drawn)
        assert want["header"]["mask_a"] > want["header"]["mask_a_stripped"] and want["header"]["mask_b"] > want["header"]["mask_b_stripped"]
    if name == "later_k_trans_zero":
        assert want["header"]["k_a"] == 0 and want["header"]["k_b"] > 0


def test_the_in_place_mask_quirk_is_pinned():
    """A pixel with T above the threshold, depth > 0, a zero normal and a depth error counts in sum(sample_mask): the redundant first
    sample_pixels call strips it from `trans` — unless that call's k is 0, when it returns before touching the mask."""
    frame, model = sc.make_frame()
    on = sample_oracle(frame, model, **sc.SMALL)["header"]
    off = sample_oracle(frame, model, **dict(sc.SMALL, transmission_sample_ratio=1e-4))["header"]
    assert on["k_a"] > 0 and off["k_a"] == 0 and on["mask_b"] > off["mask_b"] and on["mask_b_stripped"] == off["mask_b_stripped"]
    ref_on, _ = reference_temp_points_init({k: None if v is None else v.copy() for k, v in frame.items()}, model, sc.SMALL, _Perms(1))
    assert ref_on["quirk"] is True and ref_on["mask_b"] == on["mask_b"]
    single = {k: (None if v is None else v.copy()) for k, v in frame.items()}
    single["normal_map_w"].reshape(-1, 3)[sc.QUIRK_PIXEL] = (0, 0, 1)  # with a normal the pixel stays in trans
    assert sample_oracle(single, model, **sc.SMALL)["header"]["mask_b"] == on["mask_b"] - 1


def test_the_dropped_normal_is_what_it_claims():
    from sample_oracle import norm3, sum3
    v = np.array([sc.DROPPED_NORMAL], np.float32)
    n = v / (norm3(v) + np.float32(1e-8))[:, None]
    assert sum3(v)[0] != 0 and sum3(n)[0] == 0
    t = torch.from_numpy(v)
    tn = t / (torch.norm(t, p=2, dim=-1, keepdim=True) + 1e-8)
    assert float(t.sum(dim=-1)) != 0 and float(tn.sum(dim=-1)) == 0 and np.array_equal(tn.numpy(), n)


def test_the_key_rule_draws_uniformly():
    """(b) n = 256 selected pixels, k = 64, seeds 0..1999: every pixel's inclusion frequency lies within 0.25 +- 0.05 — 5 sigma of a binomial
    with sigma = sqrt(0.25 * 0.75 / 2000) = 0.0097.  Fixed seeds: deterministic.  All three draws."""
    pixels = np.arange(1000, 1256)
    for draw in (0, 1, 2):
        hits = np.zeros(256)
        for seed in range(2000):
            hits[choose(seed, draw, pixels, 64) - 1000] += 1
        freq = hits / 2000
        assert np.all(np.abs(freq - 0.25) <= 0.05), (draw, freq.min(), freq.max())


def test_the_rule_is_a_pure_function_with_ties_broken_by_pixel():
    """(c) the same arguments give the same rows, another seed another set, and exactly k rows with key_bits = 3 (ties everywhere)."""
    frame, model = sc.make_frame()
    a, b = sample_oracle(frame, model, seed=3, **sc.SMALL), sample_oracle(frame, model, seed=3, **sc.SMALL)
    c = sample_oracle(frame, model, seed=4, **sc.SMALL)
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "header") and a["header"] == b["header"]
    assert {k: v for k, v in a["header"].items() if k != "rows"} == {k: v for k, v in c["header"].items() if k != "rows"}  # (the seed moves no k)
    assert not np.array_equal(a["pixel"], c["pixel"])
    pixels = np.arange(500) * 3
    for k in (0, 1, 7, 250, 500):
        got = choose(9, 1, pixels, k, key_bits=3)
        assert got.shape[0] == k and np.all(np.diff(got) > 0)
        keys = sample_keys(9, 1, pixels, 3)
        assert keys.max() < 8
        if 0 < k < 500:  # the chosen are a prefix of the (key, pixel) order: below the threshold key all, at it the lowest pixels
            t = np.sort(keys)[k - 1]
            at = pixels[keys == t]
            assert set(pixels[keys < t]) <= set(got) and set(got) - set(pixels[keys < t]) == set(at[:k - int((keys < t).sum())])
    assert np.unique(sample_keys(0, 0, np.arange(100000))).shape[0] == 100000  # 32 bits: a bijection of the pixels, no ties
    assert HEADER[6] == "rows"


def test_the_rotation_bar_is_measured():
    """The distance between torch's float32 acos / sin / cos and the same three functions in double on the same float32 arguments, over the
    fixture's rows: 4 x this is the bar tests/test_gpu_sample.py gives the device's library functions (profiles/r08_sample_rotation_bar.txt)."""
    frame, model = sc.make_frame()
    n = sample_oracle(frame, model, **dict(sc.SMALL, uniform_sample_num=10 ** 6, error_sample_ratio=1.0))["normal"]
    d = float(np.abs(rotations(n).astype(np.float64) - rotations(n, double=True)).max())
    print("rotation distance float32 vs double library functions:", d)
    assert 0 < d <= 2.0 ** -22  # (a few ulp of a component of magnitude <= 1; the bar follows the measured value, this only guards it)
