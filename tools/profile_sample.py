"""Times the growth sampler (FusedMapper.sample_new / dqo_mapgrowth.temp_points_init, csrc/map_sample.hip) on one 1200 x 680 frame of the
cfg 3 map against the reference's own statements run with torch on the same GPU (CPU torch.randperm and its copy included, as
SLAM/utils.py:185 has it): render excluded, then render included.  The two sides alternate, five runs each; every run is the median of
`--reps` calls between two synchronisations.

    python tools/profile_sample.py [--P 500000] [--reps 20] > profiles/r08_sample.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/profile_sample.py --only gpu --reps 5      # the kernels' own times
    rocprofv3 --memory-copy-trace -d <dir> -- python tools/profile_sample.py --only gpu --reps 1         # the single device-to-host read
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

import numpy as np
import torch

CFG = dict(uniform_sample_num=50000, add_transmission_thres=0.5, add_depth_thres=0.1, add_color_thres=0.1, transmission_sample_ratio=1.0,
           error_sample_ratio=0.05, init_opacity=0.99, xyz_factor=(1.0, 1.0, 0.1))


def torch_sample_pixels(vertex_map, normal_map, color_map, k, select_mask, instance_img):
    """SLAM/utils.py:145-212 with torch on the GPU, the permutation on the CPU."""
    if k == 0:
        return None
    select_mask[torch.where(normal_map.sum(dim=-1) == 0)] = False
    if instance_img is not None:
        select_mask[torch.where(instance_img.sum(dim=-1) == 0)] = False
    if k > select_mask.sum():
        k = int(select_mask.sum())
    flat = select_mask.flatten()
    vertexs, colors, normals = vertex_map.view(-1, 3)[flat], color_map.view(-1, 3)[flat], normal_map.view(-1, 3)[flat]
    samples = torch.randperm(vertexs.shape[0])[:k]
    inst = None if instance_img is None else instance_img.view(-1, 3)[flat][samples]
    return vertexs[samples], normals[samples], colors[samples], inst


def torch_add_empty_points(rows, M=16):
    if rows is None or rows[0].shape[0] < 1:
        return None
    xyz, normal, color, inst = rows
    normal = normal / (torch.norm(normal, p=2, dim=-1, keepdim=True) + 1e-8)
    valid = normal.sum(dim=-1) != 0
    xyz, normal, color = xyz[valid], normal[valid], color[valid]
    Q = xyz.shape[0]
    shs = torch.zeros((Q, M, 3), device=xyz.device)
    shs[:, 0] = (color - 0.5) / 0.28209479177387814
    z = torch.tensor([0.0, 0.0, 1.0], device=xyz.device).repeat(Q, 1)
    axis = torch.linalg.cross(z, normal)
    axis = axis / (torch.norm(axis, p=2, dim=-1, keepdim=True) + 1e-8)
    angle = torch.acos(torch.sum(z * normal, dim=1)).unsqueeze(-1)
    axis = axis / (torch.norm(axis, p=2, dim=-1, keepdim=True) + 1e-8)
    rot = torch.cat([torch.cos(angle / 2), axis * torch.sin(angle / 2)], dim=1)
    obj = None if inst is None else (inst[valid][:, 0] * 255).int()
    return xyz, normal, shs, rot, obj


def torch_temp_points_init(fm, mm):
    """SLAM/multiprocess/mapper.py:1251-1347 with torch on the GPU."""
    args = (fm["vertex_map_w"], fm["normal_map_w"], fm["color_map"])
    inst = fm.get("instance_img")
    n_pix = fm["depth_map"].shape[0] * fm["depth_map"].shape[1]
    trans = (mm["render_transmission"] > CFG["add_transmission_thres"]) & (fm["depth_map"] > 0)
    k_trans = int((CFG["transmission_sample_ratio"] * (trans.sum() / n_pix) * CFG["uniform_sample_num"]).to(torch.int32))
    torch_sample_pixels(*args, k_trans, trans, inst)
    a = torch_add_empty_points(torch_sample_pixels(*args, k_trans, trans, inst))
    depth_error = torch.abs(fm["depth_map"] - mm["render_depth"])
    color_error = torch.abs(fm["color_map"] - mm["render_color"]).mean(dim=-1, keepdim=True)
    depth_mask = (depth_error > CFG["add_depth_thres"]) & (fm["depth_map"] > 0) & (mm["render_depth_index"] > -1)
    color_mask = (color_error > CFG["add_color_thres"]) & (fm["depth_map"] > 0) & (mm["render_transmission"] < CFG["add_transmission_thres"])
    sample_mask = (color_mask | depth_mask) & (~trans)
    k_err = int((sample_mask.sum() * CFG["error_sample_ratio"]).to(torch.int32))
    b = torch_add_empty_points(torch_sample_pixels(*args, k_err, sample_mask, inst))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["gpu", "torch"], default=None)
    a = ap.parse_args()
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    import dqo_mapgrowth as mg
    dev = torch.device("cuda")
    cam, scene = scenes.make_config(3, P=a.P)
    settings = mapping.make_settings(cam, dev)
    with torch.no_grad():
        tgt = mapping.render(settings, mapping.GaussianParams(scene, dev).activated())
    H, W = tgt["depth"].shape[-2:]
    rng = np.random.default_rng(0)
    depth = tgt["depth"].permute(1, 2, 0).clone()
    depth[:H // 3] += 0.3 * (depth[:H // 3] > 0)
    depth[H // 2:][depth[H // 2:] == 0] = 2.0
    up = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)
    frame = dict(depth_map=depth.contiguous(), color_map=tgt["render"].permute(1, 2, 0).contiguous(), vertex_map_w=up(rng.uniform(-3, 3, (H, W, 3))),
                 normal_map_w=up(rng.normal(size=(H, W, 3))), instance_img=None)
    fm = FusedMapper(scene, settings, dev)
    fm.sample_new(frame, seed=0, tick=0, **CFG)  # (sizes the render context and the sampler's buffers)
    out = fm._maintain_ctx.out
    model = dict(render_color=out[0].permute(1, 2, 0), render_depth=out[1].permute(1, 2, 0), render_depth_index=out[3].permute(1, 2, 0),
                 render_transmission=out[6].permute(1, 2, 0))
    print("header:", fm.sample_header)

    def render_torch():
        o = mapping.render(settings, dict(zip(("opacity", "scales", "rotations"), fm.activate()), xyz=fm.xyz, shs=fm.shs))
        return dict(render_color=o["render"].permute(1, 2, 0), render_depth=o["depth"].permute(1, 2, 0),
                    render_depth_index=o["depth_index_map"].permute(1, 2, 0), render_transmission=o["T_map"].permute(1, 2, 0))

    s = fm._sample_ctx
    sides = {
        "gpu, render excluded": lambda k: mg.temp_points_init(frame, model, seed=k, tick=0, buffers=s["buffers"], workspace=s["workspace"], sh_coeffs=fm.M, **CFG),
        "torch, render excluded": lambda k: torch_temp_points_init(dict(frame), model),
        "gpu, render included": lambda k: fm.sample_new(frame, seed=k, tick=0, **CFG),
        "torch, render included": lambda k: torch_temp_points_init(dict(frame), render_torch()),
    }
    if a.only:
        sides = {k: v for k, v in sides.items() if k.startswith(a.only)}
    times = {k: [] for k in sides}
    with torch.no_grad():
        for f in sides.values():
            f(0)
        for run in range(5):  # alternated: every side sees the same drift
            for name, f in sides.items():
                ts = []
                for k in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f(run * a.reps + k)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                times[name].append(statistics.median(ts))
    for name, ts in times.items():
        print(f"{name:26s} ms per frame, five runs (median of {a.reps} calls each): " + "  ".join(f"{t:.3f}" for t in ts))


if __name__ == "__main__":
    main()
