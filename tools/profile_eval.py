"""Times keyframe evaluation (FusedMapper.evaluate / dqo_eval.eval_picture, csrc/map_eval.hip) over K = 8 keyframes at 1200 x 680 on the
cfg 3 map against the eager chain it replaces on the same GPU: mapping.render through the drop-in operator (one header read per call),
the torch statements of eval_picture (SLAM/eval.py:60-70, 115-126, with the single-scale ssim of utils/loss_utils.py in place of
MS-SSIM and without LPIPS: neither library exists here) and its five .item() calls per frame.  The two sides alternate, five runs each;
every run is the median of `--reps` passes over the keyframe set between two synchronisations, reported per frame.

    python tools/profile_eval.py [--P 500000] [--K 8] [--reps 10] > profiles/eval_keyframes.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/profile_eval.py --only fused --reps 3      # the kernels' own times
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


def torch_eval_picture(out, gt_image, gt_depth_in, min_depth, max_depth, ssim):
    """SLAM/eval.py:60-70, 115-126, 178-185 with torch on the GPU."""
    image, depth, index = out["render"], out["depth"], out["depth_index_map"]
    mse = ((gt_image - image) ** 2).view(3, -1).mean(1, keepdim=True)
    psnr_value = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    ssim_value = ssim(image, gt_image).mean()
    color_loss = torch.abs(gt_image - image).mean()
    gt_depth = gt_depth_in.clone()
    valid_range_mask = (gt_depth > min_depth) & (gt_depth < max_depth)
    gt_depth[~valid_range_mask] = 0
    depth_error = (gt_depth - depth).abs()
    invalid_depth_mask = (index == -1) | (gt_depth == 0)
    depth_error[invalid_depth_mask] = 0
    valid_depth_mask = ~invalid_depth_mask
    valid_pixel_ratio = valid_depth_mask.sum() / (depth.shape[1] * depth.shape[2])
    depth_loss = torch.abs(depth[valid_depth_mask] - gt_depth[valid_depth_mask]).mean()
    return {"valid_pixel_ratio": valid_pixel_ratio.item(), "depth_loss": depth_loss.item(), "psnr": psnr_value.item(),
            "ssim": ssim_value.item(), "color_loss": color_loss.item()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500000)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["fused", "eager"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_eval: needs a GPU (there is nothing to time without one)")
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    import dqo_eval
    dev = torch.device("cuda")
    cam, scene = scenes.make_config(3, P=a.P)
    # K keyframes around cfg 3's camera: a small yaw / pitch sweep from the same place
    cams = [scenes.replica_camera(cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy, yaw=12.0 + 1.5 * (k - a.K // 2), pitch=4.0 + 0.5 * (k % 3 - 1))
            for k in range(a.K)]
    settings = [mapping.make_settings(c, dev) for c in cams]
    targets = [mapping.perturbed_target(scene, st, dev, 100 + k) for k, st in enumerate(settings)]
    frames = [(st, t["gt_color"], t["gt_depth"]) for st, t in zip(settings, targets)]
    fm = FusedMapper(scene, settings[0], dev)
    lo, hi = 0.3, 5.0
    table = fm.evaluate(frames, min_depth=lo, max_depth=hi)  # (sizes the render context: the one header read)
    if fm.maintain_overflowed():
        table = fm.evaluate(frames, min_depth=lo, max_depth=hi)
    opacity, scales, rotations = fm.activate()
    data = dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs)

    def eager():
        return [torch_eval_picture(mapping.render(st, data), gc, gd, lo, hi, mapping.ssim) for st, gc, gd in frames]

    with torch.no_grad():
        rows, ref = table.cpu().numpy(), eager()
    for k in range(a.K):
        d = dqo_eval.eval_picture_dict(table[k])
        print(f"frame {k}: fused " + "  ".join(f"{n}={d[n]:.6g}" for n in ref[k]) + "   | eager " + "  ".join(f"{n}={v:.6g}" for n, v in ref[k].items()))
    assert np.isfinite(rows).all(), "a frame outgrew the render context"
    sides = {"fused": lambda: fm.evaluate(frames, min_depth=lo, max_depth=hi), "eager": eager}
    if a.only:
        sides = {a.only: sides[a.only]}
    times = {k: [] for k in sides}
    with torch.no_grad():
        for f in sides.values():
            f()
        for run in range(5):  # alternated: every side sees the same drift
            for name, f in sides.items():
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3 / a.K)
                times[name].append(statistics.median(ts))
    print(f"device: {torch.cuda.get_device_name(0)}   P = {a.P}   K = {a.K}   {cam.W} x {cam.H}")
    what = {"fused": "FusedMapper.evaluate", "eager": "mapping.render + torch eval_picture + 5 .item()"}
    for name, ts in times.items():
        print(f"{what[name]:48s} ms per frame, five runs (median of {a.reps} passes each): " + "  ".join(f"{t:.3f}" for t in ts))


if __name__ == "__main__":
    main()
