"""Generates tests/golden/eval_golden.npz by IMPORTING the reference's own helpers (authoring container only):
/root/reference/utils/loss_utils.py (`psnr`, `l1_loss`, `ssim`, `mse`; pure torch, importable as is), run with torch on the CPU, and by
spelling out the depth statements of eval_picture (SLAM/eval.py:115-126) with torch, one statement each.  The fixture holds the base
inputs (64 x 48, values on a 1/1024 grid so the file stays small) and the recorded results `want` [5, 8] float32 of the five cases of
tests/eval_oracle.py:fixture_cases, in eval_oracle.ROW order — never reference source.

SLAM/eval.py itself cannot be imported (CUDA at import time, lpips, pytorch_msssim, open3d); its `ssim` key is MS-SSIM and is not
recorded: slot 4 is utils/loss_utils.py's single-scale ssim(image, gt).

Run:  python tests/golden/make_eval_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import utils.loss_utils as lu  # noqa: E402  (the reference module)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eval_oracle import INPUTS, ROW, fixture_cases  # noqa: E402


def base_inputs():
    rng = np.random.default_rng(20261017)
    H, W = 48, 64
    q = lambda a: (np.round(np.asarray(a) * 1024.0) / 1024.0).astype(np.float32)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    gt_color = q(np.stack([0.5 + 0.4 * np.sin(6 * xx + 2 * yy), 0.5 + 0.4 * np.cos(5 * yy), 0.3 + 0.5 * xx * yy]))
    render = q(np.clip(gt_color + rng.normal(0, 0.05, gt_color.shape), 0, 1))
    gt_depth = 0.1 + 5.6 * (0.5 + 0.5 * np.sin(3 * xx + 4 * yy))  # 0.1 .. 5.7: both ends of (0.3, 5.0) are crossed
    gt_depth[rng.uniform(size=(H, W)) < 0.05] = 0.0               # holes of the sensor
    gt_depth = q(gt_depth)[None]
    depth = q(np.clip(gt_depth + rng.normal(0, 0.03, gt_depth.shape), 0, None))
    depth_index = rng.integers(0, 5000, (1, H, W)).astype(np.int32)
    depth_index[0][rng.uniform(size=(H, W)) < 0.1] = -1
    return dict(render=render, gt_color=gt_color, depth=depth, gt_depth=gt_depth, depth_index=depth_index)


def reference_row(c, min_depth, max_depth):
    image, gt_image, depth, index = (torch.tensor(c[k]) for k in ("render", "gt_color", "depth", "depth_index"))
    psnr_value = lu.psnr(gt_image, image).mean()  # eval.py:63
    ssim_value = lu.ssim(image, gt_image)         # (single-scale: see the docstring)
    color_loss = lu.l1_loss(gt_image, image)      # eval.py:70
    # eval.py:115-126
    gt_depth = torch.tensor(c["gt_depth"]).clone()
    valid_range_mask = (gt_depth > min_depth) & (gt_depth < max_depth)
    gt_depth[~valid_range_mask] = 0
    invalid_depth_mask = (index == -1) | (gt_depth == 0)
    valid_depth_mask = ~invalid_depth_mask
    pixel_num = depth.shape[1] * depth.shape[2]
    valid_pixel_ratio = valid_depth_mask.sum() / pixel_num
    depth_loss = lu.l1_loss(depth[valid_depth_mask], gt_depth[valid_depth_mask])
    mse = lu.mse(gt_image, image).reshape(3)
    return [psnr_value.item(), color_loss.item(), depth_loss.item(), valid_pixel_ratio.item(), ssim_value.item(), *mse.tolist()]


def main():
    base = base_inputs()
    want = np.array([reference_row(c, lo, hi) for _, c, lo, hi in fixture_cases(base)], np.float32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_golden.npz")
    np.savez_compressed(path, want=want, **{k: base[k] for k in INPUTS})
    print("wrote", path, os.path.getsize(path), "bytes")
    for (name, _, _, _), row in zip(fixture_cases(base), want):
        print(f"{name:18s}", dict(zip(ROW, row.tolist())))


if __name__ == "__main__":
    main()
