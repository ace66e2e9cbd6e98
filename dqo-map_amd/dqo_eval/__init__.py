"""Keyframe evaluation on MI355X: the metrics the reference reports for a rendered frame — eval_picture, SLAM/eval.py:38-188, called per
frame from slam.py:155,184 and from metric.py — without a host round trip per number.

    eval_picture(render_output, gt_color, gt_depth, min_depth, max_depth)  ->  float32 [8] on the device (ROW)
    eval_picture_dict(row)                                                 ->  the reference's dict (the ONE host read)

One HIP launch (libdqoraster.so: dqo_eval_picture, csrc/map_eval.hip) forms psnr (eval.py:63), the colour L1 (:70) and the depth
statements (:115-126) from double sums added in a fixed order: a row is bitwise reproducible.  The SSIM slot is filled by
dqo_map_ssim_fwd_bwd in value-only mode (two more launches).  Nothing is read back, so a keyframe set is evaluated into a [K, 8] table
(`out=`, `row=`) and read once; the calls can be captured in a graph.

What is NOT here: the reference's "ssim" key is MS-SSIM (pytorch_msssim's `ms_ssim`, eval.py:64) and it also reports LPIPS (`lpips`
AlexNet, :65-68).  Neither library exists on this platform, so neither value can be pinned against its source, and neither is built.
Slot 4 / the "ssim" key here is the SINGLE-SCALE SSIM of utils/loss_utils.py:60-100 (the one the mapping loss uses), and there is no
"lpips" key.  The picture dumps (`save_picture`) and the semantic / instance branches are not part of this either.

GPU only: there is no CPU path.
"""
import torch

import _dqo_native as N

ROW = ("psnr", "color_loss", "depth_loss", "valid_pixel_ratio", "ssim", "mse_r", "mse_g", "mse_b")

_workspaces = {}


def workspace(W, H, device):
    """The two workspaces of one evaluation at W x H as one uint8 tensor: dqo_eval_picture's (zero when first used, handed back ready by
    every call) followed by dqo_map_ssim_fwd_bwd's.  Calls that share one must be ordered on one stream."""
    lib = N.lib()
    n = lib.dqo_eval_picture_workspace_bytes(W, H)
    if n == 0:
        raise RuntimeError(f"dqo_eval: bad image size {W} x {H}")
    return torch.zeros((n + lib.dqo_map_ssim_workspace_bytes(W, H),), dtype=torch.uint8, device=device)


def _image(t, channels, H, W, dtype, name):
    if t.dim() == 2 and channels == 1:
        t = t[None]
    if tuple(t.shape) != (channels, H, W):
        raise RuntimeError(f"dqo_eval.eval_picture: {name} must be [{channels},{H},{W}], got {tuple(t.shape)}")
    return t.to(dtype).contiguous()  # (no copy, no launch, when it already is)


def eval_picture(render_output, gt_color, gt_depth, min_depth, max_depth, out=None, row=0, ssim=True, *, workspace_buffer=None,
                 render_header=None):
    """eval_picture (SLAM/eval.py:38-188) of one frame, on the device.

    render_output: the dict of dqo_harness.mapping.render / Renderer.render, or any dict with `render` [3,H,W], `depth` [1,H,W] and
    `depth_index_map` int32 [1,H,W].  gt_color [3,H,W] (frame.original_image), gt_depth [1,H,W] in metres (the reference's
    255 * frame.original_depth, :115), min_depth / max_depth: the valid range (:116).
    Returns the float32 [8] device row (names: ROW)
        0 psnr   1 color_loss   2 depth_loss   3 valid_pixel_ratio   4 ssim   5..7 mse of r, g, b
    — a new tensor, or out[row] of a caller-owned float32 [K,8] table, whose other rows are not touched.  Nothing is read back and the
    call does not synchronise; eval_picture_dict(row) does the single host read.  Identical images give psnr = +inf, a frame without a
    valid depth pixel depth_loss = NaN: the reference's values.  ssim=False leaves slot 4 alone (NaN in a new row).

    The reference's `ssim` key is MS-SSIM from pytorch_msssim and it also reports LPIPS; neither library exists on this platform, so
    neither is built: slot 4 is the single-scale SSIM of utils/loss_utils.py:60-100 (dqo_map_ssim_fwd_bwd, value only).

    workspace_buffer: a tensor of workspace(W, H, device) the caller keeps (default: one per device and image size, kept by this
    module — calls that share it must be on one stream).  render_header: the geometry buffer of the forward that rendered the frame
    (uint8 tensor); a frame that overflowed its context then gets a row of NaN.  GPU tensors only: a CPU tensor raises RuntimeError."""
    render, depth, index = render_output["render"], render_output["depth"], render_output["depth_index_map"]
    N.require_gpu(render, depth, index, gt_color, gt_depth, out)
    if not render.is_cuda:
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
    lib, dev = N.lib(), render.device
    H, W = int(render.shape[-2]), int(render.shape[-1])
    f32 = torch.float32
    render, gt_color = _image(render, 3, H, W, f32, "render"), _image(gt_color, 3, H, W, f32, "gt_color")
    depth, gt_depth = _image(depth, 1, H, W, f32, "depth"), _image(gt_depth, 1, H, W, f32, "gt_depth")
    index = _image(index, 1, H, W, torch.int32, "depth_index_map")
    if out is None:
        out, row = torch.full((1, 8), float("nan"), dtype=f32, device=dev), 0
    if out.dim() != 2 or out.shape[1] != 8 or out.dtype != f32 or not out.is_contiguous() or not 0 <= int(row) < out.shape[0]:
        raise RuntimeError("dqo_eval.eval_picture: out must be a contiguous float32 [K,8] table and row one of its rows")
    ws = workspace_buffer
    if ws is None:
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), W, H)
        ws = _workspaces.get(key)
        if ws is None:
            ws = _workspaces[key] = workspace(W, H, dev)
    n_eval = lib.dqo_eval_picture_workspace_bytes(W, H)
    with torch.cuda.device(dev):
        stream = N.current_stream()
        if ssim:
            # dqo_map_ssim_fwd_bwd writes TWO floats (the value, weight * (1 - value)): into slots 4 and 5, BEFORE dqo_eval_picture writes
            # mse_r over slot 5 on the same stream — no staging buffer, no copy launch
            N.check(lib.dqo_map_ssim_fwd_bwd(W, H, N.ptr(render), N.ptr(gt_color), 0.0, out.data_ptr() + 4 * (8 * int(row) + 4), None, 0, None,
                                             ws.data_ptr() + n_eval, ws.numel() - n_eval, stream))
        N.check(lib.dqo_eval_picture(W, H, N.ptr(render), N.ptr(gt_color), N.ptr(depth), N.ptr(gt_depth), N.ptr(index), float(min_depth),
                                     float(max_depth), N.ptr(render_header), out.data_ptr(), int(row), ws.data_ptr(), n_eval, stream))
    return out[int(row)]


def eval_picture_dict(row_tensor):
    """The reference's `losses` dict (eval.py:178-185) from a device row — ONE host read.  Keys: valid_pixel_ratio, depth_loss,
    normal_loss (0, as eval.py:167), psnr, ssim (single-scale, see eval_picture), plus color_loss.  No `lpips` key: not built."""
    v = row_tensor.detach().reshape(-1)[:8].cpu().tolist()
    return {"valid_pixel_ratio": v[3], "depth_loss": v[2], "normal_loss": 0, "psnr": v[0], "ssim": v[4], "color_loss": v[1]}
