"""Tile-mask producers of DQO-MAP's mapping loop on MI355X.

Same names, argument meaning and return types as the reference helpers
    SLAM/utils.py:720-799            meanpool, pixelmask2tilemask, transmission2tilemask, colorerror2tilemask
    SLAM/multiprocess/mapper.py:930-988   Mapping.evaluate_render_range  (here a free function over the render outputs)
but one fused HIP kernel per mask (libdqoraster.so: dqo_tile_count_mask / dqo_transmission_mask / dqo_tile_color_error)
instead of pad + pool + compare chains of eager torch kernels.  window_masks is evaluate_render_range as ONE library call that writes
the caller's buffers and reads nothing back (dqo_window_masks: the top-k selection included, with a defined tie rule).  The rasteriser's tiles are 16x16, and so is the only
stride the reference ever passes; other strides raise.  GPU only: there is no CPU path.
"""
import torch

import _dqo_native as N

_STRIDE = 16


def _check_stride(stride):
    if stride != _STRIDE:
        raise ValueError(f"stride {stride}: the tile-mask kernels are built for the rasteriser's 16x16 tiles")


def _grid(h, w):
    return (h + _STRIDE - 1) // _STRIDE, (w + _STRIDE - 1) // _STRIDE


def _tile_count(pixelmask):
    N.require_gpu_op(pixelmask)
    h, w = pixelmask.shape[:2]
    m = pixelmask if pixelmask.dtype == torch.uint8 else (pixelmask != 0).to(torch.uint8)
    m = m.contiguous()
    gy, gx = _grid(h, w)
    cnt = torch.empty((gy, gx), dtype=torch.int32, device=pixelmask.device)
    with torch.cuda.device(pixelmask.device):
        N.check(N.lib().dqo_tile_count_mask(w, h, N.ptr(m), N.ptr(cnt), N.current_stream()))
    return cnt


def pixelmask2tilemask(pixelmask, stride):
    """SLAM/utils.py:731-743: 1 where any pixel of the tile is set (max-pool of the zero-padded mask); int32 [gy, gx]."""
    _check_stride(stride)
    return (_tile_count(pixelmask) > 0).int()


def transmission2tilemask(pixelmask, stride, tile_mask_ratio=0.5):
    """SLAM/utils.py:752-763: 1 where more than tile_mask_ratio of the tile's 256 pixels are set; int32 [gy, gx]."""
    _check_stride(stride)
    return (_tile_count(pixelmask).float() / float(stride * stride) > tile_mask_ratio).int()


def meanpool(matrix, stride, padding_value=0):
    """SLAM/utils.py:720-729 for a [H, W] image: mean over stride x stride tiles of the padded image."""
    _check_stride(stride)
    h, w = matrix.shape[:2]
    gy, gx = _grid(h, w)
    pad = torch.full((gy * stride, gx * stride), float(padding_value), dtype=torch.float32, device=matrix.device)
    pad[:h, :w] = matrix
    return pad.view(gy, stride, gx, stride).sum((1, 3)) / float(stride * stride)


def color_error_tiles(render, gt):
    """color_error [H, W] = sum_c |render - gt| with the pixels whose rendered colour sums to 0 zeroed
    (mapper.py:949-956), and its 16x16 mean-pool [gy, gx] (meanpool of SLAM/utils.py:720-729), in one pass."""
    N.require_gpu_op(render, gt)
    _, h, w = render.shape
    render, gt = render.float().contiguous(), gt.float().contiguous()
    gy, gx = _grid(h, w)
    err = torch.empty((h, w), dtype=torch.float32, device=render.device)
    tsum = torch.empty((gy, gx), dtype=torch.float32, device=render.device)
    with torch.cuda.device(render.device):
        N.check(N.lib().dqo_tile_color_error(w, h, N.ptr(render), N.ptr(gt), N.ptr(err), N.ptr(tsum), N.current_stream()))
    return err, tsum / float(_STRIDE * _STRIDE)


def colorerror2tilemask(color_error, stride, top_ratio=0.4, _pooled=None):
    """SLAM/utils.py:766-799: the top_ratio share of tiles with the largest mean colour error; int32 [gy, gx].
    (`_pooled`: the mean-pooled error from color_error_tiles(), to skip the pooling pass.)"""
    _check_stride(stride)
    if _pooled is None:
        h, w = color_error.shape[:2]
        gy, gx = _grid(h, w)
        pad = torch.zeros((gy * stride, gx * stride), dtype=torch.float32, device=color_error.device)
        pad[:h, :w] = color_error
        _pooled = pad.view(gy, stride, gx, stride).sum((1, 3)) / float(stride * stride)
    sample_num = int(torch.numel(_pooled) * top_ratio)
    _, idx = torch.topk(_pooled.reshape(-1), k=sample_num)
    tile_mask = torch.zeros_like(_pooled, dtype=torch.int32)
    tile_mask.view(-1)[idx] = 1
    return tile_mask


def evaluate_render_range(T_map, render=None, gt=None, global_opt=False, sample_ratio=-1):
    """Mapping.evaluate_render_range (mapper.py:930-988) over the rasteriser's outputs: returns
    (render_mask bool [H, W], tile_mask int32 [gy, gx] or None, render_ratio 0-dim tensor)."""
    N.require_gpu_op(T_map)
    t = T_map.reshape(T_map.shape[-2], T_map.shape[-1]).float().contiguous()
    h, w = t.shape
    if global_opt and sample_ratio > 0:
        err, pooled = color_error_tiles(render, gt)
        tile_mask = colorerror2tilemask(err, _STRIDE, sample_ratio, _pooled=pooled)
        render_mask = tile_mask.bool().repeat_interleave(_STRIDE, 0).repeat_interleave(_STRIDE, 1)[:h, :w]
        return render_mask, tile_mask, render_mask.sum() / (h * w)
    gy, gx = _grid(h, w)
    mask = torch.empty((h, w), dtype=torch.uint8, device=t.device)
    cnt = torch.empty((gy, gx), dtype=torch.int32, device=t.device)
    total = torch.empty((1,), dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        N.check(N.lib().dqo_transmission_mask(w, h, N.ptr(t), N.ptr(mask), N.ptr(cnt), N.ptr(total), N.current_stream()))
    render_mask = mask.bool()
    if global_opt:
        return render_mask, None, total[0] / (h * w)
    tile_mask = (cnt.float() / float(_STRIDE * _STRIDE) > 0.5).int()
    return render_mask, tile_mask, total[0] / (h * w)


MODE_LOCAL, MODE_ERROR, MODE_FINAL = 0, 1, 2  # dqo_window_masks: the three branches of mapper.py:945-985
_SUMS_OFFSET = N.CONSTANTS["DQO_WINDOW_MASKS_SUMS_OFFSET"]


def window_masks_workspace(h, w, device):
    """The workspace of window_masks for an h x w frame: zero when first used, then left to the calls that share it (one stream)."""
    n = N.lib().dqo_window_masks_workspace_bytes(w, h)
    if n == 0:
        raise ValueError(f"window_masks: bad image size {h} x {w}")
    return torch.zeros((n,), dtype=torch.uint8, device=device)


def window_masks_tile_sums(workspace, h, w):
    """float32 [gy, gx] view of the colour error sums the last error-mode call on `workspace` selected from."""
    gy, gx = _grid(h, w)
    return workspace[_SUMS_OFFSET:_SUMS_OFFSET + 4 * gy * gx].view(torch.float32).view(gy, gx)


def _checked_out(t, name, dtype, shape, device):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype:
        raise RuntimeError(f"window_masks: {name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda or t.device != device:
        raise RuntimeError(f"window_masks: {name} must be on {device} (libdqoraster operators need GPU tensors; there is no CPU path)")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"window_masks: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"window_masks: {name} must be contiguous (it is written in place)")
    return t


def _checked_image(t, name, shape, device):
    if t is None:
        raise RuntimeError(f"window_masks: the error mode needs {name}")
    if not t.is_cuda or t.device != device or t.dtype != torch.float32 or t.numel() != shape[0] * shape[1] * shape[2] or not t.is_contiguous():
        raise RuntimeError(f"window_masks: {name} must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")
    return t


def window_masks(T_map, render=None, gt=None, *, global_opt=False, sample_ratio=-1, tile_mask_ratio=0.5, render_mask=None, tile_mask=None,
                 ratio_out=None, render_header=None, workspace=None):
    """Mapping.evaluate_render_range (mapper.py:930-988) as one library call (dqo_window_masks), nothing read back:
        global_opt and sample_ratio > 0   the k = int(gy * gx * sample_ratio) tiles with the largest colour error (render, gt: [3, H, W]);
                                          the render mask is the tile mask over its pixels
        global_opt, sample_ratio <= 0     render_mask = T_map != 1, the tile mask all ones (the reference returns None)
        otherwise                         render_mask = T_map != 1, tile_mask = count / 256 > tile_mask_ratio
    Returns (render_mask uint8 [H, W], tile_mask int32 [gy, gx], ratio float32 [1]): the caller's tensors where given (checked: dtype,
    shape, contiguity, device), written in place.  Ties of the selection go to the lower tile index.  render_header: the geometry buffer
    (or header tensor) of the render the images come from; if its overflow word is set the masks keep their bytes and the ratio is NaN.
    workspace: window_masks_workspace(H, W, device), kept by the caller between calls (None: made for this call)."""
    N.require_gpu_op(T_map)
    h, w = int(T_map.shape[-2]), int(T_map.shape[-1])
    dev = T_map.device
    gy, gx = _grid(h, w)
    if T_map.dtype != torch.float32 or T_map.numel() != h * w or not T_map.is_contiguous():
        raise RuntimeError("window_masks: T_map must be a contiguous float32 [H, W] or [1, H, W] tensor")
    mode, k = MODE_LOCAL, 0
    if global_opt and sample_ratio > 0:
        mode, k = MODE_ERROR, int(gy * gx * sample_ratio)  # SLAM/utils.py:787
        render, gt = _checked_image(render, "render", (3, h, w), dev), _checked_image(gt, "gt", (3, h, w), dev)
    elif global_opt:
        mode = MODE_FINAL
    render_mask = _checked_out(render_mask, "render_mask", torch.uint8, (h, w), dev)
    tile_mask = _checked_out(tile_mask, "tile_mask", torch.int32, (gy, gx), dev)
    ratio_out = _checked_out(ratio_out, "ratio_out", torch.float32, (1,), dev)
    if workspace is None:
        workspace = window_masks_workspace(h, w, dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise RuntimeError(f"window_masks: workspace must be a contiguous uint8 tensor on {dev}")
    if render_header is not None and (not render_header.is_cuda or render_header.device != dev or render_header.numel() * render_header.element_size() < 32):
        raise RuntimeError(f"window_masks: render_header must hold the 32-byte header on {dev}")
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_window_masks(w, h, mode, N.ptr(T_map), N.ptr(render) if mode == MODE_ERROR else None,
                                         N.ptr(gt) if mode == MODE_ERROR else None, float(tile_mask_ratio), k, N.ptr(render_mask),
                                         N.ptr(tile_mask), N.ptr(ratio_out), N.ptr(render_header), N.ptr(workspace), workspace.numel(),
                                         N.current_stream()))
    return render_mask, tile_mask, ratio_out
