"""Numpy restatement of dqo_window_masks (csrc/map_tilemask.hip) — Mapping.evaluate_render_range (SLAM/multiprocess/mapper.py:930-988)
for one frame — built on oracle/map_oracle.py's tile-mask functions.

    mode 0 (local, :983-985)   render_mask = T_map != 1;  tile_mask = transmission2tilemask(render_mask, 16, tile_mask_ratio)
    mode 1 (error, :947-978)   tile_mask = the k tiles with the largest colour error sum;  render_mask = the tile mask over its pixels
    mode 2 (final, :980-982)   render_mask = T_map != 1;  tile_mask = all ones (the reference's None)
    every mode                 ratio = float32(count of render_mask) / float32(H * W)   (:987)

The selection rule is the kernel's, and it is defined, not inherited from a library: the k largest by (sum descending, tile index
ascending), a sum compared by its float32 bit pattern as an unsigned integer (sums are non-negative; a NaN lies above every number).
Without a NaN that is map_oracle.colorerror2tilemask's order, np.argsort(-pooled, kind="stable")[:k].  The sums are float32 in the
kernel's order of additions (kernel_tile_sums), so that ties are the kernel's ties."""
import numpy as np

from oracle import map_oracle as mo

TILE = 16
MODE_LOCAL, MODE_ERROR, MODE_FINAL = 0, 1, 2


def grid(h, w):
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE


def kernel_tile_sums(err):
    """float32 [gy, gx]: the sum of a float32 [H, W] image over each 16 x 16 tile (zero padding) in the kernel's order: thread
    16 * row + column holds a pixel, each wave of 64 threads adds by the xor butterfly 32, 16, 8, 4, 2, 1, then ((s0 + s1) + s2) + s3."""
    err = np.asarray(err, np.float32)
    h, w = err.shape
    gy, gx = grid(h, w)
    pad = np.zeros((gy * TILE, gx * TILE), np.float32)
    pad[:h, :w] = err
    v = pad.reshape(gy, TILE, gx, TILE).transpose(0, 2, 1, 3).reshape(gy * gx, 4, 64)
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            v = (v + v[:, :, lane ^ off]).astype(np.float32)
        s = v[:, :, 0]
        out = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    return out.astype(np.float32).reshape(gy, gx)


def select_largest(sums, k):
    """int32 mask, shape of `sums`: 1 on the k largest by (bit pattern as uint32 descending, flat index ascending)."""
    keys = np.ascontiguousarray(sums, np.float32).reshape(-1).view(np.uint32).astype(np.int64)
    order = np.argsort(-keys, kind="stable")
    mask = np.zeros(keys.size, np.int32)
    mask[order[:k]] = 1
    return mask.reshape(np.shape(sums))


def expand_tile_mask(tile_mask, h, w):
    """uint8 [h, w]: every pixel gets its tile's word (mapper.py:970-978)."""
    return np.repeat(np.repeat(np.asarray(tile_mask) != 0, TILE, 0), TILE, 1)[:h, :w].astype(np.uint8)


def render_ratio(render_mask):
    return np.float32(np.count_nonzero(render_mask)) / np.float32(render_mask.size)


def top_k(h, w, sample_ratio):
    gy, gx = grid(h, w)
    return int(gy * gx * sample_ratio)  # SLAM/utils.py:787


def window_masks(T_map, render=None, gt=None, mode=MODE_LOCAL, tile_mask_ratio=0.5, k=0):
    """dict(render_mask uint8 [H, W], tile_mask int32 [gy, gx], ratio float32, sums float32 [gy, gx] or None)."""
    sums = None
    if mode == MODE_ERROR:
        _, h, w = np.shape(render)
        with np.errstate(invalid="ignore"):
            sums = kernel_tile_sums(mo.color_error_image(render, gt))
        tile_mask = select_largest(sums, k)
        render_mask = expand_tile_mask(tile_mask, h, w)
    else:
        T = np.asarray(T_map, np.float32)
        T = T.reshape(T.shape[-2], T.shape[-1])
        render_mask = (T != 1).astype(np.uint8)
        tile_mask = mo.transmission2tilemask(render_mask, TILE, tile_mask_ratio) if mode == MODE_LOCAL else np.ones(grid(*T.shape), np.int32)
    return dict(render_mask=render_mask, tile_mask=tile_mask.astype(np.int32), ratio=render_ratio(render_mask), sums=sums)
