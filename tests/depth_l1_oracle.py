"""dqo_eval_depth_l1 (include/dqo_raster.h, csrc/map_eval.hip) restated in numpy, additions in the kernels' order: a thread adds its
four pixels (i = (4 j + p) * 256 + tid of block j) in order, a wave its 64 lanes by the xor butterfly 32, 16, .., 1, a block its four waves
in order, a view its blocks in order — all in float64, so the table is the kernel's bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
ROW = ("l1_valid", "l1_image", "rmse_valid", "both", "only_a", "only_b", "neither", "max_abs")
PIX = 4


def _block_sums(vals):
    """vals float64 [blocks, PIX, 256] (zeros where no pixel) -> [blocks]: the kernel's order of additions."""
    t = np.zeros(vals.shape[:1] + (256,))
    for p in range(PIX):
        t = t + vals[:, p]
    t = t.reshape(-1, 4, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        t = t + t[:, :, lanes ^ off]
    w = t[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _view_sum(x):
    """x float64 [HW] -> the view's sum in the kernels' order."""
    HW = len(x)
    blocks = (HW + 256 * PIX - 1) // (256 * PIX)
    pad = np.zeros(blocks * 256 * PIX)
    pad[:HW] = x
    total = f64(0.0)
    for b in _block_sums(pad.reshape(blocks, PIX, 256)):
        total = total + b
    return total


def depth_l1(a, b, view_keep=None, depth_trunc=np.inf):
    """float32 [n + 1, 8] (ROW)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    n, HW = a.shape[0], a.shape[1] * a.shape[2]
    trunc = f32(depth_trunc)
    table = np.full((n + 1, 8), np.nan, f32)
    for k in range(n):
        if view_keep is not None and not view_keep[k]:
            continue
        av, bv = a[k].reshape(HW), b[k].reshape(HW)
        ha, hb = (av > 0) & (av <= trunc), bv > 0
        diff = np.where(ha, av.astype(f64), 0.0) - np.where(hb, bv.astype(f64), 0.0)
        ad, valid = np.abs(diff), ha & hb
        s0, s1, s2 = _view_sum(np.where(valid, ad, 0.0)), _view_sum(np.where(valid, diff * diff, 0.0)), _view_sum(ad)
        both = f64(valid.sum())
        with np.errstate(all="ignore"):
            table[k] = [f32(s0 / both), f32(s2 / f64(HW)) if both > 0 else np.nan, f32(np.sqrt(s1 / both)), both, (ha & ~hb).sum(), (hb & ~ha).sum(),
                        (~ha & ~hb).sum(), ad[valid].astype(f32).max() if both > 0 else 0.0]
    for q in range(8):
        col = table[:n, q]
        col = col[col == col].astype(f64)
        if len(col) == 0:
            continue
        s = f64(0.0)
        for x in col:
            s = s + x
        table[n, q] = f32(s / f64(len(col))) if q < 3 else (f32(s) if q < 7 else col.max())
    return table
