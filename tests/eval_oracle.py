"""Test-side oracle of dqo_eval_picture / dqo_eval.eval_picture (include/dqo_raster.h): a numpy FLOAT64 restatement of the eight slots —
eval_picture's statements (SLAM/eval.py:60-70, 115-126) with psnr / l1_loss / ssim of utils/loss_utils.py:23-29, 41-100.  Every
difference is formed in double from the float32 inputs, as the kernel forms it; tests/test_eval_oracle.py holds it to what the reference's own
functions return for the fixture (tests/golden/eval_golden.npz).

The five cases of the fixture are made here (fixture_cases) from the fixture's base arrays, so the script that records the reference's
results, the CPU test and the GPU test evaluate the same inputs."""
import numpy as np

ROW = ("psnr", "color_loss", "depth_loss", "valid_pixel_ratio", "ssim", "mse_r", "mse_g", "mse_b")
INPUTS = ("render", "gt_color", "depth", "gt_depth", "depth_index")
MIN_DEPTH, MAX_DEPTH = 0.3, 5.0  # configs/base.yaml:39-40


def ssim_window():
    """utils/loss_utils.py:41-57: float32(exp(..)) / their float32 sum, then the float32 outer product — the reference's window, as doubles."""
    g = np.array([np.exp(-((x - 5) ** 2) / (2 * 1.5 ** 2)) for x in range(11)]).astype(np.float32)
    g = (g / g.sum(dtype=np.float32)).astype(np.float32)
    return np.outer(g, g).astype(np.float32).astype(np.float64)


def _window_mean(x, w):
    """conv2d(x, window, padding=5, groups=channel) of a [3,H,W] image: zero padding, the same window on every channel."""
    C, H, W = x.shape
    p = np.zeros((C, H + 10, W + 10))
    p[:, 5:5 + H, 5:5 + W] = x
    out = np.zeros_like(x)
    for dy in range(11):
        for dx in range(11):
            out += w[dy, dx] * p[:, dy:dy + H, dx:dx + W]
    return out


def ssim(img1, img2):
    """utils/loss_utils.py:60-100 (window 11, size_average=True) in float64."""
    a, b, w = np.asarray(img1, np.float64), np.asarray(img2, np.float64), ssim_window()
    mu1, mu2 = _window_mean(a, w), _window_mean(b, w)
    s1, s2, s12 = _window_mean(a * a, w) - mu1 * mu1, _window_mean(b * b, w) - mu2 * mu2, _window_mean(a * b, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())


def eval_oracle(render, gt_color, depth, gt_depth, depth_index, min_depth, max_depth, with_ssim=True):
    """float64 [8] in ROW order (slot 4 NaN without with_ssim); valid_pixel_ratio is the float32 quotient of the two integers."""
    r, g = np.asarray(render, np.float32).astype(np.float64), np.asarray(gt_color, np.float32).astype(np.float64)
    HW = r.shape[-2] * r.shape[-1]
    d = (g - r).reshape(3, HW)
    mse = (d * d).sum(1) / HW
    gd32 = np.asarray(gt_depth, np.float32).reshape(HW)
    valid = (np.asarray(depth_index).reshape(HW) != -1) & (gd32 > np.float32(min_depth)) & (gd32 < np.float32(max_depth))
    n = int(valid.sum())
    err = np.abs(np.asarray(depth, np.float32).reshape(HW).astype(np.float64) - gd32.astype(np.float64))[valid].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = (20.0 * np.log10(1.0 / np.sqrt(mse))).mean()
        depth_loss = np.float64(err) / np.float64(n)
    return np.array([psnr, np.abs(d).sum() / (3.0 * HW), depth_loss, np.float32(n) / np.float32(HW),
                     ssim(render, gt_color) if with_ssim else np.nan, mse[0], mse[1], mse[2]], np.float64)


def fixture_cases(base):
    """[(name, {input name: array}, min_depth, max_depth)] x 5 from the fixture's base arrays (base["render"] ... base["depth_index"])."""
    b = {k: np.asarray(base[k]) for k in INPUTS}
    H, W = b["depth"].shape[-2:]
    none = np.full_like(b["depth_index"], -1)
    half = b["depth_index"].copy()
    half[..., : W // 2] = -1
    return [("generic", b, MIN_DEPTH, MAX_DEPTH),
            ("identical", dict(b, render=b["gt_color"].copy()), MIN_DEPTH, MAX_DEPTH),       # psnr = +inf
            ("no_valid_pixel", dict(b, depth_index=none), MIN_DEPTH, MAX_DEPTH),              # depth loss NaN
            ("all_out_of_range", b, 6.0, 9.0),                                                # every target depth outside (min, max)
            ("half_without_hit", dict(b, depth_index=half), MIN_DEPTH, MAX_DEPTH)]
