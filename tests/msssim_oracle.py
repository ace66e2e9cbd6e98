"""MS-SSIM as the reference evaluates it — eval_ssim, SLAM/eval.py:19-25: pytorch_msssim.ms_ssim(image[None], gt[None], data_range=1.0,
size_average=True) — restated with torch CPU operators, in float64 (the oracle) or, with dtype=torch.float32, in the arithmetic the
reference's library itself computes in.

pytorch_msssim does not exist on this platform.  This is the algorithm as the library's published source states it, NOT a recording of
its output: what is held to it is held to a restatement.

    window        float32(exp(-(i - 5)^2 / (2 * 1.5^2))), i = 0..10, divided by their float32 sum (utils/loss_utils.py:41-58), then widened
    filter        separable, VALID correlation: [h,w] -> [h-10,w-10]
    one level     mu1 = f(X), mu2 = f(Y), s1 = f(X X) - mu1^2, s2 = f(Y Y) - mu2^2, s12 = f(X Y) - mu1 mu2
                  cs = (2 s12 + C2) / (s1 + s2 + C2),  ss = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) * cs;  per channel: their means
    between       avg_pool2d(kernel_size=2, padding=(h % 2, w % 2)) (count_include_pad, floor mode)
    value         F[l][c] = max(mean cs, 0) for l = 0..3, F[4][c] = max(mean ss, 0); ms_c = prod_l F[l][c] ** w[l]; mean over c

The row (dqo_eval.MS_ROW): 0 ms_ssim, 1..3 ms_r / g / b, 4 + 3 l + c the factor F[l][c], 19 NaN."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
SLOTS = 20


def window(dtype=torch.float64):
    c = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def gaussian_filter(x, w):
    """x [1,C,h,w]: the window along H, then along W, no padding (a direction shorter than the window is skipped, as in the library)."""
    C = x.shape[1]
    out = x
    if x.shape[2] >= 11:
        out = F.conv2d(out, w.view(1, 1, 11, 1).repeat(C, 1, 1, 1), groups=C)
    if x.shape[3] >= 11:
        out = F.conv2d(out, w.view(1, 1, 1, 11).repeat(C, 1, 1, 1), groups=C)
    return out


def level(X, Y, w):
    """(mean ss, mean cs) per channel of one level."""
    mu1, mu2 = gaussian_filter(X, w), gaussian_filter(Y, w)
    s1 = gaussian_filter(X * X, w) - mu1 * mu1
    s2 = gaussian_filter(Y * Y, w) - mu2 * mu2
    s12 = gaussian_filter(X * Y, w) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ss = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    return ss.flatten(2).mean(-1)[0], cs.flatten(2).mean(-1)[0]


def pool(X):
    return F.avg_pool2d(X, kernel_size=2, padding=[s % 2 for s in X.shape[2:]])


def level_sizes(W, H):
    """The (w, h) of the five levels."""
    out = [(W, H)]
    for _ in range(4):
        W, H = W // 2 + W % 2, H // 2 + H % 2
        out.append((W, H))
    return out


def ms_ssim_row(image, gt, dtype=torch.float64, with_means=False):
    """image, gt: [3,H,W] arrays (float32 values).  Returns the 20 slots as a float64 numpy array; with_means: also the fifteen means
    the factors are clamped from, [5,3] (cs at levels 0..3, ss at level 4)."""
    X, Y = torch.as_tensor(np.asarray(image)).to(dtype)[None], torch.as_tensor(np.asarray(gt)).to(dtype)[None]
    assert min(X.shape[-2:]) > (11 - 1) * 2 ** 4, "the library's assertion"
    w = window(dtype)
    means = []
    for l in range(5):
        ss, cs = level(X, Y, w)
        if l < 4:
            means.append(cs)
            X, Y = pool(X), pool(Y)
    means.append(ss)
    means = torch.stack(means)  # [5,3]
    fac = torch.relu(means)
    wt = torch.tensor(WEIGHTS, dtype=torch.float32).to(dtype)
    per_channel = torch.prod(fac ** wt[:, None], 0)
    row = np.full((SLOTS,), np.nan)
    row[0] = float(per_channel.mean())
    row[1:4] = per_channel.to(torch.float64).numpy()
    row[4:19] = fac.to(torch.float64).numpy().reshape(-1)
    return (row, means.to(torch.float64).numpy()) if with_means else row


def structured(W, H, seed, noise):
    """(render, gt), float32 [3,H,W]: a smooth pattern per channel under N(0, 0.03), the render that plus N(0, noise) plus 0.02."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    gt = np.stack([0.5 + 0.25 * np.sin(x / (7.0 + 3 * c) + c) * np.cos(y / (5.0 + 2 * c)) + 0.15 * np.sin((x + 2 * y) / (31.0 + c))
                   for c in range(3)])
    gt = gt + rng.normal(0, 0.03, gt.shape)
    render = gt + rng.normal(0, noise, gt.shape) + 0.02
    return np.clip(render, 0, 1).astype(np.float32), np.clip(gt, 0, 1).astype(np.float32)


def uniform_pair(W, H, seed):
    """Two independent uniform images."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (3, H, W)).astype(np.float32), rng.uniform(0, 1, (3, H, W)).astype(np.float32)
