"""Times one dqo_eval.lpips call (dqo_eval_lpips, csrc/map_lpips.hip: twelve launches) at 1200 x 680 on seeded random weights of the
real shapes, and beside it the same four steps written with torch operators on the same GPU (F.conv2d, F.max_pool2d and the rest,
float32) — what a user of the library would run without it.  Device events around the calls, warmed up, the two sides alternating; the
library's own per-launch timers give the split.  For every convolution the least time the f32 matrix rate allows (2 M N K FLOP over
157.3 TFLOP/s, M = the output pixels of both images) is printed next to its launch, with the share of it the launch achieves.

    python tools/profile_lpips.py [--w 1200] [--h 680] [--reps 50] [--rounds 5] > profiles/lpips_1200x680.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

import torch
import torch.nn.functional as F

F32_MATRIX_PEAK = 157.3e12  # FLOP / s, f32-input MFMA
WARMUP = 5
NET = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))  # Cin, Cout, kernel, stride, pad


def seeded_weights(seed=0):
    """He-scaled convolution weights, 0.1 randn biases, non-negative lin vectors, from a CPU generator."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    conv_w, conv_b, lin = [], [], []
    for cin, cout, k, _, _ in NET:
        conv_w.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        conv_b.append(0.1 * torch.randn(cout, generator=g))
        lin.append(torch.randn(cout, generator=g).abs() / cout)
    return conv_w, conv_b, lin


def torch_lpips(image, gt, conv_w, conv_b, lin, shift, scale):
    """The four steps with torch operators, float32, both images as a batch of two; returns the value as a device scalar."""
    t = (2.0 * torch.stack([image, gt]).clamp(0.0, 1.0) - 1.0 - shift) / scale
    total = None
    for l, (_, _, _, stride, pad) in enumerate(NET):
        if l in (1, 2):
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, conv_w[l], conv_b[l], stride=stride, padding=pad))
        n = t / torch.sqrt(1e-8 + (t * t).sum(1, keepdim=True))
        d = (lin[l].view(1, -1, 1, 1) * (n[0:1] - n[1:2]) ** 2).sum(1).mean()
        total = d if total is None else total + d
    return total


def timed(f, reps):
    """The times of `reps` calls in ms, device events around each."""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1200)
    ap.add_argument("--h", type=int, default=680)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_lpips: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
    import dqo_eval
    dev = torch.device("cuda")
    W, H = a.w, a.h
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    image = torch.rand(3, H, W, generator=g)
    gt = (image + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
    image = image.to(dev)
    conv_w, conv_b, lin = seeded_weights(0)
    weights = dqo_eval.LpipsWeights(conv_w, conv_b, lin, dev)
    conv_w, conv_b, lin = ([t.to(dev) for t in ts] for ts in (conv_w, conv_b, lin))
    shift = torch.tensor([-0.030, -0.088, -0.188], device=dev).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=dev).view(1, 3, 1, 1)
    sizes = dqo_eval.lpips_sizes(W, H)
    flops = [2.0 * 2 * h * w * cout * cin * k * k for (h, w), (cin, cout, k, _, _) in zip(sizes, NET)]
    print(f"device: {torch.cuda.get_device_name(0)}   image {W} x {H}, maps " + " ".join(f"{h}x{w}x{n[1]}" for (h, w), n in zip(sizes, NET)))
    print(f"convolutions: {sum(flops) / 1e9:.2f} GFLOP for the two images; at {F32_MATRIX_PEAK / 1e12:.1f} TFLOP/s: {sum(flops) / F32_MATRIX_PEAK * 1e3:.3f} ms")

    table = torch.zeros((1, 8), dtype=torch.float32, device=dev)
    ours = lambda: dqo_eval.lpips(image, gt, weights, out=table, row=0)
    try:
        theirs = lambda: torch_lpips(image, gt, conv_w, conv_b, lin, shift, scale)
        value = float(theirs())
    except Exception as e:  # (torch's convolution needs its own library on the machine)
        theirs, value = None, None
        print(f"torch operators: F.conv2d does not run here ({type(e).__name__}: {e}); ours alone")
    for _ in range(WARMUP):
        ours()
        if theirs is not None:
            theirs()
    torch.cuda.synchronize()
    print(f"value: ours {float(table[0, 0])!r}" + ("" if value is None else f", torch operators (float32) {value!r}"))
    t_ours, t_theirs = [], []
    for _ in range(a.rounds):  # the two sides alternate
        t_ours += timed(ours, a.reps)
        if theirs is not None:
            t_theirs += timed(theirs, a.reps)
    n = len(t_ours)
    print(f"dqo_eval.lpips (twelve launches): median {statistics.median(t_ours):.3f} ms, least {min(t_ours):.3f} ms of {n} calls in {a.rounds} rounds; "
          f"the convolutions' floor is {sum(flops) / F32_MATRIX_PEAK * 1e3 / statistics.median(t_ours) * 100:.1f} % of the median")
    if theirs is not None:
        print(f"torch operators (F.conv2d, F.max_pool2d, elementwise; float32): median {statistics.median(t_theirs):.3f} ms, least {min(t_theirs):.3f} ms "
              f"of {n} calls; ours is {statistics.median(t_theirs) / statistics.median(t_ours):.2f} x as fast at the median")
    N.profile_enable(True)
    N.profile_collect()
    for _ in range(20):
        ours()
    prof = N.profile_collect()
    N.profile_enable(False)
    total = sum(ms / max(1, calls) for ms, calls in prof.values())
    print(f"per launch (the library's timers, which serialise the launches; their sum is {total:.3f} ms):")
    for name in sorted(prof):
        ms, calls = prof[name]
        per = ms / max(1, calls)
        line = f"  {name}: {per * 1e3:.1f} us"
        if name.startswith("lpips_conv"):
            l = int(name[-1])
            floor = flops[l] / F32_MATRIX_PEAK * 1e3
            line += (f"   {flops[l] / 1e9:.2f} GFLOP, floor {floor * 1e3:.1f} us, {floor / per * 100:.1f} % of the f32 matrix rate "
                     f"({flops[l] / (per * 1e-3) / 1e12:.1f} TFLOP/s)")
        print(line)


if __name__ == "__main__":
    main()
