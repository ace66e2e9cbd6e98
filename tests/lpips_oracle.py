"""LPIPS as the reference evaluates it — SLAM/eval.py:28-30, :65-68: LearnedPerceptualImagePatchSimilarity(net_type="alex",
normalize=True) of clamp(gt, 0, 1) and clamp(image, 0, 1), a batch of one — restated with torch CPU operators, in float64 (the oracle) or,
with dtype=torch.float32, in the arithmetic the reference's libraries themselves compute in.

Neither `lpips` nor `torchmetrics` exists on this platform, and no AlexNet weights do.  This is the algorithm as the published sources of
the two packages state it, NOT a recording of their output, and the weights are seeded random tensors of the real shapes: what is held
to it is held to a restatement.

    1. x = clamp(x, 0, 1); x = 2 x - 1; s = (x - shift_c) / scale_c, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450),
       each statement in float32 (the constants are float32), then widened to dtype
    2. f0 = relu(conv(s, 11, stride 4, pad 2)), f1 = relu(conv(maxpool3/2(f0), 5, pad 2)), f2 = relu(conv(maxpool3/2(f1), 3, pad 1)),
       f3 = relu(conv(f2, 3, pad 1)), f4 = relu(conv(f3, 3, pad 1)); zero padding, floor-mode pools
    3. per layer and pixel: na = a / sqrt(1e-8 + sum_c a^2) ("torchmetrics") or a / (sqrt(sum_c a^2) + 1e-10) ("lpips");
       v = sum_c lin[c] (na_c - nb_c)^2
    4. d_l = mean of v over the pixels; lpips = d_0 + .. + d_4

The row (dqo_eval.LPIPS_ROW): 0 lpips, 1..5 d_0..d_4, 6 and 7 NaN."""
import torch
import torch.nn.functional as F

NET = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))  # Cin, Cout, kernel, stride, pad
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
SLOTS = 8


def sizes(W, H):
    """((h0, w0), .., (h4, w4)): h0 = (H - 7) // 4 + 1, h1 = (h0 - 3) // 2 + 1, h2 = h3 = h4 = (h1 - 3) // 2 + 1."""
    def side(n):
        a = (n - 7) // 4 + 1
        b = (a - 3) // 2 + 1
        c = (b - 3) // 2 + 1
        return a, b, c, c, c
    return tuple(zip(side(H), side(W)))


def make_weights(seed=0):
    """Seeded weights of the real shapes from a CPU generator: He-scaled convolution weights (std sqrt(2 / (Cin k k))), 0.1 randn biases,
    non-negative lin vectors (|randn| / Cout: a layer term comes out between 1e-5 and 1e-2).  Returns (conv_w, conv_b, lin): three lists of five
    float32 CPU tensors."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    conv_w, conv_b, lin = [], [], []
    for cin, cout, k, _, _ in NET:
        conv_w.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        conv_b.append(0.1 * torch.randn(cout, generator=g))
        lin.append(torch.randn(cout, generator=g).abs() / cout)
    return conv_w, conv_b, lin


def one_hot_weights(seed=0):
    """Convolution weights with a single 1 per output channel at a seeded tap, zero biases (and make_weights' lin vectors): an output
    element is then one input value, whatever the order of the sum — the exact check of the gather."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    conv_w, conv_b = [], []
    for cin, cout, k, _, _ in NET:
        w = torch.zeros(cout, cin * k * k)
        w[torch.arange(cout), torch.randint(0, cin * k * k, (cout,), generator=g)] = 1.0
        conv_w.append(w.reshape(cout, cin, k, k))
        conv_b.append(torch.zeros(cout))
    return conv_w, conv_b, make_weights(seed)[2]


def scaled_input(x, dtype):
    """Step 1 of a [3,H,W] image, float32 statement by statement, widened to dtype."""
    x = x.detach().to("cpu", torch.float32).clamp(0.0, 1.0)
    x = 2.0 * x
    x = x - 1.0
    x = x - torch.tensor(SHIFT, dtype=torch.float32).view(3, 1, 1)
    x = x / torch.tensor(SCALE, dtype=torch.float32).view(3, 1, 1)
    return x.to(dtype)


def features(x, conv_w, conv_b, dtype=torch.float64, magnitude=False):
    """The five maps [C,h,w] of one [3,H,W] image.  magnitude=True: also, per map, conv2d(|input|, |w|) + |b| — the sum of the magnitudes
    of an output element's terms, the scale its rounding error is held against."""
    t = scaled_input(x, dtype)[None]
    maps, mags = [], []
    for l, (cin, cout, k, stride, pad) in enumerate(NET):
        if l in (1, 2):
            t = F.max_pool2d(t, 3, 2)
        w, b = conv_w[l].to(dtype), conv_b[l].to(dtype)
        if magnitude:
            mags.append((F.conv2d(t.abs(), w.abs(), b.abs(), stride=stride, padding=pad))[0])
        t = F.relu(F.conv2d(t, w, b, stride=stride, padding=pad))
        maps.append(t[0])
    return (maps, mags) if magnitude else maps


def lpips_row(image, gt, conv_w, conv_b, lin, dtype=torch.float64, norm="torchmetrics"):
    """The row of dqo_eval.lpips as a float64 [8] tensor (slots 6, 7 NaN), every step in dtype."""
    fa, fb = features(image, conv_w, conv_b, dtype), features(gt, conv_w, conv_b, dtype)
    row = torch.full((SLOTS,), float("nan"), dtype=torch.float64)
    total = torch.zeros((), dtype=dtype)
    for l in range(5):
        a, b = fa[l], fb[l]
        if norm == "torchmetrics":
            na, nb = a / torch.sqrt(1e-8 + (a * a).sum(0, keepdim=True)), b / torch.sqrt(1e-8 + (b * b).sum(0, keepdim=True))
        elif norm == "lpips":
            na, nb = a / (torch.sqrt((a * a).sum(0, keepdim=True)) + 1e-10), b / (torch.sqrt((b * b).sum(0, keepdim=True)) + 1e-10)
        else:
            raise ValueError(norm)
        v = (lin[l].reshape(-1, 1, 1).to(dtype) * (na - nb) ** 2).sum(0)
        d = v.mean()
        row[1 + l] = d.double()
        total = total + d
    row[0] = total.double()
    return row
