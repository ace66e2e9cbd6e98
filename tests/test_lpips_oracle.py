"""CPU: the LPIPS restatement (tests/lpips_oracle.py) against itself, and dqo_eval's weight packing.  No GPU, no built kernel."""
import pytest
import torch
import torch.nn.functional as F

import lpips_oracle as LO

pytestmark = pytest.mark.filterwarnings("ignore")


@pytest.fixture(scope="module")
def weights():
    return LO.make_weights(0)


def pair(H, W, seed=1):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    a = torch.rand(3, H, W, generator=g)
    b = (a + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return a, b


def test_size_formula_is_what_torch_produces():
    """One row of H = 31..70 against one column of W = 31..70: the sides are independent, so 40 + 40 shapes cover the 1 600 pairs."""
    import dqo_eval
    for n in range(31, 71):
        t = torch.zeros(1, 1, n, 31)
        got = []
        for l, (_, _, k, stride, pad) in enumerate(LO.NET):
            if l in (1, 2):
                t = F.max_pool2d(t, 3, 2)
            t = F.conv2d(t, torch.zeros(1, 1, k, k), stride=stride, padding=pad)
            got.append(t.shape[2])
        for m in (31, 70):
            assert tuple(s[0] for s in LO.sizes(m, n)) == tuple(got), n  # n as H
            assert tuple(s[1] for s in LO.sizes(n, m)) == tuple(got), n  # n as W
        assert dqo_eval.lpips_sizes(31, n) == LO.sizes(31, n) and dqo_eval.lpips_sizes(n, 70) == LO.sizes(n, 70)
    assert LO.sizes(31, 31) == ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1))
    assert LO.sizes(67, 45)[:3] == ((10, 16), (4, 7), (1, 3))
    assert LO.sizes(1200, 680)[:3] == ((169, 299), (84, 149), (41, 74)) and LO.sizes(159, 143)[:3] == ((35, 39), (17, 19), (8, 9))


@pytest.mark.parametrize("norm", ["torchmetrics", "lpips"])
def test_identical_images_give_zero_and_the_value_is_symmetric(weights, norm):
    a, b = pair(45, 67)
    for dtype in (torch.float32, torch.float64):
        z = LO.lpips_row(a, a.clone(), *weights, dtype=dtype, norm=norm)
        assert (z[:6] == 0).all() and torch.isnan(z[6:]).all()
        ab, ba = LO.lpips_row(a, b, *weights, dtype=dtype, norm=norm), LO.lpips_row(b, a, *weights, dtype=dtype, norm=norm)
        assert torch.equal(ab[:6], ba[:6]) and (ab[:6] > 0).all()


def test_the_two_norms_differ_and_the_clamp_acts(weights):
    a, b = pair(45, 67)
    t, p = LO.lpips_row(a, b, *weights), LO.lpips_row(a, b, *weights, norm="lpips")
    assert not torch.equal(t[:6], p[:6]) and torch.allclose(t[:6], p[:6], rtol=1e-3)
    wide = a * 1.4 - 0.2
    assert torch.equal(LO.lpips_row(wide, b, *weights)[:6], LO.lpips_row(wide.clamp(0, 1), b, *weights)[:6])
    assert float(t[0]) == pytest.approx(float(t[1:6].sum()), rel=1e-12)


@pytest.mark.parametrize("H,W", [(31, 31), (45, 67), (97, 130)])
def test_float32_restatement_is_close_to_float64(weights, H, W):
    """1e-5 relative per layer term and in total.  float32 carries 6e-8 per rounding and a term is a mean over at least one pixel of a
    sum over at least 64 channels behind chains of up to 3 456 products; the worst found at these sizes is 7.2e-7 (printed below)."""
    a, b = pair(H, W)
    for norm in ("torchmetrics", "lpips"):
        r32, r64 = LO.lpips_row(a, b, *weights, dtype=torch.float32, norm=norm), LO.lpips_row(a, b, *weights, dtype=torch.float64, norm=norm)
        rel = ((r32[:6] - r64[:6]).abs() / r64[:6].abs())
        print(H, W, norm, "worst relative error of the float32 restatement:", float(rel.max()))
        assert (rel <= 1e-5).all(), rel


def test_weight_packing(weights):
    import dqo_eval
    conv_w, conv_b, lin = weights
    packed = dqo_eval.LpipsWeights(conv_w, conv_b, lin, "cpu").packed
    assert packed.dtype == torch.float32 and packed.numel() == 2470848 == sum(ci * k * k * co + 2 * co for ci, co, k, _, _ in LO.NET)
    # layer 1: W[k][co], k = (kh * 5 + kw) * 64 + ci, behind layer 0's 363 * 64 + 64 + 64 floats; then the bias and the lin vector
    base = 363 * 64 + 128
    for co, ci, kh, kw in ((0, 0, 0, 0), (5, 7, 1, 2), (191, 63, 4, 4)):
        assert packed[base + ((kh * 5 + kw) * 64 + ci) * 192 + co] == conv_w[1][co, ci, kh, kw]
    assert torch.equal(packed[base + 1600 * 192:base + 1600 * 192 + 192], conv_b[1])
    assert torch.equal(packed[base + 1600 * 192 + 192:base + 1600 * 192 + 384], lin[1])
    assert torch.equal(packed[-256:], lin[4]) and packed[0] == conv_w[0][0, 0, 0, 0] and packed[64 * 3 + 1] == conv_w[0][1, 0, 0, 1]
    # the state dicts of the published sources pack the same buffer
    alex = {}
    for l, i in enumerate((0, 3, 6, 8, 10)):
        alex[f"features.{i}.weight"], alex[f"features.{i}.bias"] = conv_w[l], conv_b[l]
    lins = {f"lin{l}.model.1.weight": lin[l].reshape(1, -1, 1, 1) for l in range(5)}
    assert torch.equal(dqo_eval.LpipsWeights.from_state_dicts(alex, lins).packed, packed)
    # a wrong shape raises
    for what, bad in (("conv_w", [conv_w[1]] + conv_w[1:]), ("conv_b", conv_b[:4] + [conv_b[4][:-1]]), ("lin", lin[:2] + [lin[2].reshape(-1, 1)] + lin[3:])):
        args = dict(conv_w=conv_w, conv_b=conv_b, lin=lin)
        args[what] = bad
        with pytest.raises(RuntimeError, match=what):
            dqo_eval.LpipsWeights(args["conv_w"], args["conv_b"], args["lin"], "cpu")
    with pytest.raises(RuntimeError, match="five"):
        dqo_eval.LpipsWeights(conv_w[:4], conv_b, lin, "cpu")


def test_python_surface():
    import dqo_eval
    assert dqo_eval.LPIPS_ROW[:6] == ("lpips", "d0", "d1", "d2", "d3", "d4") and len(dqo_eval.LPIPS_ROW) == 8
    assert dqo_eval.LPIPS_NET == LO.NET
    # lpips_row: the dict gains "lpips"; without it the dict is what it was, key for key
    row = torch.arange(8, dtype=torch.float32)
    assert list(dqo_eval.eval_picture_dict(row)) == ["valid_pixel_ratio", "depth_loss", "normal_loss", "psnr", "ssim", "color_loss"]
    both = torch.arange(36, dtype=torch.float32) + 100
    for r, m, p in ((both[:8], both[8:28], both[28:]), (row, both[8:28], both[28:].clone())):  # one storage: one read; else one per row
        d = dqo_eval.eval_picture_dict(r, ms_row=m, lpips_row=p)
        assert d["lpips"] == 128.0 and d["ssim"] == 108.0 and d["ssim_single_scale"] == float(r[4]) and d["psnr"] == float(r[0])
        d = dqo_eval.eval_picture_dict(r, lpips_row=p)
        assert d["lpips"] == 128.0 and d["ssim"] == float(r[4]) and "ssim_single_scale" not in d
        assert dqo_eval.eval_picture_dict(r, ms_row=m) == {k: v for k, v in dqo_eval.eval_picture_dict(r, m, p).items() if k != "lpips"}
    w = dqo_eval.LpipsWeights(*LO.one_hot_weights(0), "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.lpips(torch.zeros(3, 40, 40), torch.zeros(3, 40, 40), w)
