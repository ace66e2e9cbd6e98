"""GPU: LPIPS of a rendered frame (dqo_eval.lpips, FusedMapper.evaluate_lpips — csrc/map_lpips.hip) against the float64 restatement of the
published algorithm (tests/lpips_oracle.py) on seeded random weights of the real shapes.  Nothing here was recorded from `lpips` or
`torchmetrics`: neither exists on this platform.

The bars, with their reasons:
    feature maps   |hip - f64| <= 1e-6 * (sum_k |w_k| |x_k| + |b|) per element, the sum from the oracle's conv2d of magnitudes.  A serial
                   float chain of K = 4096 terms is about 3.5e-7 of that sum and ours is at most K = 3456; the float32 restatement,
                   its error chained through all five layers, stays within 2.8e-7 of it at these sizes.  About 3 x margin over both.
    the row        slots 0..5 within 1e-5 relative of the float64 oracle (the float32 restatement is within 1e-6 of it,
                   tests/test_lpips_oracle.py prints the figure), slots 6 and 7 NaN.

The sizes (H x W): 31 x 31, the minimum — maps of 7 x 7, 3 x 3, 1 x 1, the pools consume exactly their window, every layer less than
two 64-row tiles; 45 x 67 — maps of 10 x 16, 4 x 7, 1 x 3: layer 0 is exactly five row tiles, the others end inside their first;
97 x 130 — maps of 23 x 31, 11 x 15, 5 x 7: 23, 6 and 2 row tiles of 64, each with a tail, and the two images meet inside a tile at
every layer; 143 x 159 — the smallest whose last three maps (8 x 9, 144 rows) fill more than one of the 128-row tiles layers 3 and 4
use: a full tile, in which the two images meet, and a tail of 16 rows.  K = 363 ends inside its last chunk of 16 at every size."""
import functools

import numpy as np
import pytest

import lpips_oracle as LO

pytestmark = pytest.mark.gpu

SIZES = [(31, 31), (45, 67), (97, 130), (143, 159)]  # H, W
FEATURE_BAR, ROW_BAR = 1e-6, 1e-5


def _pair(H, W, seed=1):
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    a = torch.rand(3, H, W, generator=g)
    b = (a + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return a, b


def _wide_pair(H, W):
    """Values in [-0.2, 1.2]: the clamp acts on about a quarter of them."""
    a, b = _pair(H, W, 2)
    return a * 1.4 - 0.2, b * 1.4 - 0.2


@functools.lru_cache(maxsize=None)
def _cpu_weights(kind):
    return LO.make_weights(0) if kind == "random" else LO.one_hot_weights(0)


@functools.lru_cache(maxsize=None)
def _weights(kind):
    """dqo_eval.LpipsWeights on the device; made once, shared, never written to."""
    import dqo_eval
    return dqo_eval.LpipsWeights(*_cpu_weights(kind), "cuda")


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(a, b, the float64 maps and magnitude sums of both, the float64 rows of both norms); computed once, shared, never written to."""
    import torch
    a, b = _pair(H, W)
    conv_w, conv_b, lin = _cpu_weights("random")
    fa, ma = LO.features(a, conv_w, conv_b, torch.float64, magnitude=True)
    fb, mb = LO.features(b, conv_w, conv_b, torch.float64, magnitude=True)
    rows = {norm: LO.lpips_row(a, b, conv_w, conv_b, lin, torch.float64, norm).numpy() for norm in ("torchmetrics", "lpips")}
    return a, b, (fa, fb), (ma, mb), rows


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _assert_row(got, want, what):
    got = np.asarray(got, np.float64)
    for k in range(6):
        print(f"{what} slot {k} got {got[k]!r} want {want[k]!r} relative {abs(got[k] - want[k]) / abs(want[k]):.3e} bar {ROW_BAR:.0e}")
    assert np.isnan(got[6]) and np.isnan(got[7]), (what, got)
    for k in range(6):
        assert abs(got[k] - want[k]) <= ROW_BAR * abs(want[k]), (what, k, got[k], want[k])


@pytest.mark.parametrize("H,W", SIZES)
def test_every_feature_map_and_the_row_equal_the_float64_oracle(H, W):
    import torch
    import dqo_eval
    a, b, maps, mags, rows = _case(H, W)
    assert (rows["torchmetrics"][:6] > 1e-6).all(), rows  # (no layer term is a rounding's size)
    ws = dqo_eval.lpips_workspace(W, H, "cuda")
    row = dqo_eval.lpips(a.cuda(), b.cuda(), _weights("random"), workspace_buffer=ws)
    torch.cuda.synchronize()
    assert row.dtype == torch.float32 and tuple(row.shape) == (8,) and row.is_cuda
    for l in range(5):
        got = dqo_eval.lpips_feature_view(ws, W, H, l).cpu().double()
        assert tuple(got.shape) == (2,) + LO.sizes(W, H)[l] + (LO.NET[l][1],)
        for i in range(2):
            want, mag = maps[i][l].permute(1, 2, 0), mags[i][l].permute(1, 2, 0)
            ratio = ((got[i] - want).abs() / mag).max().item()
            print(f"{H}x{W} layer {l} image {i}: worst |hip - f64| / (sum |w||x| + |b|) = {ratio:.3e}, bar {FEATURE_BAR:.0e}; "
                  f"{int((want > 0).sum())} of {want.numel()} elements positive")
            assert (want > 0).any() and ((got[i] - want).abs() <= FEATURE_BAR * mag).all(), (l, i, ratio)
    _assert_row(row.cpu().numpy(), rows["torchmetrics"], f"{H}x{W} torchmetrics")
    other = dqo_eval.lpips(a.cuda(), b.cuda(), _weights("random"), norm="lpips", workspace_buffer=ws)
    _assert_row(other.cpu().numpy(), rows["lpips"], f"{H}x{W} lpips")  # (the two norms differ by 1e-9 relative here: below a float's step)


@pytest.mark.parametrize("H,W", SIZES)
def test_one_hot_weights_give_the_float32_oracle_bit_for_bit(H, W):
    """A single 1 per output channel, zero bias: an output element is one input value whatever the order of the sum, so this holds the
    gather, the padding, the stride, the packed k order and the pixel-major layout exactly — on clamped-range inputs as well."""
    import torch
    import dqo_eval
    a, b = _wide_pair(H, W)
    conv_w, conv_b, _ = _cpu_weights("one_hot")
    ws = dqo_eval.lpips_workspace(W, H, "cuda")
    dqo_eval.lpips(a.cuda(), b.cuda(), _weights("one_hot"), workspace_buffer=ws)
    torch.cuda.synchronize()
    want = [LO.features(x, conv_w, conv_b, torch.float32) for x in (a, b)]
    for l in range(5):
        got = dqo_eval.lpips_feature_view(ws, W, H, l)
        for i in range(2):
            w = want[i][l].permute(1, 2, 0).contiguous() + 0.0  # (+ 0.0: a -0 of the CPU's sum becomes the +0 a chain from +0 gives)
            assert (w > 0).any() or (H, W) not in SIZES[2:]  # (a 1 x 1 map's taps lie in the padding but for one in nine)
            assert _bits(got[i]).tobytes() == _bits(w).tobytes(), (l, i, int((got[i].cpu() != w).sum()))


def test_exact_properties():
    """(b) identical images: +0 in slots 0..5; (c) symmetric, bit for bit; (d) two calls on one workspace: the same bits, and the ticket
    words are zero afterwards; (e) inputs outside [0, 1]: the bits of the clamped inputs."""
    import torch
    import dqo_eval
    H, W = 45, 67
    a, b = (t.cuda() for t in _pair(H, W))
    wts, ws = _weights("random"), dqo_eval.lpips_workspace(W, H, "cuda")
    same = _bits(dqo_eval.lpips(a, a.clone(), wts, workspace_buffer=ws))
    assert (same[:6] == 0).all(), same  # (+0: all bits clear)
    assert (_bits(dqo_eval.lpips(a, a, wts, workspace_buffer=ws))[:6] == 0).all()
    ab, ba = _bits(dqo_eval.lpips(a, b, wts, workspace_buffer=ws)), _bits(dqo_eval.lpips(b, a, wts, workspace_buffer=ws))
    assert ab.tobytes() == ba.tobytes() and (ab[:6] != 0).all()
    again = _bits(dqo_eval.lpips(a, b, wts, workspace_buffer=ws))
    torch.cuda.synchronize()
    assert again.tobytes() == ab.tobytes() and len(ab.tobytes()) == 32
    assert int(ws[:4352].view(torch.int32).abs().sum().item()) == 0  # (DQO_REDUCE_HEAD_WORDS: the ticket words)
    for norm in ("torchmetrics", "lpips"):
        assert _bits(dqo_eval.lpips(a, b, wts, norm=norm)).tobytes() == _bits(dqo_eval.lpips(a, b, wts, norm=norm, workspace_buffer=ws)).tobytes()
    wa, wb = (t.cuda() for t in _wide_pair(H, W))
    assert (wa < 0).any() and (wa > 1).any()
    wide, clamped = _bits(dqo_eval.lpips(wa, wb, wts)), _bits(dqo_eval.lpips(wa.clamp(0, 1), wb.clamp(0, 1), wts))
    assert wide.tobytes() == clamped.tobytes() and wide.tobytes() != ab.tobytes()


def test_a_table_row_is_the_single_row_and_an_overflowed_render_gives_nan():
    """(f) out= / row= writes one row of a [3,8] table and leaves the others; (g) a render header marked overflowed gives eight NaN."""
    import torch
    import dqo_eval
    H, W = 45, 67
    a, b, _, _, rows = _case(H, W)
    a, b, wts = a.cuda(), b.cuda(), _weights("random")
    single = _bits(dqo_eval.lpips(a, b, wts))
    sentinel = 0x7FC0ABCD  # (a NaN with a payload: only a bit comparison sees it)
    table = torch.full((3, 8), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    r = dqo_eval.lpips(a, b, wts, out=table, row=1)
    torch.cuda.synchronize()
    t = _bits(table)
    assert r.data_ptr() == table[1].data_ptr() and t[1].tobytes() == single.tobytes() and (t[[0, 2]] == sentinel).all()
    header = torch.zeros((8,), dtype=torch.int32, device="cuda")  # DqoRastHeader: word 2 = overflow
    header[2] = 1
    got = dqo_eval.lpips(a, b, wts, render_header=header.view(torch.uint8)).cpu().numpy()
    assert np.isnan(got).all(), got
    header[2] = 0
    _assert_row(dqo_eval.lpips(a, b, wts, render_header=header.view(torch.uint8)).cpu().numpy(), rows["torchmetrics"], "clean header")


def test_capturable_in_a_graph():
    """One capture at 45 x 67, a single stream and no branches, replayed twice on changed inputs: the eager bits."""
    import torch
    import dqo_eval
    H, W = 45, 67
    wts = _weights("random")
    frames = [_pair(H, W, s) for s in (21, 22, 23)]
    eager = [_bits(dqo_eval.lpips(x.cuda(), y.cuda(), wts)) for x, y in frames]
    x, y = (t.cuda() for t in frames[0])
    table = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (the module's workspace for this size exists: nothing is allocated while capturing)
        dqo_eval.lpips(x, y, wts, out=table, row=0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dqo_eval.lpips(x, y, wts, out=table, row=0)
    for k in (1, 2):
        x.copy_(frames[k][0].cuda()), y.copy_(frames[k][1].cuda())
        g.replay()
        torch.cuda.synchronize()
        assert _bits(table)[0].tobytes() == eager[k].tobytes(), k
    assert eager[1].tobytes() != eager[2].tobytes()


def _scene():
    """An 8 k Gaussian frustum cloud at 160 x 120 seen from three cameras; every camera's target is the render of a perturbed copy."""
    import torch
    from dqo_harness import mapping, scenes
    dev = torch.device("cuda")
    cams = [scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]), (11.0, -6.0, [0.15, -0.05, 0.0]))]
    scene = scenes.frustum_cloud(17, 8000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    targets = [mapping.perturbed_target(scene, st, dev, 40 + k) for k, st in enumerate(settings)]
    return dev, scene, settings, targets


def test_evaluate_lpips_fills_its_table_from_the_same_render():
    import torch
    import dqo_eval
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _scene()
    wts = _weights("random")
    fm = FusedMapper(scene, settings[0], dev)
    frames = [(None if k == 0 else st, t["gt_color"], t["gt_depth"]) for k, (st, t) in enumerate(zip(settings, targets))]
    with pytest.raises(RuntimeError, match=r"\[3,8\]"):  # a [K,7] table: refused before anything is rendered
        fm.evaluate_lpips(frames, torch.zeros((3, 7), dtype=torch.float32, device=dev), wts)
    assert fm._maintain_ctx is None
    plain = _bits(fm.evaluate(frames, min_depth=0.3, max_depth=5.0))
    sentinel = 0x7FC0ABCD
    table8 = torch.full((3, 8), sentinel, dtype=torch.int32, device=dev).view(torch.float32)
    table = fm.evaluate_lpips(frames, table8, wts, min_depth=0.3, max_depth=5.0)
    torch.cuda.synchronize()
    assert _bits(table).tobytes() == plain.tobytes()  # the picture table does not know about the other one
    before = torch.cuda.memory_allocated()  # after the first call nothing is allocated and nothing is read
    torch.cuda.set_sync_debug_mode("error")
    try:
        fm.evaluate_lpips(frames, table8, wts, min_depth=0.3, max_depth=5.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    opacity, scales, rotations = fm.activate()
    for k, (st, t) in enumerate(zip(settings, targets)):
        ref = mapping.render(st, dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs))
        want = dqo_eval.lpips(ref["render"], t["gt_color"], wts)
        got = table8[k].cpu().numpy()
        assert _bits(table8[k]).tobytes() == _bits(want).tobytes(), (k, got, want.cpu().numpy())
        assert np.isfinite(got[:6]).all() and got[0] > 0 and np.isnan(got[6:]).all(), (k, got)
        d = dqo_eval.eval_picture_dict(table[k], lpips_row=table8[k])
        assert d["lpips"] == float(got[0]) and d["psnr"] == float(table[k, 0]) and "ssim_single_scale" not in d


def test_refusals_come_before_any_launch():
    import torch
    import dqo_eval
    wts = _weights("random")
    ok = torch.zeros((3, 40, 50), dtype=torch.float32, device="cuda")
    small = torch.zeros((3, 30, 50), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="31"):
        dqo_eval.lpips(small, small, wts)
    with pytest.raises(RuntimeError, match=r"\[K,8\]"):
        dqo_eval.lpips(ok, ok, wts, out=torch.zeros((4, 7), dtype=torch.float32, device="cuda"), row=0)
    with pytest.raises(RuntimeError, match="norm"):
        dqo_eval.lpips(ok, ok, wts, norm="vgg")
    with pytest.raises(RuntimeError, match="LpipsWeights"):
        dqo_eval.lpips(ok, ok, wts.packed)
    with pytest.raises(RuntimeError, match=r"\[3,40,50\]"):
        dqo_eval.lpips(ok, torch.zeros((3, 40, 49), dtype=torch.float32, device="cuda"), wts)
