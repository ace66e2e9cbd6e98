"""GPU: MS-SSIM of a rendered frame (dqo_eval.ms_ssim, FusedMapper.evaluate_ms_ssim — csrc/map_msssim.hip) against the float64
restatement of pytorch_msssim's ms_ssim (tests/msssim_oracle.py).

The bars are MEASURED, not chosen: for the eight structured cases below (four shapes, two noise levels) the restatement is run in float32
— the arithmetic the reference's library computes in — and in float64, and the largest absolute difference over the factor slots 4..18
and over the value slots 0..3 is taken.  The kernel is held to the float64 oracle within 8 x that difference: its float32 filter adds in
another order than torch's, and the s = E[x^2] - mu^2 cancellation amplifies that by the same factor on both sides; eight is headroom for
order, not for a wrong formula (a pooling or window error is 1e-3 or more).  Measured with this file's inputs (torch CPU, float32 against
float64 of the RESTATEMENT — pytorch_msssim itself does not exist on this platform and nothing here was recorded from it):

    factors  (slots 4..18)   largest |f32 - f64| = 4.95e-06 (161 x 161, noise 0.02, level 4: one filtered pixel)   bar 3.96e-05
    values   (slots 0..3)    largest |f32 - f64| = 6.61e-07 (161 x 161, noise 0.02)                               bar 5.29e-06

The test recomputes both on every run (test_bars_are_the_measured_ones prints them) rather than trusting these lines."""
import functools

import numpy as np
import pytest

from msssim_oracle import ms_ssim_row, structured, uniform_pair

pytestmark = pytest.mark.gpu

SHAPES = [(161, 161), (176, 164), (203, 177), (640, 480)]  # the bars are measured on these
RAGGED_RUN = (500, 340)  # level 0: 31 x 21 tiles, a block takes four side by side, the last block of a tile row three
NOISES = (0.02, 0.1)
FACTORS, VALUES, USED = list(range(4, 19)), list(range(0, 4)), list(range(19))
HEADROOM = 8.0


@functools.lru_cache(maxsize=None)
def _case(W, H, noise):
    """(render, gt, float64 row, float32 row) of a structured case; computed once, shared, never written to."""
    import torch
    render, gt = structured(W, H, W + H, noise)
    return render, gt, ms_ssim_row(render, gt), ms_ssim_row(render, gt, torch.float32)


@functools.lru_cache(maxsize=None)
def _bars():
    """(factor bar, value bar): 8 x the largest float32-against-float64 difference of the restatement over all eight cases."""
    d_fac = d_val = 0.0
    for W, H in SHAPES:
        for noise in NOISES:
            _, _, r64, r32 = _case(W, H, noise)
            d_fac, d_val = max(d_fac, np.abs(r64[FACTORS] - r32[FACTORS]).max()), max(d_val, np.abs(r64[VALUES] - r32[VALUES]).max())
    return HEADROOM * d_fac, HEADROOM * d_val


def _gpu(*arrays):
    import torch
    return [torch.tensor(a, device="cuda") for a in arrays]


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _assert_row(got, want, what, exact_zero=()):
    bar_f, bar_v = _bars()
    got = np.asarray(got, np.float64)
    assert np.isnan(got[19]), (what, got[19])
    for k in USED:
        bar = bar_f if k >= 4 else bar_v
        print(f"{what} slot {k:2d} got {got[k]!r} want {want[k]!r} diff {abs(got[k] - want[k]):.3e} bar {bar:.3e}")
    for k in USED:
        if k in exact_zero:
            assert got[k] == 0.0, (what, k, got[k])
        else:
            assert abs(got[k] - want[k]) <= (bar_f if k >= 4 else bar_v), (what, k, got[k], want[k])


def test_bars_are_the_measured_ones():
    bar_f, bar_v = _bars()
    print(f"largest f32 - f64 difference of the restatement: factors {bar_f / HEADROOM:.3e}, values {bar_v / HEADROOM:.3e}; "
          f"bars {bar_f:.3e}, {bar_v:.3e}")
    # float32 against exact arithmetic: somewhere between one rounding and a thousand of them, far below a formula error (1e-3)
    assert 6e-8 < bar_v / HEADROOM < bar_f / HEADROOM < 6e-5


@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("W,H", SHAPES + [RAGGED_RUN])
def test_kernel_equals_the_float64_oracle(W, H, noise):
    """161 x 161: the smallest legal size, odd at every level, level 4 a single filtered pixel; 176 x 164: even down to 11 x 11;
    203 x 177: ragged, odd and even at different levels for W and H, one tile per block at every level; 640 x 480: 3 600 tiles at
    level 0, eight per block, 450 blocks on 28 ticket lines, and two per block at level 1; 500 x 340: a tile row that its blocks' runs of
    four do not divide (held to the bars of the other four shapes)."""
    import torch
    import dqo_eval
    render, gt, want, _ = _case(W, H, noise)
    assert (want[FACTORS] > 0.05).all() and (want[FACTORS] < 1).all(), want  # (no clamp hides a level)
    row = dqo_eval.ms_ssim(*_gpu(render, gt))
    torch.cuda.synchronize()
    assert row.dtype == torch.float32 and tuple(row.shape) == (20,) and row.is_cuda
    _assert_row(row.cpu().numpy(), want, f"{W}x{H} noise {noise}")


def test_identical_images_give_exactly_one():
    import dqo_eval
    a, _ = uniform_pair(203, 177, 3)
    x, y = _gpu(a, a.copy())
    got = dqo_eval.ms_ssim(x, y).cpu().numpy()
    assert (got[USED] == np.float32(1.0)).all() and np.isnan(got[19]), got
    got = dqo_eval.ms_ssim(x, x).cpu().numpy()  # ... and of one tensor with itself
    assert (got[USED] == np.float32(1.0)).all(), got


def test_a_negated_image_gives_exactly_zero():
    import dqo_eval
    a, _ = uniform_pair(203, 177, 3)
    got = dqo_eval.ms_ssim(*_gpu(a, 1.0 - a)).cpu().numpy()
    assert got[0] == 0.0 and (got[1:4] == 0.0).all() and (got[4:16] == 0.0).all(), got
    _assert_row(got, ms_ssim_row(a, 1.0 - a), "negated", exact_zero=tuple(range(16)))


def test_independent_noise_clamps_a_factor_at_zero():
    """Seed 0 at 203 x 177: the mean cs of one channel at level 0 is negative, so its factor is exactly 0 and so is that channel's value;
    every other mean is more than 1e-4 from zero, so no sign hangs on a rounding."""
    import dqo_eval
    a, b = uniform_pair(203, 177, 0)
    want, means = ms_ssim_row(a, b, with_means=True)
    zero = [k for k in FACTORS if want[k] == 0.0]
    assert zero and (np.abs(means) > 1e-4).all(), (want, means)
    got = dqo_eval.ms_ssim(*_gpu(a, b)).cpu().numpy()
    _assert_row(got, want, "uniform", exact_zero=tuple(zero) + tuple(k for k in VALUES[1:] if want[k] == 0.0))


def test_repeats_bitwise_a_table_row_is_the_single_row_and_a_second_size_is_right():
    import torch
    import dqo_eval
    render, gt, want, _ = _case(203, 177, 0.1)
    x, y = _gpu(render, gt)
    a = dqo_eval.ms_ssim(x, y)
    b = dqo_eval.ms_ssim(x, y)
    sentinel = 0x7FC0ABCD  # (a NaN with a payload: only a bit comparison sees it)
    table = torch.full((4, 20), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    r = dqo_eval.ms_ssim(x, y, out=table, row=2)
    torch.cuda.synchronize()
    assert r.data_ptr() == table[2].data_ptr()
    assert _bits(a).tobytes() == _bits(b).tobytes() and len(_bits(a).tobytes()) == 80
    t = _bits(table)
    assert t[2].tobytes() == _bits(a).tobytes()
    assert (t[[0, 1, 3]] == sentinel).all()
    # another size on the same device afterwards: the workspaces were handed back clean
    render2, gt2, want2, _ = _case(176, 164, 0.02)
    _assert_row(dqo_eval.ms_ssim(*_gpu(render2, gt2)).cpu().numpy(), want2, "second size")
    _assert_row(dqo_eval.ms_ssim(x, y).cpu().numpy(), want, "first size again")
    # ... and ONE caller's buffer serves both sizes in turn: the ticket words come back at zero from every call
    ws = dqo_eval.ms_ssim_workspace(203, 177, "cuda")
    assert ws.numel() >= dqo_eval.ms_ssim_workspace(176, 164, "cuda").numel()
    _assert_row(dqo_eval.ms_ssim(x, y, workspace_buffer=ws).cpu().numpy(), want, "shared buffer, first size")
    _assert_row(dqo_eval.ms_ssim(*_gpu(render2, gt2), workspace_buffer=ws).cpu().numpy(), want2, "shared buffer, second size")
    assert _bits(dqo_eval.ms_ssim(x, y, workspace_buffer=ws)).tobytes() == _bits(a).tobytes()


def test_an_overflowed_render_gives_a_row_of_nan():
    import torch
    import dqo_eval
    render, gt, want, _ = _case(176, 164, 0.1)
    x, y = _gpu(render, gt)
    header = torch.zeros((8,), dtype=torch.int32, device="cuda")  # DqoRastHeader: word 2 = overflow
    header[2] = 1
    got = dqo_eval.ms_ssim(x, y, render_header=header.view(torch.uint8)).cpu().numpy()
    assert np.isnan(got).all(), got
    header[2] = 0
    _assert_row(dqo_eval.ms_ssim(x, y, render_header=header.view(torch.uint8)).cpu().numpy(), want, "clean header")


def test_capturable_in_a_graph_and_replays_on_changed_inputs():
    import torch
    import dqo_eval
    frames = [structured(203, 177, s, 0.05) for s in (21, 22, 23)]
    eager = [_bits(dqo_eval.ms_ssim(*_gpu(*f))) for f in frames]
    x, y = _gpu(*frames[0])
    table = torch.zeros((1, 20), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (the module's workspace for this size exists: nothing is allocated while capturing)
        dqo_eval.ms_ssim(x, y, out=table, row=0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dqo_eval.ms_ssim(x, y, out=table, row=0)
    for k in (1, 2):
        nx, ny = _gpu(*frames[k])
        x.copy_(nx), y.copy_(ny)
        g.replay()
        torch.cuda.synchronize()
        assert _bits(table)[0].tobytes() == eager[k].tobytes(), k
    assert eager[1].tobytes() != eager[2].tobytes()


def _mapper_scene(W, H):
    """A 4 k Gaussian frustum cloud seen from two cameras; every camera's target is the render of a perturbed copy."""
    import torch
    from dqo_harness import mapping, scenes
    dev = torch.device("cuda")
    f = 0.82 * W
    cams = [scenes.Camera(W, H, f, f, (W - 1) / 2, (H - 1) / 2, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]))]
    scene = scenes.frustum_cloud(17, 4000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    targets = [mapping.perturbed_target(scene, st, dev, 40 + k) for k, st in enumerate(settings)]
    return dev, scene, settings, targets


def test_evaluate_fills_the_ms_ssim_table_from_the_same_render():
    import torch
    import dqo_eval
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _mapper_scene(176, 164)
    fm = FusedMapper(scene, settings[0], dev)
    frames = [(None if k == 0 else st, t["gt_color"], t["gt_depth"]) for k, (st, t) in enumerate(zip(settings, targets))]
    plain = _bits(fm.evaluate(frames, min_depth=0.3, max_depth=5.0))
    sentinel = 0x7FC0ABCD
    table20 = torch.full((2, 20), sentinel, dtype=torch.int32, device=dev).view(torch.float32)
    table = fm.evaluate_ms_ssim(frames, table20, min_depth=0.3, max_depth=5.0)
    torch.cuda.synchronize()
    assert _bits(table).tobytes() == plain.tobytes()  # the [K,8] table does not know about the other one
    # after the first call nothing is allocated and nothing is read
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fm.evaluate_ms_ssim(frames, table20, min_depth=0.3, max_depth=5.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    opacity, scales, rotations = fm.activate()
    for k, (st, t) in enumerate(zip(settings, targets)):
        ref = mapping.render(st, dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs))
        want = dqo_eval.ms_ssim(ref["render"], t["gt_color"])
        got = table20[k].cpu().numpy()
        assert _bits(table20[k]).tobytes() == _bits(want).tobytes(), (k, got, want.cpu().numpy())
        assert np.isfinite(got[USED]).all() and 0 < got[0] < 1 and np.isnan(got[19]), (k, got)
        d = dqo_eval.eval_picture_dict(table[k], ms_row=table20[k])
        assert d["ssim"] == float(got[0]) and d["ssim_single_scale"] == float(table[k, 4]) and d["psnr"] == float(table[k, 0])
        assert "ssim_single_scale" not in dqo_eval.eval_picture_dict(table[k])


def test_a_small_mapper_refuses_ms_ssim():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _mapper_scene(176, 160)
    fm = FusedMapper(scene, settings[0], dev)
    frames = [(None, targets[0]["gt_color"], targets[0]["gt_depth"])]
    with pytest.raises(RuntimeError, match="160"):
        fm.evaluate_ms_ssim(frames, torch.zeros((1, 20), dtype=torch.float32, device=dev))


def test_refusals_come_before_any_launch():
    import torch
    import dqo_eval
    ok = torch.zeros((3, 200, 300), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.ms_ssim(torch.zeros((3, 200, 300)), torch.zeros((3, 200, 300)))
    small = torch.zeros((3, 160, 300), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="160"):
        dqo_eval.ms_ssim(small, small)
    with pytest.raises(RuntimeError, match=r"\[K,20\]"):
        dqo_eval.ms_ssim(ok, ok, out=torch.zeros((4, 40), dtype=torch.float32, device="cuda")[:, ::2], row=0)
    with pytest.raises(RuntimeError, match=r"\[K,20\]"):
        dqo_eval.ms_ssim(ok, ok, out=torch.zeros((4, 8), dtype=torch.float32, device="cuda"), row=0)
    with pytest.raises(RuntimeError, match=r"\[3,200,300\]"):
        dqo_eval.ms_ssim(ok, torch.zeros((3, 200, 299), dtype=torch.float32, device="cuda"))
