"""GPU: keyframe evaluation (dqo_eval.eval_picture, FusedMapper.evaluate — csrc/map_eval.hip) against the float64 oracle
(tests/eval_oracle.py) and the reference's recorded results (tests/golden/eval_golden.npz).

Bars of the kernel against the oracle, and why: every term is exact in double on both sides, the order of the additions costs at most
H W 2^-53, what remains is one division, a sqrt / log10 and the rounding to float32 (2^-24 ~ 6e-8).  2e-6 relative (psnr also within
2e-5 dB) is about 30 x that.  valid_pixel_ratio is a float32 division of two integers: exact."""
import ctypes
import functools
import os

import numpy as np
import pytest

from eval_oracle import INPUTS, ROW, eval_oracle
from test_eval_oracle import assert_row, load_fixture

pytestmark = pytest.mark.gpu

REL_BAR, PSNR_BAR_DB = 2e-6, 2e-5
KERNEL_SLOTS = (0, 1, 2, 3, 5, 6, 7)


def _inputs(W, H, seed):
    """Seeded random frame: colours in [0, 1); a target depth in [0, 6) with holes, so that both ends of (0.3, 5) are crossed; a render
    depth around it; a hit index with -1 on a tenth of the pixels."""
    rng = np.random.default_rng(seed)
    gd = rng.uniform(0, 6, (1, H, W))
    gd[rng.uniform(size=gd.shape) < 0.05] = 0.0
    idx = rng.integers(0, 100000, (1, H, W))
    idx[rng.uniform(size=idx.shape) < 0.1] = -1
    return dict(render=rng.uniform(0, 1, (3, H, W)).astype(np.float32), gt_color=rng.uniform(0, 1, (3, H, W)).astype(np.float32),
                depth=(gd + rng.normal(0, 0.05, gd.shape)).astype(np.float32), gt_depth=gd.astype(np.float32), depth_index=idx.astype(np.int32))


def _gpu(c):
    import torch
    t = {k: torch.tensor(c[k], device="cuda") for k in INPUTS}
    return dict(render=t["render"], depth=t["depth"], depth_index_map=t["depth_index"]), t["gt_color"], t["gt_depth"]


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _assert_kernel_row(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for k in KERNEL_SLOTS:
        g, w = got[k], want[k]
        print(f"{what} {ROW[k]:18s} got {g!r} want {w!r}")
        if not np.isfinite(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, ROW[k], g, w)
        elif k == 3:
            assert np.float32(g) == np.float32(w), (what, ROW[k], g, w)
        else:
            assert abs(g - w) <= REL_BAR * abs(w), (what, ROW[k], g, w)
            if k == 0:
                assert abs(g - w) <= PSNR_BAR_DB, (what, ROW[k], g, w)


@pytest.mark.parametrize("W,H", [(1, 1), (17, 5), (64, 48), (203, 131), (640, 480)])
def test_kernel_equals_the_float64_oracle(W, H):
    """One pixel; less than one wave; three full blocks of 1 024 pixels; ragged in both directions over 26 blocks (one ticket line, a
    partial last block); and 640 x 480: 300 blocks on 18 ticket lines — more blocks than the 64 first-level lines there can be."""
    import torch
    import _dqo_native as N
    import dqo_eval
    if (W, H) == (640, 480):  # a block's partial is one 64-byte line of the workspace behind its head
        lib = N.lib()
        assert (lib.dqo_eval_picture_workspace_bytes(W, H) - lib.dqo_eval_picture_workspace_bytes(1, 1)) // 64 + 1 > 64
    c = _inputs(W, H, 1000 + W)
    want = eval_oracle(*(c[n] for n in INPUTS), 0.3, 5.0, with_ssim=False)
    row = dqo_eval.eval_picture(*_gpu(c), 0.3, 5.0, ssim=False)
    torch.cuda.synchronize()
    assert row.dtype == torch.float32 and tuple(row.shape) == (8,) and row.is_cuda
    got = row.cpu().numpy()
    assert np.isnan(got[4])  # (a new row, ssim=False: the slot is nobody's)
    _assert_kernel_row(got, want, f"{W}x{H}")
    if W * H > 1:
        assert np.isfinite(want[list(KERNEL_SLOTS)]).all() and 0 < want[3] < 1


@pytest.mark.parametrize("k", range(5), ids=["generic", "identical", "no_valid_pixel", "all_out_of_range", "half_without_hit"])
def test_fixture_cases_through_the_kernel(k):
    """The reference's recorded results (torch float32), the CPU test's bars: 1e-4 absolute on psnr, the two losses and ssim."""
    import torch
    import dqo_eval
    cases, want = load_fixture()
    name, c, lo, hi = cases[k]
    row = dqo_eval.eval_picture(*_gpu(c), lo, hi)
    d = dqo_eval.eval_picture_dict(row)
    got = row.cpu().numpy()
    assert_row(got, want[k], name)
    _assert_kernel_row(got, eval_oracle(*(c[n] for n in INPUTS), lo, hi, with_ssim=False), name)
    assert d["normal_loss"] == 0 and "lpips" not in d
    for key, slot in (("psnr", 0), ("color_loss", 1), ("depth_loss", 2), ("valid_pixel_ratio", 3), ("ssim", 4)):
        assert d[key] == got[slot] or (np.isnan(d[key]) and np.isnan(got[slot])), key


def test_repeats_bitwise_and_a_table_row_is_the_single_row():
    import torch
    import dqo_eval
    c = _inputs(203, 131, 7)
    args = _gpu(c)
    a = dqo_eval.eval_picture(*args, 0.3, 5.0)
    b = dqo_eval.eval_picture(*args, 0.3, 5.0)
    sentinel = 0x7FC0ABCD  # (a NaN with a payload: only a bit comparison sees it)
    table = torch.full((4, 8), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    r = dqo_eval.eval_picture(*args, 0.3, 5.0, out=table, row=2)
    torch.cuda.synchronize()
    assert r.data_ptr() == table[2].data_ptr()
    assert _bits(a).tobytes() == _bits(b).tobytes() and len(_bits(a).tobytes()) == 32
    t = _bits(table)
    assert t[2].tobytes() == _bits(a).tobytes()
    assert (t[[0, 1, 3]] == sentinel).all()
    # ssim=False leaves slot 4 of a caller's row alone
    table2 = torch.full((1, 8), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    dqo_eval.eval_picture(*args, 0.3, 5.0, out=table2, row=0, ssim=False)
    t2 = _bits(table2)[0]
    assert t2[4] == sentinel and (np.delete(t2, 4) == np.delete(_bits(a), 4)).all()


def test_capturable_in_a_graph_and_replays_on_changed_inputs():
    """Captured on the default queue setting; replayed twice after the inputs were rewritten in place: the eager call's bits."""
    import torch
    import dqo_eval
    frames = [_inputs(203, 131, s) for s in (21, 22, 23)]
    out, gt_c, gt_d = _gpu(frames[0])
    eager = []
    for c in frames:  # (the first call also makes the module's workspace for this size: nothing is allocated while capturing)
        eager.append(_bits(dqo_eval.eval_picture(*_gpu(c), 0.3, 5.0)))
    table = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dqo_eval.eval_picture(out, gt_c, gt_d, 0.3, 5.0, out=table, row=0)
    for k in (1, 2):
        new_out, new_c, new_d = _gpu(frames[k])
        for name in out:
            out[name].copy_(new_out[name])
        gt_c.copy_(new_c), gt_d.copy_(new_d)
        g.replay()
        torch.cuda.synchronize()
        assert _bits(table)[0].tobytes() == eager[k].tobytes(), k
    assert eager[1].tobytes() != eager[2].tobytes()


@functools.lru_cache(maxsize=1)
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


def test_evaluate_equals_eval_picture_of_the_ops_render_and_then_reads_nothing():
    import torch
    import _dqo_native as N
    import dqo_eval
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _scene()
    fm = FusedMapper(scene, settings[0], dev)
    frames = [(None if k == 0 else st, t["gt_color"], t["gt_depth"]) for k, (st, t) in enumerate(zip(settings, targets))]
    lib = N.lib()
    calls, real = [], lib.dqo_rast_read_header

    def counted(*a):
        calls.append(1)
        return real(*a)

    lib.dqo_rast_read_header = counted
    try:
        first = _bits(fm.evaluate(frames, min_depth=0.3, max_depth=5.0))
        torch.cuda.synchronize()
        assert len(calls) == 1 and not fm.maintain_overflowed()  # (one header read sized the context)
        before, n_calls = torch.cuda.memory_allocated(), len(calls)
        torch.cuda.set_sync_debug_mode("error")
        try:
            table = fm.evaluate(frames, min_depth=0.3, max_depth=5.0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.cuda.memory_allocated() == before and len(calls) == n_calls
    finally:
        lib.dqo_rast_read_header = real
    torch.cuda.synchronize()
    assert tuple(table.shape) == (3, 8) and table.dtype == torch.float32 and _bits(table).tobytes() == first.tobytes()
    opacity, scales, rotations = fm.activate()
    W, H = 160, 120
    ws = torch.empty((lib.dqo_map_ssim_workspace_bytes(W, H),), dtype=torch.uint8, device=dev)
    for k, (st, t) in enumerate(zip(settings, targets)):
        ref = mapping.render(st, dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs))
        want = _bits(dqo_eval.eval_picture(ref, t["gt_color"], t["gt_depth"], 0.3, 5.0, ssim=False))
        ssim = torch.zeros((2,), dtype=torch.float32, device=dev)
        N.check(lib.dqo_map_ssim_fwd_bwd(W, H, N.ptr(ref["render"]), N.ptr(t["gt_color"]), 0.0, N.ptr(ssim), None, 0, None, N.ptr(ws), ws.numel(),
                                         N.current_stream()))
        torch.cuda.synchronize()
        got = _bits(table[k])
        for s in KERNEL_SLOTS:
            assert got[s] == want[s], (k, ROW[s])
        assert got[4] == _bits(ssim)[0], k
        v = table[k].cpu().numpy()
        assert np.isfinite(v).all() and 0 < v[3] <= 1 and 0 < v[4] < 1 and 5 < v[0] < 60, (k, v)
    # a caller's table
    mine = torch.zeros((3, 8), dtype=torch.float32, device=dev)
    assert fm.evaluate(frames, min_depth=0.3, max_depth=5.0, out=mine) is mine
    torch.cuda.synchronize()
    assert _bits(mine).tobytes() == first.tobytes()


def test_evaluate_tells_progress():
    """The target is the render of a perturbed copy of the map: thirty iterations towards it must show — no threshold."""
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _scene()
    t = targets[0]
    fm = FusedMapper(scene, settings[0], dev)
    frames = [(None, t["gt_color"], t["gt_depth"])]
    before = fm.evaluate(frames, min_depth=0.3, max_depth=5.0).clone()
    fm.capture(t["gt_color"], t["gt_depth"], t["pix_obj"] >= 0)
    fm.run(30)
    after = fm.evaluate(frames, min_depth=0.3, max_depth=5.0).clone()
    torch.cuda.synchronize()
    b, a = before[0].cpu().numpy(), after[0].cpu().numpy()
    print("before", dict(zip(ROW, b.tolist())), "after", dict(zip(ROW, a.tolist())))
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a[0] > b[0] and a[1] < b[1]


def test_a_sharded_mapper_refuses():
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, targets = _scene()
    fm = FusedMapper(scene, settings[0], dev, attach_count_reducer=lambda n: n)
    with pytest.raises(NotImplementedError, match="sharded"):
        fm.evaluate([(None, targets[0]["gt_color"], targets[0]["gt_depth"])])
