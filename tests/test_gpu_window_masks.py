"""GPU: dqo_window_masks (csrc/map_tilemask.hip) — Mapping.evaluate_render_range for one frame of the window, in place — against its
numpy restatement (tests/window_mask_oracle.py) BIT FOR BIT, the reference's recorded results (tests/golden/tilemask_golden.npz), and
FusedMapper.refresh_window against the same call on the drop-in operator's render.

Nothing here has a tolerance of its own: masks, tile masks and the ratio's float32 bits are integers or a float32 division of two
integers, and the tile sums are float32 additions in an order the oracle restates.  A workspace is made once per image size for the
whole module and never zeroed again: every call must hand it back ready."""
import ctypes
import functools

import numpy as np
import pytest

import window_mask_oracle as wo
from test_oracle_tilemask import topk_mask_agrees
from test_window_mask_oracle import assert_goldens

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


@functools.lru_cache(maxsize=None)
def _workspace(H, W):
    import dqo_tilemask
    return dqo_tilemask.window_masks_workspace(H, W, "cuda")


def _inputs(W, H, seed):
    """Seeded frame: T_map exactly 1.0 on about half the pixels; a render with pixels whose three channels are exactly 0; a target."""
    rng = np.random.default_rng(seed)
    T = np.where(rng.uniform(size=(H, W)) < 0.5, np.float32(1), rng.uniform(0, 1, (H, W)).astype(np.float32))
    render = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    render[:, rng.uniform(size=(H, W)) < 0.2] = 0
    gt = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    return T, render, gt


def _sums_case(W, H, sums):
    """A frame whose tile sums are exactly `sums` ([gy, gx] float32): the whole error of a tile sits in its first pixel, channel 0."""
    render, gt = np.full((3, H, W), 0.5, np.float32), np.full((3, H, W), 0.5, np.float32)
    render[0, ::16, ::16], gt[0, ::16, ::16] = sums, 0
    return np.ones((H, W), np.float32), render, gt


def _call(T, render, gt, mode, ratio=0.5, k=0, header=None, fill=None):
    """dqo_window_masks through the C ABI on fresh outputs (filled with `fill`) and the module's workspace of that size."""
    import torch
    import _dqo_native as N
    H, W = T.shape
    gy, gx = wo.grid(H, W)
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")
    tT, tr, tg = t(T), t(render), t(gt)
    mask = torch.full((H, W), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
    tile = torch.full((gy, gx), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    out = torch.zeros((1,), dtype=torch.float32, device="cuda")
    ws = _workspace(H, W)
    N.check(N.lib().dqo_window_masks(W, H, mode, N.ptr(tT), N.ptr(tr), N.ptr(tg), float(ratio), int(k), N.ptr(mask), N.ptr(tile), N.ptr(out),
                                     N.ptr(header), N.ptr(ws), ws.numel(), N.current_stream()))
    torch.cuda.synchronize()
    import dqo_tilemask
    sums = dqo_tilemask.window_masks_tile_sums(ws, H, W).cpu().numpy().copy() if mode == wo.MODE_ERROR else None
    return dict(render_mask=mask.cpu().numpy(), tile_mask=tile.cpu().numpy(), ratio=out.cpu().numpy()[0], sums=sums)


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got["tile_mask"], want["tile_mask"], err_msg=f"{what} tile mask")
    np.testing.assert_array_equal(got["render_mask"], want["render_mask"], err_msg=f"{what} render mask")
    g, w = np.float32(got["ratio"]).view(np.uint32), np.float32(want["ratio"]).view(np.uint32)
    print(f"{what}: ratio {got['ratio']!r} want {want['ratio']!r}, tiles set {int(got['tile_mask'].sum())}")
    assert g == w, (what, got["ratio"], want["ratio"])
    if want["sums"] is not None:
        gs, wsum = got["sums"].view(np.uint32), want["sums"].view(np.uint32)
        both_nan = np.isnan(got["sums"]) & np.isnan(want["sums"])
        assert ((gs == wsum) | both_nan).all(), (what, "tile sums", int(((gs != wsum) & ~both_nan).sum()))


@pytest.mark.parametrize("W,H", [(1, 1), (17, 5), (64, 48), (203, 131), (640, 480), (1200, 680)])
def test_kernel_equals_the_oracle_bit_for_bit(W, H):
    """One pixel; one ragged tile; twelve full tiles; ragged in both directions (117 tiles: one ticket line, the select's last chunk
    partial); 640 x 480: 1200 tiles — more than the last block has threads, 75 ticket lines wanted of the 64 there are; 1200 x 680: 3225
    tiles and half a tile row at the bottom."""
    T, render, gt = _inputs(W, H, 3000 + W)
    gy, gx = wo.grid(H, W)
    for ratio in (0.5, 0.25):
        _assert_same(_call(T, None, None, wo.MODE_LOCAL, ratio), wo.window_masks(T, mode=wo.MODE_LOCAL, tile_mask_ratio=ratio), f"{W}x{H} local {ratio}")
    _assert_same(_call(T, None, None, wo.MODE_FINAL), wo.window_masks(T, mode=wo.MODE_FINAL), f"{W}x{H} final")
    for sample_ratio in (0.4, 0.1):
        k = wo.top_k(H, W, sample_ratio)
        got, want = _call(T, render, gt, wo.MODE_ERROR, k=k), wo.window_masks(None, render, gt, wo.MODE_ERROR, k=k)
        _assert_same(got, want, f"{W}x{H} error k={k}")
        assert got["tile_mask"].sum() == k
        if len(np.unique(got["sums"])) == gy * gx and k > 0:  # away from ties: the set torch.topk picks on the read-back sums
            import torch
            idx = torch.topk(torch.tensor(got["sums"].reshape(-1), device="cuda"), k).indices.cpu().numpy()
            assert set(idx.tolist()) == set(np.nonzero(got["tile_mask"].reshape(-1))[0].tolist())
    if W * H > 1:
        assert 0 < wo.window_masks(T, mode=wo.MODE_LOCAL)["ratio"] < 1


@pytest.mark.parametrize("W,H", [(203, 131), (640, 480)])
@pytest.mark.parametrize("case", ["k_zero", "k_all", "identical", "low_digits", "plateau", "nan_pixel"])
def test_selection_cases(W, H, case):
    rng = np.random.default_rng(len(case) * 1000 + W)
    gy, gx = wo.grid(H, W)
    n = gy * gx
    T, render, gt = _inputs(W, H, 4000 + W)
    k = n // 3
    if case == "k_zero":
        k = 0
    elif case == "k_all":
        k = n
    elif case == "identical":  # every sum is 0: the first k tile indices
        gt = render.copy()
    elif case == "low_digits":  # sums in [1, 1 + 2^-12): the two top key bytes tie everywhere, the low digits decide
        sums = (np.float32(1) + rng.integers(0, 2048, (gy, gx)).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
        T, render, gt = _sums_case(W, H, sums)
    elif case == "plateau":  # equal sums that straddle the k-th place: 300 of them (half the tiles where there are fewer than 600)
        sums = rng.uniform(0.5, 4, n).astype(np.float32)
        flat = min(300, n // 2)
        level = np.float32(np.sort(sums)[n // 2])
        sums[rng.permutation(n)[:flat]] = level
        k = int((sums > level).sum()) + flat // 2
        T, render, gt = _sums_case(W, H, sums.reshape(gy, gx))
    elif case == "nan_pixel":
        k = 3
        render[:, H // 2, W // 2] = 0.5  # (not one of the zeroed pixels, whose error is 0 whatever the target)
        gt[1, H // 2, W // 2] = np.nan
    got, want = _call(T, render, gt, wo.MODE_ERROR, k=k), wo.window_masks(None, render, gt, wo.MODE_ERROR, k=k)
    _assert_same(got, want, f"{W}x{H} {case}")
    flat_mask = got["tile_mask"].reshape(-1)
    assert flat_mask.sum() == k
    if case == "identical":
        assert (got["sums"] == 0).all() and flat_mask[:k].all()
    if case == "low_digits":
        assert (got["sums"].view(np.uint32) >> 16 == 0x3F80).all() and len(np.unique(got["sums"])) > 100
    if case == "plateau":
        ties = np.nonzero(got["sums"].reshape(-1) == level)[0]
        taken = flat_mask[ties]
        assert 0 < taken.sum() < len(ties) and taken[:taken.sum()].all()  # the lowest tile indices of the plateau, and only those
    if case == "nan_pixel":
        assert np.isnan(got["sums"][(H // 2) // 16, (W // 2) // 16]) and got["tile_mask"][(H // 2) // 16, (W // 2) // 16] == 1
    if case == "k_all":
        assert got["render_mask"].all() and got["ratio"] == 1
    if case == "k_zero":
        assert not got["render_mask"].any() and got["ratio"] == 0


def test_reference_goldens_through_the_kernel():
    assert_goldens(lambda T, render, gt, mode, r, k: _call(T, render, gt, mode, r, k))


def test_python_entry_writes_the_callers_tensors_and_checks_them():
    import torch
    import dqo_tilemask as M
    W, H = 203, 131
    T, render, gt = _inputs(W, H, 11)
    tT, tr, tg = (torch.tensor(a, device="cuda") for a in (T[None], render, gt))
    gy, gx = wo.grid(H, W)
    mask, tile, ratio = (torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((gy, gx), dtype=torch.int32, device="cuda"),
                         torch.zeros((1,), dtype=torch.float32, device="cuda"))
    for kw, mode, k in ((dict(), wo.MODE_LOCAL, 0), (dict(global_opt=True), wo.MODE_FINAL, 0),
                        (dict(global_opt=True, sample_ratio=0.4), wo.MODE_ERROR, wo.top_k(H, W, 0.4))):
        a, b, c = M.window_masks(tT, tr, tg, render_mask=mask, tile_mask=tile, ratio_out=ratio, workspace=_workspace(H, W), **kw)
        assert a is mask and b is tile and c is ratio
        torch.cuda.synchronize()
        want = wo.window_masks(T, render, gt, mode, 0.5, k)
        _assert_same(dict(render_mask=mask.cpu().numpy(), tile_mask=tile.cpu().numpy(), ratio=ratio.cpu().numpy()[0], sums=None),
                     dict(want, sums=None), f"python entry mode {mode}")
    a, b, c = M.window_masks(tT)  # its own outputs and workspace
    assert a.dtype == torch.uint8 and tuple(a.shape) == (H, W) and b.dtype == torch.int32 and tuple(b.shape) == (gy, gx) and tuple(c.shape) == (1,)
    np.testing.assert_array_equal(a.cpu().numpy(), (T != 1).astype(np.uint8))
    for bad in (dict(render_mask=mask.bool()), dict(render_mask=mask[:, :-1]), dict(tile_mask=tile.float()), dict(tile_mask=tile.t()),
                dict(ratio_out=torch.zeros((2,), dtype=torch.float32, device="cuda")), dict(render_mask=mask.cpu()),
                dict(global_opt=True, sample_ratio=0.4, render=None)):
        with pytest.raises(RuntimeError):
            M.window_masks(tT, bad.pop("render", tr), tg, **bad)
    with pytest.raises(RuntimeError):
        M.window_masks(tT.cpu())


def test_argument_errors_launch_nothing():
    import torch
    import _dqo_native as N
    lib = N.lib()
    W, H = 64, 48
    gy, gx = wo.grid(H, W)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    T, render, gt, out = f(H, W), f(3, H, W), f(3, H, W), f(1)
    mask, tile = torch.full((H, W), 7, dtype=torch.uint8, device="cuda"), torch.full((gy, gx), 7, dtype=torch.int32, device="cuda")
    ws = _workspace(H, W)
    p, s = N.ptr, N.current_stream()
    assert lib.dqo_window_masks_workspace_bytes(W, H) == ws.numel() and lib.dqo_window_masks_workspace_bytes(0, 5) == 0
    bad = [(W, H, 0, p(T), None, None, 0.5, 0, None, p(tile), p(out), None, p(ws), ws.numel(), s),          # a NULL output
           (W, H, 0, p(T), None, None, 0.5, 0, p(mask), None, p(out), None, p(ws), ws.numel(), s),
           (W, H, 0, p(T), None, None, 0.5, 0, p(mask), p(tile), None, None, p(ws), ws.numel(), s),
           (W, H, 1, p(T), None, p(gt), 0.5, 1, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s),      # error mode without render / gt
           (W, H, 1, p(T), p(render), None, 0.5, 1, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s),
           (W, H, 1, p(T), p(render), p(gt), 0.5, -1, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s),  # k outside [0, gy * gx]
           (W, H, 1, p(T), p(render), p(gt), 0.5, gy * gx + 1, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s),
           (W, H, 0, p(T), None, None, 0.5, 0, p(mask), p(tile), p(out), None, p(ws), ws.numel() - 1, s),    # a workspace that is too small
           (W, H, 0, p(T), None, None, 0.5, 0, p(mask), p(tile), p(out), None, None, ws.numel(), s),
           (W, H, 3, p(T), None, None, 0.5, 0, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s)]
    for args in bad:
        assert lib.dqo_window_masks(*args) == -1 and lib.dqo_last_error()  # DQO_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (mask == 7).all() and (tile == 7).all() and out[0] == 0
    assert lib.dqo_window_masks(W, H, 1, None, p(render), p(gt), 0.5, gy * gx, p(mask), p(tile), p(out), None, p(ws), ws.numel(), s) == 0
    torch.cuda.synchronize()
    assert (mask == 1).all() and (tile == 1).all() and out[0] == 1


def test_repeats_bitwise_and_replays_from_a_graph_on_changed_inputs():
    """Two calls write the same bytes; the call captured in a graph and replayed after the inputs were rewritten in place gives the new
    inputs' masks — in the error mode (two kernel nodes) and the local mode (one)."""
    import torch
    import dqo_tilemask as M
    W, H = 203, 131
    gy, gx = wo.grid(H, W)
    frames = [_inputs(W, H, s) for s in (31, 32, 33)]
    dev = lambda c: tuple(torch.tensor(a, device="cuda") for a in (c[0][None], c[1], c[2]))
    ws = _workspace(H, W)
    for kw, mode, k in ((dict(global_opt=True, sample_ratio=0.4), wo.MODE_ERROR, wo.top_k(H, W, 0.4)), (dict(), wo.MODE_LOCAL, 0)):
        first = [t.clone() for t in M.window_masks(*dev(frames[0]), workspace=ws, **kw)]
        again = M.window_masks(*dev(frames[0]), workspace=ws, **kw)
        torch.cuda.synchronize()
        for a, b in zip(first, again):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        tT, tr, tg = dev(frames[0])
        mask, tile, ratio = (torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((gy, gx), dtype=torch.int32, device="cuda"),
                             torch.zeros((1,), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            M.window_masks(tT, tr, tg, render_mask=mask, tile_mask=tile, ratio_out=ratio, workspace=ws, **kw)
        seen = []
        for c in frames[1:]:
            for dst, src in zip((tT, tr, tg), dev(c)):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            got = dict(render_mask=mask.cpu().numpy(), tile_mask=tile.cpu().numpy(), ratio=ratio.cpu().numpy()[0], sums=None)
            _assert_same(got, dict(wo.window_masks(c[0], c[1], c[2], mode, 0.5, k), sums=None), f"replay mode {mode}")
            seen.append(got["tile_mask"].tobytes())
        assert seen[0] != seen[1]


def test_an_overflowed_render_keeps_the_masks_and_flags_the_ratio():
    """The header's overflow word set (a flagged state, written here by hand): every mode leaves both masks as they were and writes NaN;
    the workspace is handed back ready all the same."""
    import torch
    W, H = 203, 131
    T, render, gt = _inputs(W, H, 41)
    k = wo.top_k(H, W, 0.4)
    over = torch.tensor([5, 5, 1, 0, 0, 0, 2, 0], dtype=torch.int32, device="cuda")  # DqoRastHeader: word 2 = overflow
    fine = torch.tensor([5, 5, 0, 0, 0, 0, 2, 0], dtype=torch.int32, device="cuda")
    for mode in (wo.MODE_LOCAL, wo.MODE_ERROR, wo.MODE_FINAL):
        got = _call(T, render, gt, mode, k=k, header=over, fill=7)
        assert (got["render_mask"] == 7).all() and (got["tile_mask"] == 7).all(), mode
        assert np.isnan(got["ratio"]) and np.float32(got["ratio"]).view(np.uint32) == NAN_BITS, mode
        _assert_same(dict(_call(T, render, gt, mode, k=k, header=fine, fill=7), sums=None), dict(wo.window_masks(T, render, gt, mode, 0.5, k), sums=None),
                     f"after the flagged call, mode {mode}")


# ---- FusedMapper.refresh_window ------------------------------------------------------------------------------------------------------
def _window(torch, seed, render_masks=True, tile_masks=True):
    """The 160 x 120 scene and its three cameras (test_gpu_eval._scene) as a window's frames, with random render masks.  The tile masks are
    the frames' own all-ones tensors: a capture sizes its capacities under the tile mask it is given, and refresh_window may switch any
    tile on."""
    from test_gpu_eval import _scene
    dev, scene, settings, targets = _scene()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    frames = []
    for st, t in zip(settings, targets):
        fr = dict(gt_color=t["gt_color"].clone(), gt_depth=t["gt_depth"].clone(), settings=st)
        if render_masks:
            fr["render_mask"] = (torch.rand((120, 160), generator=gen) < 0.6).to(dev)
        if tile_masks:
            fr["tile_mask"] = torch.ones((8, 10), dtype=torch.int32, device=dev)
        frames.append(fr)
    return dev, scene, settings, frames


def _bytes(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize("mode", ["local", "error"])
def test_refresh_window_equals_window_masks_of_the_ops_render_and_then_reads_nothing(mode):
    import torch
    import _dqo_native as N
    import dqo_tilemask as M
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, frames = _window(torch, 5)
    kw = dict(global_opt=True, sample_ratio=0.4) if mode == "error" else dict()
    fm = FusedMapper(scene, settings[0], dev)
    fm.capture_window(frames, loss_tap=True, fused_tail=True, capacity_margin=2.0)
    fm._graph_of((0, 2))  # a mixed graph captured BEFORE the refresh: frame 0's camera under frame 2's masks, in buffers of its own
    assert fm._mixed[(0, 2)].mask.data_ptr() != fm._frames[2].mask.data_ptr()
    rows = (torch.rand((fm.P,), generator=torch.Generator(device="cpu").manual_seed(9)) < 0.5).to(dev) if mode == "local" else None
    before_masks = [_bytes(g.mask) for g in fm._frames]
    lib = N.lib()
    calls, real = [], lib.dqo_rast_read_header

    def counted(*a):
        calls.append(1)
        return real(*a)

    lib.dqo_rast_read_header = counted
    try:
        ratios = fm.refresh_window(rows=rows, **kw)
        torch.cuda.synchronize()
        assert len(calls) == 1 and not fm.maintain_overflowed()  # (one header read sized the context)
        first = [(_bytes(g.mask), _bytes(g.tile_mask)) for g in fm._frames] + [_bytes(ratios)]
        before, n_calls = torch.cuda.memory_allocated(), len(calls)
        torch.cuda.set_sync_debug_mode("error")
        try:
            ratios2 = fm.refresh_window(rows=rows, **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.cuda.memory_allocated() == before and len(calls) == n_calls
    finally:
        lib.dqo_rast_read_header = real
    torch.cuda.synchronize()
    assert ratios2 is ratios and tuple(ratios.shape) == (3,) and ratios.dtype == torch.float32
    assert [(_bytes(g.mask), _bytes(g.tile_mask)) for g in fm._frames] + [_bytes(ratios2)] == first
    assert all(_bytes(g.mask) != b for g, b in zip(fm._frames, before_masks))
    assert torch.equal(fm.tile_mask, torch.ones_like(fm.tile_mask))
    # against the drop-in operator's render of the same rows at each camera
    opacity, scales, rotations = fm.activate()
    sel = fm.trained_rows() if rows is None else rows
    cloud = dict(xyz=fm.xyz[sel], opacity=opacity[sel], scales=scales[sel], rotations=rotations[sel], shs=fm.shs[sel])
    for k, (st, fr) in enumerate(zip(settings, frames)):
        g = fm._frames[k]
        ref = mapping.render(st, cloud)
        want = M.window_masks(ref["T_map"].contiguous(), ref["render"].contiguous(), fr["gt_color"], **kw)
        torch.cuda.synchronize()
        assert _bytes(g.mask) == _bytes(want[0]) and _bytes(g.tile_mask) == _bytes(want[1]) and _bytes(ratios[k:k + 1]) == _bytes(want[2]), k
        rm, tm, rr = M.evaluate_render_range(ref["T_map"], ref["render"], fr["gt_color"], **kw)  # the parent's chain, away from ties
        if mode == "local":
            assert torch.equal(rm, g.mask.bool()) and torch.equal(tm, g.tile_mask)
        else:
            pooled = M.color_error_tiles(ref["render"], fr["gt_color"])[1].cpu().numpy()
            assert topk_mask_agrees(g.tile_mask.cpu().numpy(), tm.cpu().numpy(), pooled, wo.top_k(120, 160, 0.4))
        assert abs(float(rr) - float(ratios[k])) < 1e-6 and 0 < float(ratios[k]) <= 1
    # the mixed graph captured before the refresh sees frame 2's new masks
    mixed = fm._mixed[(0, 2)]
    assert _bytes(mixed.mask) == _bytes(fm._frames[2].mask) and _bytes(mixed.tile_mask) == _bytes(fm._frames[2].tile_mask)
    # the replays train under the new masks: the losses of a mapper whose window was captured with them from the start
    twin = FusedMapper(scene, settings[0], dev)
    twin.capture_window([dict(fr, render_mask=g.mask.clone().bool(), tile_mask=g.tile_mask.clone()) for fr, g in zip(frames, fm._frames)],
                        loss_tap=True, fused_tail=True, capacity_margin=2.0)
    for k in (0, 1, 2, (0, 2)):
        fm.replay(frame=k), twin.replay(frame=k)
        torch.cuda.synchronize()
        assert not fm.graph_overflowed() and not twin.graph_overflowed(), k
        assert torch.equal(fm.loss, twin.loss) and float(fm.loss[0]) > 0, k
    for name in fm._params():
        assert torch.equal(fm._params()[name], twin._params()[name]), name


def test_refresh_window_takes_slots_and_a_callers_table():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, frames = _window(torch, 6)
    fm = FusedMapper(scene, settings[0], dev)
    fm.capture_window(frames, loss_tap=True, fused_tail=True, capacity_margin=2.0)
    allr = fm.refresh_window().clone()
    old = _bytes(fm._frames[0].mask)
    fm._frames[0].mask.zero_()
    mine = torch.zeros((2,), dtype=torch.float32, device=dev)
    assert fm.refresh_window(frames=[2, 1], out=mine) is mine
    torch.cuda.synchronize()
    assert _bytes(mine) == _bytes(allr[[2, 1]]) and not fm._frames[0].mask.any()  # (slot 0 was not asked for)
    fm.refresh_window(frames=[0])
    torch.cuda.synchronize()
    assert _bytes(fm._frames[0].mask) == old


def test_refresh_window_refusals():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, frames = _window(torch, 7)
    with pytest.raises(NotImplementedError):
        FusedMapper(scene, settings[0], dev, attach_count_reducer=lambda n: n).refresh_window()
    fm = FusedMapper(scene, settings[0], dev)
    no_mask = {k: v for k, v in frames[0].items() if k != "render_mask"}
    shared_tiles = {k: v for k, v in frames[1].items() if k != "tile_mask"}
    fm.capture_window([no_mask, shared_tiles, frames[2]], loss_tap=True, fused_tail=True)
    kept = [(_bytes(g.mask) if g.mask is not None else None, _bytes(g.tile_mask)) for g in fm._frames]
    with pytest.raises(RuntimeError, match="without a render mask"):
        fm.refresh_window(frames=[0])
    with pytest.raises(RuntimeError, match="shared all-ones tile mask"):
        fm.refresh_window(frames=[1])
    with pytest.raises(RuntimeError, match="shared all-ones tile mask|without a render mask"):
        fm.refresh_window()  # (refused as a whole: frame 2 is not touched either)
    g = fm._frames[2]
    real = g.settings
    g.settings = real._replace(image_height=136)
    try:
        with pytest.raises(RuntimeError, match="image size"):
            fm.refresh_window(frames=[2])
    finally:
        g.settings = real
    with pytest.raises(RuntimeError, match="rows"):
        fm.refresh_window(frames=[2], rows=torch.ones((fm.P - 1,), dtype=torch.bool, device=dev))
    torch.cuda.synchronize()
    assert [(_bytes(g.mask) if g.mask is not None else None, _bytes(g.tile_mask)) for g in fm._frames] == kept
    assert torch.equal(fm.tile_mask, torch.ones_like(fm.tile_mask)) and fm._maintain_ctx is None  # nothing was rendered
    fm.refresh_window(frames=[2])
    torch.cuda.synchronize()
    assert torch.equal(fm.tile_mask, torch.ones_like(fm.tile_mask)) and _bytes(fm._frames[2].mask) != kept[2][0]
