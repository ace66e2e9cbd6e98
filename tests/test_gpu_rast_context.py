"""_dqo_context.RastContext driven by hand (measure, size, render) gives the frame the drop-in op gives in 'exact' mode, bit for bit, and
the module's header readers read what the op's own readers read."""
import numpy as np
import pytest

from dqo_harness import scenes
import util_rast as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _frame(torch, P):
    """Configuration 1 cut to its first P Gaussians: the op's frame in 'exact' mode and what a hand-driven context needs for the same."""
    import _dqo_native as N
    import diff_gaussian_rasterization_depth as dgr
    cam, sc = scenes.make_config(1, P=max(P, 1))
    dev = torch.device("cuda")
    t = lambda a: torch.tensor(np.ascontiguousarray(a[:P], np.float32), device=dev)
    xyz, shs, opacity, scales, rotations = t(sc["xyz"]), t(sc["shs"]), t(sc["opacity"]), t(sc["scales"]), t(sc["rotations"])
    rs = U.raster_settings_torch(cam, dev)
    e = torch.empty(0, device=dev)
    assert dgr._sync_mode == "exact"
    with torch.no_grad():
        ref = dgr.rasterize_gaussians(xyz, shs, e, opacity, scales, rotations, e, None, rs)
    op = dict(out=ref, num_rendered=dgr.last_num_rendered(), num_visible=dgr._last["num_visible"], header=dgr.last_header())
    params = dgr._params(rs, P, shs.shape[1] if P else 0)
    inputs = dgr._inputs(rs, xyz, shs, e, opacity, scales, rotations, e, None)
    keep = (xyz, shs, opacity, scales, rotations, rs)  # (the structs hold raw pointers)
    return cam, op, params, inputs, N.current_stream(), keep


@pytest.mark.parametrize("P", [2000, 0])
def test_a_context_driven_by_hand_renders_the_ops_frame(torch_cuda, P):
    import _dqo_context as C
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, op, params, inputs, stream, keep = _frame(torch, P)
    dev = torch.device("cuda")
    out, outputs = dgr._new_outputs(P, cam.H, cam.W, dev)
    ctx = C.RastContext(P, cam.W, cam.H, dev)
    assert ctx.binning is None and (ctx.P, ctx.W, ctx.H) == (P, cam.W, cam.H) and ctx.geom.numel() >= 32
    hdr = ctx.measure(params, inputs, outputs, stream)
    assert int(hdr.num_candidates) == op["num_rendered"] and int(hdr.num_visible) == op["num_visible"]
    ctx.size(max(int(hdr.num_candidates), 1))
    assert ctx.cap == max(op["num_rendered"], 1) and ctx.bucket == 0 and ctx.binning is not None
    ctx.render(params, inputs, outputs, stream)
    torch.cuda.synchronize()
    assert len(out) == len(op["out"]) == 9
    for name, a, b in zip(U.HipRun.names, out, op["out"]):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert C.read_header(ctx.geom) == op["header"] and not C.overflowed(ctx.geom)
    if P == 0:  # the geometry buffer of an empty map, a rendered background, a header with zero counts
        assert all(v == 0 for v in op["header"].values()), op["header"]
        assert float(out[0].abs().max()) == 0 and bool((out[6] == 1).all()) and bool((out[3] <= 0).all())
    else:
        assert op["header"]["num_rendered"] > 0 and op["header"]["num_candidates"] == op["num_rendered"]
        assert bool((out[3] >= 0).any())  # (the frame is not empty: Gaussians were hit)


def test_a_context_that_is_too_small_flags_the_frame_and_renders_background(torch_cuda):
    """64 instance slots for a frame of thousands of pairs: the overflow flag does its job (the lists are emptied, nothing is written out
    of bounds), as the op's carried capacity of 64 in test_gpu_rast_edge.py and the outgrown pooled context in test_gpu_context_pool.py."""
    import _dqo_context as C
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, op, params, inputs, stream, keep = _frame(torch, 2000)
    assert op["num_rendered"] > 64
    dev = torch.device("cuda")
    out, outputs = dgr._new_outputs(2000, cam.H, cam.W, dev)
    ctx = C.RastContext(2000, cam.W, cam.H, dev)
    ctx.measure(params, inputs, outputs, stream)
    ctx.size(64)
    ctx.render(params, inputs, outputs, stream)
    torch.cuda.synchronize()
    assert C.overflowed(ctx.geom) and C.read_header(ctx.geom)["overflow"] != 0
    assert bool((out[3] <= 0).all()) and bool((out[6] == 1).all())  # hit_depth, T
