"""GPU parity at BASELINE.json's full size (config 3: 500 000 Gaussians, 1200x680) and size-independent properties of the
operator at that size: the HIP path through the drop-in Python surface (C ABI) against the CPU oracle and against itself."""
import numpy as np
import pytest

from dqo_harness import scenes
import util_rast as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()  # fails loudly if the HIP extension is missing
    return torch


@pytest.fixture(scope="module")
def cfg3():
    cam, sc = scenes.make_config(3)
    rng = np.random.default_rng(11)
    dL = (rng.normal(size=(3, cam.H, cam.W)).astype(np.float32), rng.normal(size=(1, cam.H, cam.W)).astype(np.float32))
    return cam, sc, dL


def _report(name, fs, gs):
    """Per-tensor numbers of the full-size cases go to gpurun_out/parity_<name>.json (DESIGN.md §2 quotes them)."""
    import json
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"parity_{name}.json"), "w") as fh:
        json.dump({"forward": fs, "grads": gs}, fh, indent=1)
    print(name, "fwd", fs, "grads", gs)


def _full_size_case(oracle, cfg, name, fp64=True, P=None, gated=False):
    """One BASELINE configuration at its full size against the OpenMP build of the oracle (same statements as the serial one, bitwise
    equal results: tests/test_oracle_rast.py::test_openmp_build_equals_serial): forward within 1e-4, flipped pixels within the 0.1 %
    budget and masked out of the incoming gradient on BOTH sides, gradients within 1e-3 of the fp32 oracle — north_star's numbers,
    no slack term.  The fp64 oracle runs beside EVERY configuration (seconds on the GPU box's host cores): a gradient row beyond 1e-3
    must be explained by the fp32 oracle's own distance from fp64 on that row (util_rast.compare_grads); unexplained rows are not
    allowed (unexplained_cap = 0) and are named.  gated: the blend kernels' GATE instantiation (rasterize_gaussians_gated) with bench.py's own
    gate, against the gated oracle."""
    cam, sc = scenes.make_config(cfg, P=P)
    rng = np.random.default_rng(11)
    dL = (rng.normal(size=(3, cam.H, cam.W)).astype(np.float32), rng.normal(size=(1, cam.H, cam.W)).astype(np.float32))
    gate, gate_kw = None, {}
    if gated:
        go, po, _ = U.bench_gate(cfg, cam, sc)
        gate, gate_kw = (go, po), dict(gaussian_object=go, pixel_object=po)
    hr = U.HipRun(cam, sc, object_gate=gate)
    o = oracle.OracleRasterizer(np.float32, omp=True)
    st = U.oracle_settings(oracle, cam)
    fwd = lambda orc: orc.forward(st, sc["xyz"], sc["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                                  shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"], **gate_kw)
    names = ("color", "depth", "hit_color", "hit_depth", "hit_color_weight", "hit_depth_weight", "T_map", "n_touched", "radii")
    rr = fwd(o)
    r = {k: getattr(rr, k) for k in names}
    o64 = r64 = None
    if fp64:
        o64 = oracle.OracleRasterizer(np.float64, omp=True)
        rr64 = fwd(o64)
        r64 = {k: getattr(rr64, k) for k in names}
    h = hr.res
    bad = U.flipped_pixels(h, r, r64)
    fs = U.compare_forward(h, r, r64)
    np.testing.assert_array_equal(h["radii"], r["radii"])
    # n_touched counts pixels with T' > 0.5 (forward.cu:833-835): an integer behind a float threshold, so a last-ulp difference
    # of T (v_exp_f32 vs libm exp) may move single pixels across it
    dn = np.abs(h["n_touched"].astype(np.int64) - r["n_touched"])
    assert dn.max() <= 1 and (dn != 0).mean() < 1e-4, (dn.max(), (dn != 0).sum())
    keep = (~bad).astype(np.float32)
    dLm = (dL[0] * keep[None], dL[1] * keep[None])
    hg = hr.backward(dLm, retain=False)
    og = U.oracle_backward(o, dLm)
    og64 = U.oracle_backward(o64, dLm) if fp64 else None
    gs = U.compare_grads(hg, og, og64)
    fs["P"], fs["N_reference"] = int(sc["xyz"].shape[0]), int(rr.num_rendered)
    _report(name, fs, gs)


def test_cfg3_full_size_vs_oracle(torch_cuda, oracle):
    """The metric's own workload (500 000 Gaussians, 1200x680, 8 object ids); the fp64 oracle runs beside for the report."""
    _full_size_case(oracle, 3, "cfg3")


def test_cfg3_full_size_gated_vs_oracle(torch_cuda, oracle):
    """The instantiation bench.py times — blend_forward_kernel<true> / blend_backward_kernel<7, true> — at the size it times it: the
    gated op with bench.py's own gate (pixel owners from the render of the perturbed map) against the gated oracle, fp64 beside,
    the same bars as the ungated case."""
    _full_size_case(oracle, 3, "cfg3_gated", gated=True)


def test_cfg3_fused_iteration_vs_cpu_oracle_iteration(torch_cuda, oracle):
    fs, gs = U.fused_iteration_case(torch_cuda, oracle, 3)
    _report("cfg3_fused_iteration", fs, gs)


def test_cfg5_fused_iteration_vs_cpu_oracle_iteration(torch_cuda, oracle):
    """The same at 2 M Gaussians, where the timed path also splits its long tile lists (list_split "auto": composed transmittance maps
    in the forward, the queue of long-list sorts) — bench.py --cfg 5's instantiation."""
    fs, gs = U.fused_iteration_case(torch_cuda, oracle, 5)
    _report("cfg5_fused_iteration", fs, gs)


def test_cfg2_full_size_vs_oracle(torch_cuda, oracle):
    """BASELINE config 2: 100 000 Gaussians, 1200x680."""
    _full_size_case(oracle, 2, "cfg2")


def test_cfg4_full_size_vs_oracle(torch_cuda, oracle):
    """BASELINE config 4's map on ONE GPU: 1 000 000 Gaussians, 16 object ids."""
    _full_size_case(oracle, 4, "cfg4")


def test_cfg5_full_size_vs_oracle(torch_cuda, oracle):
    """BASELINE config 5's map on ONE GPU: 2 000 000 Gaussians, SH degree 3 with non-zero higher-order coefficients."""
    _full_size_case(oracle, 5, "cfg5")


def test_backward_is_bitwise_reproducible(torch_cuda, cfg3):
    """No global float atomics in the backward (the only float adds that go through memory are wave-private LDS adds of one
    instruction's lanes, served in a fixed order): two runs give identical bits (the reference's atomicAdd order varies, B10)."""
    cam, sc, dL = cfg3
    _, g1 = U.run_hip(cam, sc, dL=dL)
    _, g2 = U.run_hip(cam, sc, dL=dL)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


def test_backward_is_linear_in_the_incoming_gradient(torch_cuda, cfg3):
    """d(loss)/d(params) is a linear map of (dL/dcolor, dL/ddepth): backward(a) + backward(b) == backward(a + b) up to fp32
    rounding of the sums (size-independent property, checked at full size)."""
    cam, sc, dL = cfg3
    rng = np.random.default_rng(12)
    dL2 = (rng.normal(size=dL[0].shape).astype(np.float32), rng.normal(size=dL[1].shape).astype(np.float32))
    _, ga = U.run_hip(cam, sc, dL=dL)
    _, gb = U.run_hip(cam, sc, dL=dL2)
    _, gs = U.run_hip(cam, sc, dL=(dL[0] + dL2[0], dL[1] + dL2[1]))
    for k in ga:
        want = ga[k].astype(np.float64) + gb[k].astype(np.float64)
        e = U._row_err(gs[k], want)
        # fp32 rounding of the sums, amplified on the few ill-conditioned rows of the per-Gaussian chain (util_rast.compare_grads)
        assert (e > 2e-4).sum() <= 1e-3 * e.size and e.max() < 5e-2, (k, e.max(), int((e > 2e-4).sum()))


def test_tile_mask_restricts_without_changing_unmasked_tiles(torch_cuda, cfg3):
    """Rendering with a tile mask equals the unmasked render on every unmasked tile (bitwise) and leaves masked tiles at
    the reference's initial fills; gradients of Gaussians that only touch masked tiles vanish."""
    cam, sc, dL = cfg3
    gy, gx = (cam.H + 15) // 16, (cam.W + 15) // 16
    mask = (np.random.default_rng(13).uniform(size=(gy, gx)) < 0.5).astype(np.int32)
    pm = np.repeat(np.repeat(mask, 16, 0), 16, 1)[:cam.H, :cam.W].astype(bool)
    full, _ = U.run_hip(cam, sc)
    part, gpart = U.run_hip(cam, sc, tile_mask=mask, dL=dL)
    for k in ("color", "depth", "hit_color", "hit_depth", "hit_color_weight", "hit_depth_weight", "T_map"):
        a, b = full[k], part[k]
        assert np.array_equal(a[..., pm], b[..., pm]), k
    assert (part["color"][:, ~pm] == 0).all() and (part["T_map"][0][~pm] == 1).all() and (part["hit_depth"][0][~pm] == 0).all()
    # a Gaussian whose whole tile rect is masked receives exactly zero gradient
    _, gfull = U.run_hip(cam, sc, dL=(dL[0] * pm, dL[1] * pm))
    for k in gpart:
        want = gfull[k].astype(np.float64)
        scale = np.abs(want).max() + 1e-30
        assert np.abs(gpart[k] - want).max() / scale < 2e-4, k
