"""GPU: every Gaussian's gradient held to its OWN magnitude (util_rast.compare_grads_own_row, fp64 oracle as the truth) under incoming
gradients whose per-pixel terms cannot cancel (util_rast.colour_probe, uniform_colour_probe, disjoint_pixel_probe), at the shapes where
the kernels go wrong: the sort-path boundaries, the split backward, odd image sizes, every SH degree, a tile mask, the object gate, the
full-size scene and the timed path (FusedMapper's fused tail).  compare_grads holds a row to the TENSOR's largest magnitude, so the small
rows (deep in long lists, low transmittance, tile edges) are hardly checked there; here every row is.

Per case and tensor the numbers (rows checked, rows covered by the disjoint probe, rows explained, worst row-own error of HIP and of the
fp32 oracle) go to stdout, and to $DQO_REPORT_DIR/grad_rows_<case>.json when that variable names a directory."""
import json
import os

import numpy as np
import pytest

from dqo_harness import scenes
import util_rast as U

pytestmark = pytest.mark.gpu

ALL = ("means3D", "sh", "opacity", "scales", "rotations")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()
    return torch


@pytest.fixture
def dgr():
    import diff_gaussian_rasterization_depth as dgr
    yield dgr
    dgr.set_list_split(0)


def _report(name, rep):
    print(name, json.dumps(rep))
    out = os.environ.get("DQO_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"grad_rows_{name}.json"), "w") as fh:
            json.dump(rep, fh, indent=1)


def _pair(oracle, cam, sc, omp, **kw):
    """HIP forward (kept for several backwards) and the fp32 / fp64 oracle forwards; the flipped pixels of the three."""
    hr = U.HipRun(cam, sc, **kw)
    o, r, _ = U.run_oracle(oracle, cam, sc, omp=omp, **kw)
    o64, r64, _ = U.run_oracle(oracle, cam, sc, dtype=np.float64, omp=omp, **kw)
    bad = U.flipped_pixels(hr.res, r, r64)
    U.compare_forward(hr.res, r, r64)
    return hr, o, r, o64, bad


def _probe(hr, o, o64, bad, dL, keys, precomp, what):
    """One incoming gradient, zeroed on the flipped pixels for both sides (as parity_case does), HIP vs the oracle pair."""
    keep = (~bad).astype(np.float32)
    dLm = (dL[0] * keep[None], dL[1] * keep[None])
    hg = hr.backward(dLm, retain=True)
    g32, g64 = U.oracle_backward(o, dLm, precomp), U.oracle_backward(o64, dLm, precomp)
    return U.compare_grads_own_row(hg, g32, g64, keys=keys, what=what), g64


def _merge(acc, st):
    for k, s in st.items():
        a = acc.setdefault(k, dict(rows=0, nonzero=0, beyond_bar=0, explained=0, oracle_beyond_half_bar=0, worst_hip=0.0,
                                   worst_oracle=0.0, worst_hip_unexplained_excluded=0.0))
        for f in ("nonzero", "beyond_bar", "explained", "oracle_beyond_half_bar"):
            a[f] += s[f]
        a["rows"] = s["rows"]
        for f in ("worst_hip", "worst_oracle", "worst_hip_unexplained_excluded"):
            a[f] = max(a[f], s[f])


def rows_case(oracle, name, cam, sc, probes=("colour", "disjoint"), rounds=4, min_cover=None, omp=False, seed=0, dL_mask=None,
              **kw):
    """The probes on one scene.  colour: sh (or colors); uniform: colors + opacity on a colors_precomp forward with bg = 0; disjoint:
    all five tensors over `rounds` selections, with the fraction of visible rows that received a term asserted >= min_cover.
    dL_mask (bool [H, W]): the incoming gradient is zero outside it (quadrants that get no gradient)."""
    rep = {}
    sh_path = kw.get("colors_precomp") is None
    keys = ALL if sh_path else tuple("colors" if k == "sh" else k for k in ALL)
    colour_key = ("sh",) if sh_path else ("colors",)
    need_main = "colour" in probes or "disjoint" in probes
    if need_main:
        hr, o, r, o64, bad = _pair(oracle, cam, sc, omp, **kw)
        excl = bad if dL_mask is None else (bad | ~dL_mask)
        rep["flipped_px"] = int(bad.sum())
    if "colour" in probes:
        dL = U.colour_probe(cam, seed + 1)
        if dL_mask is not None:
            dL = (dL[0] * dL_mask[None], dL[1])
        rep["colour"], _ = _probe(hr, o, o64, bad, dL, colour_key, not sh_path, f"{name} colour probe")
    if "disjoint" in probes:
        vis = r["radii"] > 0
        got = np.zeros_like(vis)
        acc = {}
        for p in U.disjoint_pixel_probe(o, r["hit_depth"], seed + 2, rounds, exclude=excl):
            st, g64 = _probe(hr, o, o64, bad, p["dL"], keys, not sh_path, f"{name} disjoint probe")
            for k in keys:
                nz = (np.abs(g64[k]).reshape(len(vis), -1) > 0).any(1)
                assert not (nz & ~p["covered"]).any(), f"{name} {k}: a row outside the selection received a term"
                got |= nz
            _merge(acc, st)
        cover = float(got[vis].mean()) if vis.any() else 0.0
        for k in acc:
            acc[k]["covered_rows"] = int(got.sum())
        rep["disjoint"] = dict(acc, visible_rows=int(vis.sum()), covered_fraction=cover)
        if min_cover is not None:
            assert cover >= min_cover, f"{name}: the disjoint probe reached {cover:.3f} of the visible rows, floor {min_cover}"
    if "uniform" in probes:
        cp, dL = U.uniform_colour_probe(cam, len(sc["xyz"]), seed + 3)
        if dL_mask is not None:
            dL = (dL[0] * dL_mask[None], dL[1])
        ukw = dict(kw, colors_precomp=cp, bg=(0, 0, 0))
        hu, ou, _, ou64, badu = _pair(oracle, cam, sc, omp, **ukw)
        rep["uniform"], _ = _probe(hu, ou, ou64, badu, dL, ("colors", "opacity"), True, f"{name} uniform-colour probe")
    _report(name, rep)
    return rep


# ---- the benchmark scenes ----

def test_cfg1(torch_cuda, oracle):
    cam, sc = scenes.make_config(1)
    rows_case(oracle, "cfg1", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=8, min_cover=0.1)


def test_cfg1_background(torch_cuda, oracle):
    """bg != 0 enters dL/dalpha only: the colour probe still has no cancelling term."""
    cam, sc = scenes.make_config(1)
    rows_case(oracle, "cfg1_bg", cam, sc, probes=("colour", "disjoint"), rounds=2, bg=(0.3, 0.5, 0.7))


@pytest.mark.parametrize("P", [100_000, 500_000])
def test_cfg3(torch_cuda, oracle, P):
    cam, sc = scenes.make_config(3, P=P)
    rows_case(oracle, f"cfg3_{P // 1000}k", cam, sc, probes=("colour", "disjoint", "uniform") if P <= 100_000 else ("colour", "disjoint"),
              rounds=4, min_cover=0.05, omp=True)


def test_cfg3_gated(torch_cuda, oracle):
    """The gated op (blend kernels' GATE instantiation) with bench.py's own gate."""
    cam, sc = scenes.make_config(3, P=100_000)
    go, po, _ = U.bench_gate(3, cam, sc)
    rows_case(oracle, "cfg3_100k_gated", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=4, min_cover=0.05, omp=True,
              object_gate=(go, po))


# ---- long lists across the sort-path boundaries ----

def _one_tile_scene(n):
    """test_gpu_rast_edge.py::test_sort_paths_at_their_boundaries: exactly n semi-transparent surfels in one tile."""
    cam = scenes.Camera(48, 32, 60.0, 60.0, 23.5, 15.5)
    rng = np.random.default_rng(n)
    sc = scenes.frustum_cloud(11, n, cam, zmin=1.0, zmax=4.0)
    z = np.round(rng.uniform(1.0, 4.0, n) * 8) / 8
    u, v = rng.uniform(20.5, 27.5, n), rng.uniform(4.5, 11.5, n)
    pc = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], 1)
    sc["xyz"] = ((pc - cam.t) @ cam.Rw2c).astype(np.float32)
    sc["scales"] = (rng.uniform(0.004, 0.012, (n, 3)) * z[:, None]).astype(np.float32)
    sc["opacity"] = rng.uniform(0.01, 0.04, (n, 1)).astype(np.float32)
    return cam, sc


@pytest.mark.parametrize("n", [511, 513, 1025, 2049, 4097, 8193])
def test_sort_path_boundaries(torch_cuda, oracle, n):
    cam, sc = _one_tile_scene(n)
    rep = rows_case(oracle, f"one_tile_{n}", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=4)
    assert rep["colour"]["sh"]["nonzero"] >= 0.9 * n  # every entry of the list is walked (semi-transparent)


@pytest.mark.parametrize("P", [1300, 2800, 9000])
def test_long_tile_lists_global_sort(torch_cuda, oracle, P):
    """test_gpu_rast_edge.py::test_long_tile_lists_global_sort's scenes: lists of 513..1024, > 1024 and > 4096 entries."""
    cam = scenes.Camera(96, 64, 80.0, 80.0, 47.5, 31.5)
    rng = np.random.default_rng(0)
    sc = scenes.frustum_cloud(5, P, cam, zmin=1.0, zmax=4.0)
    pc = np.stack([rng.uniform(-0.12, 0.12, P), rng.uniform(-0.12, 0.12, P), rng.uniform(1.0, 4.0, P)], 1)
    pc[:, :2] *= pc[:, 2:3]
    sc["xyz"] = pc.astype(np.float32)
    sc["opacity"] = rng.uniform(0.02, 0.08, (P, 1)).astype(np.float32)
    rows_case(oracle, f"long_lists_{P}", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=4)


# ---- the split backward ----

@pytest.mark.parametrize("runs", [64, 256])
def test_split_backward(torch_cuda, oracle, dgr, runs):
    """set_list_split(runs) before the forward: its context carries the split into the backward (test_gpu_list_split.py's scenes)."""
    cam, sc = scenes.make_config(3, P=30000)
    dgr.set_list_split(runs)
    try:
        rows_case(oracle, f"split_{runs}_cfg3_30k", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=4, min_cover=0.2)
    finally:
        dgr.set_list_split(0)


@pytest.mark.parametrize("runs", [64, 256])
def test_split_backward_with_quadrants_that_get_no_gradient(torch_cuda, oracle, dgr, runs):
    """test_gpu_list_split.py::test_split_backward_with_quadrants_that_get_no_gradient's scene: half the image carries no incoming
    gradient (the split backward's early exit)."""
    cam, sc = scenes.make_config(5, P=120000)
    half = np.zeros((cam.H, cam.W), bool)
    half[:, : cam.W // 2] = True
    dgr.set_list_split(runs)
    try:
        rows_case(oracle, f"split_{runs}_cfg5_120k_half", cam, sc, probes=("colour", "disjoint"), rounds=3, min_cover=0.02, omp=True,
                  dL_mask=half)
    finally:
        dgr.set_list_split(0)


# ---- image shapes, SH degrees, tile mask ----

@pytest.mark.parametrize("W,H", [(17, 9), (333, 47)])
def test_odd_image_sizes(torch_cuda, oracle, W, H):
    """Off-centre principal point as in test_gpu_rast_edge.py::test_odd_image_sizes."""
    cam = scenes.Camera(W, H, 0.8 * W, 0.8 * W, W / 2 - 0.3, H / 2 + 0.2, scenes.rot_yx(3.0, -2.0), np.array([0.01, 0.02, 0.0]))
    sc = scenes.frustum_cloud(W, 800, cam, zmin=0.8, zmax=3.0)
    sc["scales"] = (sc["scales"] * 3).astype(np.float32)
    rows_case(oracle, f"odd_{W}x{H}", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=6)


def test_off_centre_principal_point(torch_cuda, oracle):
    cam0, _ = scenes.make_config(1)
    cam = scenes.Camera(cam0.W, cam0.H, cam0.fx, cam0.fy, cam0.cx + 57.3, cam0.cy - 41.8, scenes.rot_yx(7.0, -3.0),
                        np.array([0.05, -0.02, 0.1]))
    sc = scenes.frustum_cloud(1, 10000, cam)
    rows_case(oracle, "off_centre", cam, sc, probes=("colour", "disjoint"), rounds=4, min_cover=0.05)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degrees(torch_cuda, oracle, deg):
    cam, sc = scenes.make_config(3, P=30000)
    rows_case(oracle, f"sh_degree_{deg}", cam, sc, probes=("colour", "disjoint"), rounds=2, sh_degree=deg)


def test_tile_mask(torch_cuda, oracle):
    cam, sc = scenes.make_config(3, P=30000)
    gy, gx = (cam.H + 15) // 16, (cam.W + 15) // 16
    mask = (np.random.default_rng(13).uniform(size=(gy, gx)) < 0.5).astype(np.int32)
    rows_case(oracle, "tile_mask", cam, sc, probes=("colour", "disjoint", "uniform"), rounds=3, min_cover=0.1, tile_mask=mask)


# ---- the timed path ----

def test_fused_iteration_colour_probe(torch_cuda, oracle):
    """FusedMapper (loss tap, fused tail, tile buckets, bench.py's gate, list_split "auto") for one captured iteration, as
    util_rast.fused_iteration_case, with gt_color = 0 and depth_weight = 0: the L1 colour gradient is +w_k (the object's weight) on
    every covered pixel and exactly 0 in depth — a colour probe.  The gradient the tail consumed is m / (1 - beta1) of its first Adam
    moment; shs held row-own against the oracle iteration (per-object masked loss -> oracle backward, fp64 as the truth)."""
    torch = torch_cuda
    from dqo_harness import mapping, sharding
    from dqo_harness.fused_mapping import FusedMapper
    from oracle import map_oracle as mo
    cam, sc = scenes.make_config(3)
    go, po, tgt = U.bench_gate(3, cam, sc)
    dev = torch.device("cuda")
    settings = mapping.make_settings(cam, dev)
    own = po >= 0
    tile_mask = sharding.tile_mask_from_pixel_mask(own)
    fm = FusedMapper(sc, settings, dev, depth_weight=0.0).set_object_gate(go, po)
    act = [a.detach().cpu().numpy().copy() for a in fm.activate()]
    sca = dict(sc, opacity=act[0], scales=act[1], rotations=act[2])
    hr = U.HipRun(cam, sca, grad=False, object_gate=(go, po), tile_mask=tile_mask)
    st = U.oracle_settings(oracle, cam)
    orc = {}
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        o = oracle.OracleRasterizer(dt, omp=True)
        r = o.forward(st, sca["xyz"], sca["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center, shs=sca["shs"],
                      scales=sca["scales"], rotations=sca["rotations"], tile_mask=tile_mask, gaussian_object=go, pixel_object=po)
        orc[name] = (o, r, {k: getattr(r, k) for k in U.HipRun.names})
    bad = U.flipped_pixels(hr.res, orc["f32"][2], orc["f64"][2])
    assert bad[own].mean() <= 1e-3
    mask = own & ~bad
    gtc = torch.zeros_like(tgt["gt_color"])
    fm.capture(gtc, tgt["gt_depth"], torch.tensor(mask, device=dev), tile_mask=torch.tensor(tile_mask, device=dev),
               loss_tap=True, fused_tail=True, list_split="auto")
    torch.cuda.synchronize()
    assert not fm.graph_overflowed() and fm.step_count == 1
    assert float(fm.loss[2].item()) >= 0.0
    hg = dict(sh=(fm.state["shs"][0].double() / (1.0 - fm.betas[0])).cpu().numpy())
    og = {}
    for name in ("f32", "f64"):
        o, r, _ = orc[name]
        tot, col, dep, dC, dD = mo.per_object_masked_loss(r.color, r.depth, r.hit_depth, np.zeros_like(r.color), tgt["gt_depth"].cpu().numpy(),
                                                          po, mask, depth_weight=0.0)
        if name == "f32":
            dL = (dC.astype(np.float32), dD.astype(np.float32))
            assert (dL[0] >= 0).all() and not dL[1].any(), "depth_weight = 0 and gt_color = 0 must make the loss gradient a colour probe"
            np.testing.assert_allclose(fm.loss[:3].double().cpu().numpy(), [tot, col, dep], rtol=1e-5)
        og[name] = dict(sh=np.asarray(o.backward(*dL).sh))
    st_ = U.compare_grads_own_row(hg, og["f32"], og["f64"], keys=("sh",), what="fused iteration")
    _report("fused_iteration_cfg3", dict(flipped_px=int(bad[own].sum()), list_split=[int(fm._g.ls_fwd), int(fm._g.ls_bwd)],
                                              colour=st_))
