"""Helpers shared by the GPU parity tests: run the HIP operator (through the drop-in Python surface, i.e. through the C ABI)
and the CPU oracle on the same seeded inputs."""
import math

import numpy as np

NT60 = math.cos(math.radians(60.0))


def raster_settings_torch(cam, device, sh_degree=3, bg=(0, 0, 0), **kw):
    import torch
    from diff_gaussian_rasterization_depth import GaussianRasterizationSettings
    d = dict(opaque_threshold=0.6, depth_threshold=1.0, normal_threshold=NT60, color_sigma=3.0, T_threshold=1e-4, scale_modifier=1.0)
    d.update(kw)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=device)
    return GaussianRasterizationSettings(
        image_height=cam.H, image_width=cam.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=t(bg), scale_modifier=d["scale_modifier"],
        viewmatrix=t(cam.world_view_transform), projmatrix=t(cam.full_proj_transform), sh_degree=sh_degree, campos=t(cam.camera_center),
        opaque_threshold=d["opaque_threshold"], normal_threshold=d["normal_threshold"], depth_threshold=d["depth_threshold"],
        prefiltered=bool(d.get("prefiltered", False)), debug=False, cx=cam.cx, cy=cam.cy, color_sigma=d["color_sigma"],
        T_threshold=d["T_threshold"])


def oracle_settings(ol, cam, sh_degree=3, bg=(0, 0, 0), **kw):
    d = dict(opaque_threshold=0.6, depth_threshold=1.0, normal_threshold=NT60, color_sigma=3.0, T_threshold=1e-4, scale_modifier=1.0)
    d.update(kw)
    d.pop("prefiltered", None)  # (the reference only traps on it, auxiliary.h:155-161: no effect on any output)
    return ol.RastSettings(cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, sh_degree=sh_degree, bg=bg, **d)


class HipRun:
    """One forward of the HIP operator (through the drop-in Python surface = through the C ABI) whose backward can be called
    afterwards — several times — with incoming gradients chosen after looking at the forward's outputs."""

    names = ("color", "depth", "hit_color", "hit_depth", "hit_color_weight", "hit_depth_weight", "T_map", "n_touched", "radii")

    def __init__(self, cam, sc, device="cuda", tile_mask=None, colors_precomp=None, grad=True, sh_degree=3, bg=(0, 0, 0), object_gate=None,
                 **kw):
        """object_gate = (gaussian_object [P], pixel_object [H, W]) int arrays: the gated op (rasterize_gaussians_gated)."""
        import torch
        from diff_gaussian_rasterization_depth import GaussianRasterizer, rasterize_gaussians_gated
        self.torch, self.device = torch, device
        rs = raster_settings_torch(cam, device, sh_degree=sh_degree, bg=bg, **kw)
        rast = GaussianRasterizer(rs)
        t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=device, requires_grad=grad)
        self.xyz, self.opac, self.scales, self.rots = t(sc["xyz"]), t(sc["opacity"]), t(sc["scales"]), t(sc["rotations"])
        self.shs = t(sc["shs"]) if colors_precomp is None else None
        self.cp = t(colors_precomp) if colors_precomp is not None else None
        tm = None if tile_mask is None else torch.tensor(np.ascontiguousarray(tile_mask, np.int32), device=device)
        if object_gate is None:
            self.out = rast(means3D=self.xyz, opacities=self.opac, shs=self.shs, colors_precomp=self.cp, scales=self.scales,
                            rotations=self.rots, tile_mask=tm)
        else:
            e = torch.Tensor([])
            go = torch.tensor(np.ascontiguousarray(object_gate[0], np.int32), device=device)
            po = torch.tensor(np.ascontiguousarray(object_gate[1], np.int32), device=device)
            self.out = rasterize_gaussians_gated(self.xyz, self.shs if self.shs is not None else e, self.cp if self.cp is not None else e,
                                                 self.opac, self.scales, self.rots, e, tm, rs, go, po)
        self.res = {k: v.detach().cpu().numpy() for k, v in zip(self.names, self.out)}

    def _leaves(self):
        d = dict(means3D=self.xyz, opacity=self.opac, scales=self.scales, rotations=self.rots)
        if self.shs is not None:
            d["sh"] = self.shs
        else:
            d["colors"] = self.cp
        return d

    def backward(self, dL, retain=True):
        """Gradients of sum(color * dL[0]) + sum(depth * dL[1]) w.r.t. the inputs (fresh tensors every call)."""
        torch = self.torch
        gC = torch.tensor(np.ascontiguousarray(dL[0], np.float32), device=self.device)
        gD = torch.tensor(np.ascontiguousarray(dL[1], np.float32), device=self.device)
        leaves = self._leaves()
        gs = torch.autograd.grad([self.out[0], self.out[1]], list(leaves.values()), [gC, gD], retain_graph=retain)
        return {k: g.detach().cpu().numpy() for k, g in zip(leaves, gs)}


def run_hip(cam, sc, device="cuda", tile_mask=None, colors_precomp=None, dL=None, sh_degree=3, bg=(0, 0, 0), **kw):
    """Returns (outputs dict of numpy arrays, grads dict or None)."""
    r = HipRun(cam, sc, device=device, tile_mask=tile_mask, colors_precomp=colors_precomp, grad=dL is not None, sh_degree=sh_degree,
               bg=bg, **kw)
    return r.res, (None if dL is None else r.backward(dL, retain=False))


def run_oracle(ol, cam, sc, tile_mask=None, colors_precomp=None, dL=None, sh_degree=3, bg=(0, 0, 0), dtype=np.float32, object_gate=None,
               omp=False, **kw):
    o = ol.OracleRasterizer(dtype, omp=omp)
    st = oracle_settings(ol, cam, sh_degree=sh_degree, bg=bg, **kw)
    r = o.forward(st, sc["xyz"], sc["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                  shs=None if colors_precomp is not None else sc["shs"], colors_precomp=colors_precomp, scales=sc["scales"],
                  rotations=sc["rotations"], tile_mask=tile_mask,
                  **({} if object_gate is None else dict(gaussian_object=object_gate[0], pixel_object=object_gate[1])))
    res = dict(color=r.color, depth=r.depth, hit_color=r.hit_color, hit_depth=r.hit_depth, hit_color_weight=r.hit_color_weight,
               hit_depth_weight=r.hit_depth_weight, T_map=r.T_map, n_touched=r.n_touched, radii=r.radii)
    grads = None if dL is None else oracle_backward(o, dL, colors_precomp is not None)
    return o, res, grads


def oracle_backward(o, dL, precomp=False):
    """Backward of an oracle object whose forward has run (may be called repeatedly with different incoming gradients)."""
    g = o.backward(np.ascontiguousarray(dL[0], np.float32), np.ascontiguousarray(dL[1], np.float32))
    grads = dict(means3D=g.means3D, opacity=g.opacity, scales=g.scales, rotations=g.rotations)
    if not precomp:
        grads["sh"] = g.sh
    else:
        grads["colors"] = g.colors
    return grads


def flipped_pixels(h, o, o64=None):
    """[H, W] bool: pixels where a DISCRETE decision of the blend loop differs between the two evaluations.  alpha >= 1/255,
    alpha >= opaque_threshold, T' < T_threshold and w > w_max sit behind float compares, so a last-ulp difference of exp() (v_exp_f32
    vs libm) can flip one; the pixel's outputs then differ by a whole contribution.  SURVEY.md §8(d): such pixels are counted
    against a budget (<= 0.1 % of the image) and excluded from the continuous comparisons — forward AND backward (the incoming
    gradient is zeroed on them for both sides)."""
    bad = (h["hit_depth"] != o["hit_depth"]) | (h["hit_color"] != o["hit_color"])
    # a flipped contributor decision also shows up as a RELATIVE jump of the final T of at least 1/255 = 3.9e-3 (every blended entry
    # multiplies T by 1 - alpha), where unflipped pixels agree to ~1e-5 relative however small T has become (T >= 1e-6: T_threshold
    # x (1 - 0.99)).  Relative, not absolute: the flipped entry may sit early in the list, at T = 0.06, with a final T of 1e-4.
    bad |= np.abs(h["T_map"] - o["T_map"]) > 1e-3 * np.abs(o["T_map"])
    if o64 is not None:
        bad |= (o64["hit_depth"] != o["hit_depth"]) | (o64["hit_color"] != o["hit_color"])
        bad |= np.abs(o64["T_map"] - o["T_map"]) > 1e-3 * np.abs(o["T_map"])
    return bad[0]


def forward_errors(a, b, ok):
    """max |a - b| per continuous output over the pixels `ok`."""
    return {k: (float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))[:, ok].max()) if ok.any() else 0.0)
            for k in ("color", "depth", "hit_color_weight", "hit_depth_weight", "T_map")}


def compare_forward(h, o, o64=None, max_mismatch_frac=1e-3, tol=1e-4):
    """Parity bar of BASELINE.json north_star: RGB / depth (and the weight / T maps) within 1e-4 of the fp32 oracle, no slack
    term; discrete maps bit-exact up to the mismatch budget of flipped_pixels().  `o64` (optional, the fp64 oracle) only widens
    the flipped set by the pixels where the fp32 oracle itself flips against fp64, and adds HIP-vs-fp64 numbers to the report."""
    HW = h["depth"].size
    bad = flipped_pixels(h, o, o64)
    frac = bad.sum() / HW
    assert frac <= max_mismatch_frac, f"index-map mismatch {frac:.2e} over budget"
    ok = ~bad
    stats = forward_errors(h, o, ok)
    for k, v in stats.items():
        assert v <= tol, f"{k}: max abs diff {v:.3e} > {tol} (vs fp32 oracle)"
    if o64 is not None:
        stats["vs_fp64"] = forward_errors(h, o64, ok)
        stats["oracle32_vs_fp64"] = forward_errors(o, o64, ok)
    np.testing.assert_array_equal(h["radii"], o["radii"])
    nt = np.abs(h["n_touched"].astype(np.int64) - o["n_touched"].astype(np.int64))
    assert nt.sum() <= max(8, 4 * bad.sum()), f"n_touched differs by {nt.sum()} counts"
    stats["mismatch_px"] = int(bad.sum())
    return stats


def grad_errors(a, truth):
    """(max abs error / max |truth|, 99th percentile of the per-Gaussian row error relative to the row's own magnitude)."""
    a, truth = a.reshape(truth.shape).astype(np.float64), truth.astype(np.float64)
    scale = np.abs(truth).max() + 1e-30
    tmax = np.abs(a - truth).max() / scale
    rows_t = truth.reshape(truth.shape[0], -1) if truth.ndim > 1 else truth.reshape(-1, 1)
    rows_a = a.reshape(rows_t.shape)
    rel = np.abs(rows_a - rows_t).max(1) / (np.abs(rows_t).max(1) + 1e-3 * scale)
    return float(tmax), (float(np.quantile(rel, 0.99)) if rel.size else 0.0)


def _row_err(a, truth):
    """Per-Gaussian (row) max abs error relative to the TENSOR's largest magnitude."""
    truth = truth.astype(np.float64)
    a = a.reshape(truth.shape).astype(np.float64)
    scale = np.abs(truth).max() + 1e-30
    rows_t = truth.reshape(truth.shape[0], -1) if truth.ndim > 1 else truth.reshape(-1, 1)
    return np.abs(a.reshape(rows_t.shape) - rows_t).max(1) / scale


def unexplained_cap(rows):
    """Rows that may sit beyond the bar WITHOUT an explanation: NONE (rounds 3-5 allowed max(1, 1e-5 x rows); since the derivative of the
    2x2 inverse runs in double — csrc/dqo_gauss_chain.h — the HIP chain no longer adds float noise of its own to those rows)."""
    return 0


def _describe_rows(idx, e, e_o=None, e_h=None, limit=5):
    """The worst rows of a set, for an assert message / the report: (row, error vs the fp32 oracle[, the fp32 oracle's own error vs fp64,
    the HIP error vs fp64])."""
    order = idx[np.argsort(-e[idx])][:limit]
    return [dict(row=int(i), err_vs_fp32_oracle=float(e[i]), **({} if e_o is None else dict(fp32_oracle_vs_fp64=float(e_o[i]), hip_vs_fp64=float(e_h[i]))))
            for i in order]


def compare_grads(hg, og, og64=None, rtol=1e-3):
    """Gradients within 1e-3 of the fp32 oracle (north_star), per Gaussian row, relative to the tensor's largest magnitude — no
    slack term.  Callers zero the incoming gradient on flipped_pixels() for both sides first.

    The reference's per-Gaussian chain (dL/dconic -> cov2D -> cov3D -> scale / quaternion, backward.cu:331-355, 426-487) is
    ill-conditioned for thin surfels: on a few rows ANY two float32 evaluations disagree in the second digit, the reference with
    itself included (its float atomicAdd order changes from run to run, quirk B10).  A row beyond the bar must therefore be EXPLAINED:
    with the fp64 oracle beside (every full-size configuration runs it), the fp32 ORACLE ITSELF is off its fp64 twin by more than a
    third of the bar on that row and the HIP result is no further from fp64 than TWICE what the oracle is — ill-conditioned, not wrong.
    Unexplained rows (all rows beyond the bar when there is no fp64 oracle) are not allowed (unexplained_cap = 0); they are named in the
    assert message (row, its three errors).
    Returns per tensor a dict: max_row_err, q99 (99th percentile of the row error relative to the row's own magnitude), rows,
    beyond_bar, explained, unexplained, worst_explained, worst_unexplained."""
    stats = {}
    for k in og:
        e = _row_err(hg[k], og[k])
        out = e > rtol
        n_out, n = int(out.sum()), int(e.size)
        tmax, q99 = grad_errors(hg[k], og[k])
        expl = np.zeros_like(out)
        e_o = e_h = None
        if n_out and og64 is not None:
            e_o = _row_err(og[k], og64[k])
            e_h = _row_err(hg[k], og64[k])
            expl = out & (e_o > 0.3 * rtol) & (e_h <= 2 * e_o)
        unexp = out & ~expl
        n_unexp = int(unexp.sum())
        stats[k] = dict(max_row_err=float(e.max()) if n else 0.0, q99=q99, rows=n, beyond_bar=n_out, explained=int(expl.sum()),
                        unexplained=n_unexp, worst_explained=float(e[expl].max()) if expl.any() else 0.0,
                        worst_unexplained=float(e[unexp].max()) if n_unexp else 0.0)
        if n_unexp:  # which rows, and what is known about them (an unexplained row is either not ill-conditioned by the fp64 test, or the
            # HIP value is further from fp64 than 3x the fp32 oracle is)
            stats[k]["unexplained_rows"] = _describe_rows(np.nonzero(unexp)[0], e, e_o, e_h)
        assert n_unexp <= unexplained_cap(n), (
            f"grad {k}: {n_unexp} of {n} rows are off the fp32 oracle by more than {rtol:.0e} of the largest magnitude"
            + (" with no fp64 oracle to explain them" if og64 is None else
               " and are NOT explained by the fp32 oracle's own error against fp64 (explained = fp32 oracle off fp64 by > 0.3 x bar on "
               "the row AND hip no further from fp64 than 2 x that)")
            + f"; cap {unexplained_cap(n)} rows; worst rows: {stats[k]['unexplained_rows']}")
        if n >= 1000:
            assert q99 <= rtol, f"grad {k}: 99% row-wise error {q99:.3e} > {rtol:.1e} (vs fp32 oracle)"
    if og64 is not None:
        stats["vs_fp64"] = {k: grad_errors(hg[k], og64[k]) for k in og}
        stats["oracle32_vs_fp64"] = {k: grad_errors(og[k], og64[k]) for k in og}
    return stats


def assert_grads_match(ga, gb, what="", rtol=1e-3):
    """Two HIP evaluations of the same gradients that differ by ROUNDING only (another summation order, a forward whose per-pixel state
    differs in the last bits): EVERY Gaussian row within `rtol` of the tensor's largest magnitude.  (Rounds 4-5 let max(2, 2e-5 x rows)
    rows go up to 1e-2: the float evaluation of the 2x2 inverse's derivative amplified last-bit differences of its inputs ~1e4 times on a
    handful of thin surfels; in double — csrc/dqo_gauss_chain.h — it does not.)"""
    for k in ga:
        e = _row_err(gb[k], ga[k])
        assert (e.max() if e.size else 0.0) <= rtol, (what, k, int((e > rtol).sum()), float(e.max()))


def parity_case(ol, cam, sc, dL, fp64=False, device="cuda", **kw):
    """The full protocol on one scene: forward of HIP and oracle, flipped pixels, incoming gradient zeroed on them for BOTH, then
    backward of both.  Returns (forward stats, gradient stats)."""
    hr = HipRun(cam, sc, device=device, **kw)
    o, r, _ = run_oracle(ol, cam, sc, **kw)
    o64 = r64 = None
    if fp64:
        o64, r64, _ = run_oracle(ol, cam, sc, dtype=np.float64, **kw)
    bad = flipped_pixels(hr.res, r, r64)
    fs = compare_forward(hr.res, r, r64)
    keep = (~bad).astype(np.float32)
    dLm = (dL[0] * keep[None], dL[1] * keep[None])
    precomp = kw.get("colors_precomp") is not None
    hg = hr.backward(dLm, retain=False)
    og = oracle_backward(o, dLm, precomp)
    og64 = oracle_backward(o64, dLm, precomp) if fp64 else None
    gs = compare_grads(hg, og, og64)
    return fs, gs


def bench_gate(cfg, cam, sc, **settings_kw):
    """The object gate of the per-object job exactly as bench.py builds it (build_problem -> mapping.perturbed_target): a pixel belongs
    to the object of the Gaussian that fixes its depth in the render of the perturbed map.  Returns (gaussian_object [P], pixel_object
    [H, W]) int32 arrays and the target's dict of GPU tensors."""
    import torch
    from dqo_harness import mapping, scenes
    dev = torch.device("cuda")
    tgt = mapping.perturbed_target(sc, mapping.make_settings(cam, dev, **settings_kw), dev, scenes.CONFIGS[cfg]["seed"] + 7)
    return np.asarray(sc["obj_id"], np.int32), tgt["pix_obj"].cpu().numpy().astype(np.int32), tgt



def fused_iteration_case(torch_cuda, oracle, cfg, P=None, bg=(0.0, 0.0, 0.0)):
    """ONE iteration of the path bench.py times (FusedMapper on cfg 3 at 500 k: tile_objects binning, gated blend kernels, the
    per-object loss tap, gaussian_tail_kernel with the sparse Adam — the capture's own eager iteration issues exactly the calls the
    graph holds) against the full CPU iteration bench.py's cpu_baseline runs: oracle raster forward (gated) -> per-object masked loss
    (oracle/map_oracle.py <- SLAM/multiprocess/mapper.py:836-875) -> oracle raster backward (backward.cu:808-1066, 152-548) ->
    activation Jacobians.  The gradient row of the fused tail never reaches HBM; its first Adam moment does:
    exp_avg / (1 - beta1) IS the gradient the tail consumed (zero moments before, attach loss zero at the initial state), compared
    through util_rast.compare_grads at 1e-3 with the fp64 oracle beside.  Flipped pixels (util_rast.flipped_pixels, found with the
    eager gated op on the same activated inputs) are taken out of the render mask on both sides."""
    torch = torch_cuda
    from dqo_harness import mapping, scenes, sharding
    from dqo_harness.fused_mapping import FusedMapper
    from oracle import map_oracle as mo
    cam, sc = scenes.make_config(cfg, P=P)
    go, po, tgt = bench_gate(cfg, cam, sc, bg=bg)
    dev = torch.device("cuda")
    settings = mapping.make_settings(cam, dev, bg=bg)
    own = po >= 0
    tile_mask = sharding.tile_mask_from_pixel_mask(own)
    fm = FusedMapper(sc, settings, dev).set_object_gate(go, po)
    # the rasteriser's inputs of the first iteration = the mapper's activations of its raw parameters (sigmoid(logit(o)) is o up to
    # an ulp): both the flipped-pixel probe and the oracle get exactly these
    act = [a.detach().cpu().numpy().copy() for a in fm.activate()]
    sca = dict(sc, opacity=act[0], scales=act[1], rotations=act[2])
    raw = [fm.opacity_raw.cpu().numpy().copy(), fm.scaling_raw.cpu().numpy().copy(), fm.rotation_raw.cpu().numpy().copy()]
    hr = HipRun(cam, sca, grad=False, object_gate=(go, po), tile_mask=tile_mask, bg=bg)
    st = oracle_settings(oracle, cam, bg=bg)
    orc = {}
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        o = oracle.OracleRasterizer(dt, omp=True)
        r = o.forward(st, sca["xyz"], sca["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center, shs=sca["shs"],
                      scales=sca["scales"], rotations=sca["rotations"], tile_mask=tile_mask, gaussian_object=go, pixel_object=po)
        orc[name] = (o, r, {k: getattr(r, k) for k in HipRun.names})
    bad = flipped_pixels(hr.res, orc["f32"][2], orc["f64"][2])
    assert bad[own].mean() <= 1e-3, f"flipped pixels {int(bad[own].sum())} over the 0.1 % budget"
    mask = own & ~bad
    gtc, gtd = tgt["gt_color"].cpu().numpy(), tgt["gt_depth"].cpu().numpy()
    # ---- the GPU iteration: capture() = one eager iteration of the graph's own calls (+ the capture, unused here) ----
    fm.capture(tgt["gt_color"], tgt["gt_depth"], torch.tensor(mask, device=dev), tile_mask=torch.tensor(tile_mask, device=dev),
               loss_tap=True, fused_tail=True, list_split="auto")
    torch.cuda.synchronize()
    assert not fm.graph_overflowed() and fm.step_count == 1
    loss_hip = fm.loss[:3].double().cpu().numpy()
    b1 = fm.betas[0]
    hg = {k: (fm.state[s][0].double() / (1.0 - b1)).cpu().numpy() for k, s in
          (("means3D", "xyz"), ("sh", "shs"), ("opacity", "opacity"), ("scales", "scaling"), ("rotations", "rotation"))}
    # ---- the CPU iteration ----
    og = {}
    for name in ("f32", "f64"):
        o, r, _ = orc[name]
        tot, col, dep, dC, dD = mo.per_object_masked_loss(r.color, r.depth, r.hit_depth, gtc, gtd, po, mask)
        if name == "f32":
            np.testing.assert_allclose(loss_hip, [tot, col, dep], rtol=1e-5, err_msg="loss of the fused iteration vs the CPU iteration")
            dL = (dC.astype(np.float32), dD.astype(np.float32))
        g = o.backward(*dL)  # (the same incoming gradient for the fp64 twin: it explains rows, it is not a second target)
        g_op, g_sc, g_rot = mo.raw_grads(raw[0], raw[1], raw[2], g.opacity, g.scales, g.rotations)
        og[name] = dict(means3D=np.asarray(g.means3D), sh=np.asarray(g.sh), opacity=g_op, scales=g_sc, rotations=g_rot)
    gs = compare_grads(hg, og["f32"], og["f64"])
    # the step was taken: every Gaussian with a gradient moved by about one learning rate (Adam's first step is lr x g / (|g| + eps))
    moved = (fm.xyz.cpu().numpy() != sc["xyz"]).any(1)
    has_g = (np.abs(og["f32"]["means3D"]) > 0).any(1)
    assert moved[has_g].mean() > 0.99 and not moved[~has_g & (hr.res["radii"] == 0)].any()
    fs = dict(loss_hip=loss_hip.tolist(), loss_oracle=[float(tot), float(col), float(dep)], flipped_px=int(bad[own].sum()), P=int(len(go)),
              N_reference=int(orc["f32"][1].num_rendered), N_kept=int(fm.header()["num_rendered"]))
    fs["list_split"] = [int(fm._g.ls_fwd), int(fm._g.ls_bwd)]
    return fs, gs


# ---------------------------------------------------------------------------------------------------------------------------------
# Row-own gradient parity: every Gaussian's gradient held to its OWN magnitude (compare_grads holds a row to the tensor's largest
# magnitude, so rows far below it — deep in long lists, at low transmittance, at tile edges — are hardly checked there).  A row-own bar
# only holds where the incoming gradient does not let the per-pixel terms of a row cancel; the probes below choose such gradients.
# ---------------------------------------------------------------------------------------------------------------------------------

# Calibrated with the fp32 oracle against fp64 (tests/test_grad_probes.py pins it): under colour_probe / uniform_colour_probe its worst
# row-own error is 2.7e-4 on cfg 1 and 4.2e-4 on cfg 3 at 30 k (median 4.5e-6), i.e. within rtol / 2 on every row.
OWN_ROW_RTOL = 2e-3
# Under disjoint_pixel_probe a row's single term still carries the pixel's own dL/dalpha = T sum_ch (col - accum_rec) dL_ch, which
# may nearly cancel: there the fp32 oracle is off fp64 by more than rtol / 2 on 0.4 % (cfg 3, 30 k) to 2 % (cfg 1) of the rows.  Those
# rows are the only ones a HIP error beyond the bar may be explained by, and they may be at most this fraction of the non-zero rows;
# above it the probe, not the kernel, is wrong (a random incoming gradient over all pixels puts ~40 % of the rows there).
OWN_ROW_ORACLE_FRAC = 5e-2
FLT_MIN = float(np.finfo(np.float32).tiny)


def own_row_err(a, truth):
    """(per-row max |a - truth| / max |truth row|, max |truth row|).  A zero truth row gives 0 if `a`'s row is exactly zero, else inf."""
    t = np.asarray(truth, np.float64)
    t = t.reshape(t.shape[0], -1)
    a = np.asarray(a, np.float64).reshape(t.shape)
    mag = np.abs(t).max(1) if t.size else np.zeros(t.shape[0])
    d = np.abs(a - t).max(1) if t.size else np.zeros(t.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(mag > 0, d / np.where(mag > 0, mag, 1.0), np.where(d > 0, np.inf, 0.0))
    return e, mag


def compare_grads_own_row(hg, og32, og64, rtol=OWN_ROW_RTOL, keys=None, rows=None, what=""):
    """Every checked Gaussian row of HIP within `rtol` of its OWN largest magnitude in the fp64 oracle: max|hip - o64| <= rtol x
    max|o64 row|, no percentile, no tensor-max floor.  Only meaningful under an incoming gradient whose per-pixel terms cannot cancel on
    the checked tensors (colour_probe, uniform_colour_probe, disjoint_pixel_probe); `keys` = those tensors, `rows` = optional bool [P]
    restricting the rows (default all).

    rtol = OWN_ROW_RTOL = 2e-3, calibrated from the fp32 oracle's own row-own error against fp64 under these probes.
    A row beyond the bar is EXPLAINED by the rule of compare_grads: the fp32 oracle is off fp64 by more than rtol / 2 on that row and HIP
    is no further from fp64 than twice that (the ill-conditioned rows of the per-Gaussian chain).  Every row whose fp64 truth is
    exactly zero must be exactly zero in HIP, every row whose truth is a normal float32 must be non-zero in HIP (dropped or unwritten
    rows); neither can be explained.
    Before HIP is looked at, the fp32 oracle must pass the same checks at rtol / 2 on all but OWN_ROW_ORACLE_FRAC of the non-zero rows:
    if it does not, the probe lets terms cancel and the assert says so.
    Returns per tensor: rows (checked), nonzero, beyond_bar, explained, oracle_beyond_half_bar, worst_hip, worst_oracle (row-own
    errors vs fp64 of HIP and of the fp32 oracle over the non-zero rows)."""
    keys = list(og64) if keys is None else list(keys)
    stats = {}
    for k in keys:
        e_h, mag = own_row_err(hg[k], og64[k])
        e_o, _ = own_row_err(og32[k], og64[k])
        sel = np.ones(mag.shape, bool) if rows is None else np.asarray(rows, bool)
        zero, normal = sel & (mag == 0), sel & (mag >= FLT_MIN)
        nz = sel & (mag > 0)
        o_rows = np.asarray(og32[k], np.float64).reshape(mag.size, -1)
        h_rows = np.asarray(hg[k], np.float64).reshape(mag.size, -1)
        # ---- the probe first: the fp32 oracle at rtol / 2 ----
        o_zero_bad = zero & (np.abs(o_rows).max(1) > 0) if o_rows.size else zero & False
        o_lost = normal & (np.abs(o_rows).max(1) == 0) if o_rows.size else normal & False
        o_out = nz & (e_o > rtol / 2)
        n_nz = int(nz.sum())
        assert not o_zero_bad.any() and not o_lost.any(), (
            f"{what} {k}: the fp32 oracle's zero pattern differs from fp64 ({int(o_zero_bad.sum())} rows non-zero, {int(o_lost.sum())} "
            "rows lost): the probe is wrong")
        assert o_out.sum() <= OWN_ROW_ORACLE_FRAC * n_nz, (
            f"{what} {k}: the fp32 oracle is off fp64 by more than {rtol / 2:.0e} of its own row on {int(o_out.sum())} of {n_nz} "
            f"rows (allowed {OWN_ROW_ORACLE_FRAC:.0e} of them): the probe lets terms cancel; worst rows "
            f"{_describe_own(np.nonzero(o_out)[0], e_o, e_h)}")
        # ---- HIP ----
        h_zero_bad = zero & (np.abs(h_rows).max(1) > 0) if h_rows.size else zero & False
        h_lost = normal & (np.abs(h_rows).max(1) == 0) if h_rows.size else normal & False
        assert not h_zero_bad.any(), (f"{what} {k}: {int(h_zero_bad.sum())} rows are non-zero in HIP where the fp64 truth is exactly "
                                      f"zero; rows {np.nonzero(h_zero_bad)[0][:8].tolist()}")
        assert not h_lost.any(), (f"{what} {k}: {int(h_lost.sum())} rows are exactly zero in HIP where the fp64 truth is not (dropped or "
                                  f"unwritten); rows {_describe_own(np.nonzero(h_lost)[0], e_h, e_o)}")
        out = nz & (e_h > rtol)
        expl = out & (e_o > rtol / 2) & (e_h <= 2 * e_o)
        unexp = out & ~expl
        stats[k] = dict(rows=int(sel.sum()), nonzero=n_nz, beyond_bar=int(out.sum()), explained=int(expl.sum()),
                        oracle_beyond_half_bar=int(o_out.sum()), worst_hip=float(e_h[nz].max()) if n_nz else 0.0,
                        worst_oracle=float(e_o[nz].max()) if n_nz else 0.0,
                        worst_hip_unexplained_excluded=float(e_h[nz & ~expl].max()) if (nz & ~expl).any() else 0.0)
        assert not unexp.any(), (
            f"{what} {k}: {int(unexp.sum())} of {n_nz} rows are off the fp64 oracle by more than {rtol:.0e} of their OWN magnitude and "
            "are not explained (explained = fp32 oracle off fp64 by > rtol / 2 on the row AND hip no further from fp64 than 2 x that); "
            f"worst rows {_describe_own(np.nonzero(unexp)[0], e_h, e_o)}")
    return stats


def _describe_own(idx, e, e_other, limit=5):
    order = idx[np.argsort(-e[idx])][:limit]
    return [dict(row=int(i), err=float(e[i]), other_vs_fp64=float(e_other[i])) for i in order]


def colour_probe(cam, seed):
    """Incoming gradient (dL/dcolor, dL/ddepth) = (|N(0, 1)|, 0).  Every colour gradient is then sum(alpha T dL) >= 0 over pixels, and
    every SH coefficient's gradient basis_k(dir) x that sum (zero on clamped channels): no term of a row can cancel another.  Checks
    `sh` (any degree) or `colors` (colors_precomp); holds with any background (bg only enters dL/dalpha)."""
    rng = np.random.default_rng(seed)
    return (np.abs(rng.normal(size=(3, cam.H, cam.W))).astype(np.float32), np.zeros((1, cam.H, cam.W), np.float32))


def uniform_colour_probe(cam, P, seed, value=0.5):
    """(colors_precomp [P, 3] = value everywhere, incoming gradient).  With bg = 0 the blend's accumulated colour behind an entry is a
    convex combination of `value` and 0, so col - accum_rec >= 0 and, with the positive colour gradient of colour_probe, dL/dalpha >= 0:
    the `colors` and `opacity` gradients have no negative term.  The caller renders with bg = 0."""
    return np.full((P, 3), value, np.float32), colour_probe(cam, seed)


def disjoint_pixels(o, hit, seed, exclude=None, tries=8):
    """One greedy selection of pixels, from the oracle forward's context, such that no Gaussian that can receive a term at a chosen
    pixel belongs to another chosen pixel.  A pixel's backward walks the first n_contrib entries of its tile's list and gives a term to
    those whose alpha reaches 1/255 (the blend's cut-off), plus the depth term to its hit Gaussian (hit = hit_depth [H, W]); the set
    taken here is those entries with alpha >= 1/510 (a margin, so that no rounding of alpha can add a term outside it; without the
    gate, which only removes terms) and the hit Gaussian.  `exclude` (bool [H, W]): pixels never chosen (the flipped ones).  Tiles in
    random order; in each up to `tries` random pixels, the first whose set is still free is taken.
    Returns (pixels bool [H, W], covered bool [P] = the union of the sets)."""
    H, W, gx = o.H, o.W, o.gx
    rng = np.random.default_rng(seed)
    rg, pl, nc = o.ctx("ranges"), o.ctx("point_list").astype(np.int64), o.ctx("n_contrib").astype(np.int64)
    m2, co = o.ctx("means2D").astype(np.float64), o.ctx("conic_opacity").astype(np.float64)
    hit = np.asarray(hit).reshape(H, W).astype(np.int64)
    excl = np.zeros((H, W), bool) if exclude is None else np.asarray(exclude, bool).reshape(H, W)
    used = np.zeros(o.P, bool)
    pick = np.zeros((H, W), bool)
    for t in rng.permutation(o.ctx("tile_indices")):
        r0 = int(rg[t, 0])
        ty, tx = divmod(int(t), gx)
        y0, x0 = 16 * ty, 16 * tx
        n, h = nc[y0:y0 + 16, x0:x0 + 16], hit[y0:y0 + 16, x0:x0 + 16]
        cand = np.argwhere((n > 0) & ~excl[y0:y0 + 16, x0:x0 + 16])
        for yy, xx in cand[rng.permutation(len(cand))[:tries]]:
            g = pl[r0:r0 + n[yy, xx]]
            dx, dy = m2[g, 0] - (x0 + xx), m2[g, 1] - (y0 + yy)
            c = co[g]
            power = -0.5 * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
            s = g[(power <= 1e-6) & (np.minimum(0.99, c[:, 3] * np.exp(np.minimum(power, 0.0))) >= 0.5 / 255.0)]
            if h[yy, xx] >= 0:
                s = np.append(s, h[yy, xx])
            if s.size and not used[s].any():
                used[s] = True
                pick[y0 + yy, x0 + xx] = True
                break
    return pick, used


def disjoint_pixel_probe(o, hit, seed, rounds, exclude=None):
    """`rounds` incoming gradients, each with random-sign colour and depth gradients on one disjoint_pixels() selection (its own seed)
    and zero elsewhere.  Every Gaussian receives at most ONE pixel's term (its blend term and, for the pixel's hit Gaussian, the depth
    term), so nothing cancels across pixels and all five tensors (means3D, sh, opacity, scales, rotations) can be held to their own
    rows.  This is the only probe that covers the depth-hit path (colour_probe and uniform_colour_probe have a zero depth gradient).
    Returns a list of dicts: dL (colour, depth), pixels bool [H, W], covered bool [P] (rows that may receive a term)."""
    out = []
    for r in range(rounds):
        pix, cov = disjoint_pixels(o, hit, seed * 1000 + r, exclude)
        rng = np.random.default_rng(seed * 1000 + r)
        dC = (rng.normal(size=(3, o.H, o.W)) * pix[None]).astype(np.float32)
        dD = (rng.normal(size=(1, o.H, o.W)) * pix[None]).astype(np.float32)
        out.append(dict(dL=(dC, dD), pixels=pix, covered=cov))
    return out
