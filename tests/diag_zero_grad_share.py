"""Share of the in-view Gaussians of a BASELINE config that provably get a zero gradient in the bench's per-object job: the rows the
exact sparse Adam could leave alone.  CPU only: the C++ oracle renders the perturbed target (the object masks) and the
gated forward the counts are taken from (which is why it lives beside the tests: tools/ runs on the product alone).
    python tests/diag_zero_grad_share.py [--cfg 3] [--P N] [--view room|all]

Three nested criteria for "no gradient" among the rows with radii > 0 that are outside the attach set (opacity >= 0.9):
  no_instance  the Gaussian is in no tile list that has a pixel of its own object (an upper bound on the fused path's `cnt == 0`, whose
               culling also drops tiles the footprint misses)
  no_pair      no pixel blends it: at every pixel of its tiles the gate, alpha < 1/255 or the pixel's early exit came first (the
               oracle's pair masks).  This is the exact condition for a zero gradient row and what `rec_valid` can see at best.
  n_touched=0  the forward's n_touched counter is zero.  NOT a proof of a zero gradient: the counter only counts pixels whose transmittance
               behind the Gaussian is still above 0.5 (forward.cu:833-835), so it overstates the share; printed for comparison only.
"""
import argparse
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "dqo-map_amd")]


def oracle_settings(ol, cam):
    # the normal threshold of dqo_harness.mapping.make_settings / bench.cpu_iteration
    return ol.RastSettings(cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, normal_threshold=float(np.cos(np.deg2rad(60.0))))


def forward(ol, cam, sc, omp=True, **kw):
    o = ol.OracleRasterizer(np.float32, omp=omp)
    r = o.forward(oracle_settings(ol, cam), sc["xyz"], sc["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                  shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"], **kw)
    return o, r


def oracle_pix_obj(ol, cam, full, seed, omp=True):
    """dqo_harness.mapping.perturbed_target's object masks from the oracle's render instead of the GPU's: the same perturbed copy (same
    generator, same draws), a pixel belongs to the object of the Gaussian that fixes its depth, -1 where nothing does."""
    P = full["xyz"].shape[0]
    rng = np.random.default_rng(seed)
    pert = dict(full)
    pert["xyz"] = (full["xyz"] + rng.normal(0, 0.004, full["xyz"].shape)).astype(np.float32)
    pert["shs"] = full["shs"].copy()
    pert["shs"][:, 0, :] += rng.normal(0, 0.15, (P, 3)).astype(np.float32)
    o, r = forward(ol, cam, pert, omp)
    hit = r.hit_depth[0]
    pix_obj = np.asarray(full["obj_id"], np.int32)[np.clip(hit, 0, None)]
    pix_obj[hit < 0] = -1
    o.free()
    return np.ascontiguousarray(pix_obj, np.int32)


def zero_grad_rows(ol, cam, sc, pix_obj, omp=True, masks=False):
    """Counts over the rows of `sc` for the gated forward at `cam` (pix_obj [H, W] int32).  Returns a dict of ints and shares; with
    masks=True also the bool [P] arrays behind them (in_view, attach, has_instance, has_pair, touched)."""
    obj = np.asarray(sc["obj_id"], np.int32)
    P = obj.shape[0]
    o, r = forward(ol, cam, sc, omp, pair_masks=True, gaussian_object=obj, pixel_object=pix_obj)
    ids = o.ctx("point_list").astype(np.int64)
    tiles = o.ctx("point_tile").astype(np.int64)
    blended = o.ctx("pair_mask").any(axis=1)
    o.free()
    gx, gy = (cam.W + 15) // 16, (cam.H + 15) // 16
    # object ids per tile: an instance can matter only where its tile holds a pixel of its own object
    pad = np.full((gy * 16, gx * 16), -1, np.int32)
    pad[:cam.H, :cam.W] = pix_obj
    per_tile = pad.reshape(gy, 16, gx, 16).transpose(0, 2, 1, 3).reshape(gy * gx, 256)
    n_obj = int(max(obj.max(), per_tile.max())) + 1
    tile_has = np.zeros((gy * gx, n_obj), bool)
    t_idx = np.repeat(np.arange(gy * gx), 256)
    flat = per_tile.reshape(-1)
    tile_has[t_idx[flat >= 0], flat[flat >= 0]] = True
    owned = tile_has[tiles, obj[ids]]
    has_instance = np.zeros(P, bool)
    has_instance[ids[owned]] = True
    has_pair = np.zeros(P, bool)
    has_pair[ids[blended]] = True
    in_view = r.radii > 0
    attach = np.clip(np.asarray(sc["opacity"], np.float32).reshape(-1), 1e-4, 1 - 1e-4) < 0.9  # bench.py: n_attach_full
    free = in_view & ~attach
    n_view = int(in_view.sum())
    out = dict(P=P, instances=int(ids.shape[0]), in_view=n_view, attach_in_view=int((in_view & attach).sum()),
               no_instance=int((free & ~has_instance).sum()), no_pair=int((free & ~has_pair).sum()),
               n_touched_zero=int((free & (r.n_touched == 0)).sum()),
               no_pair_with_attach=int((in_view & ~has_pair).sum()))
    for k in ("no_instance", "no_pair", "n_touched_zero", "no_pair_with_attach"):
        out["f_" + k] = round(out[k] / max(n_view, 1), 4)
    if masks:
        return out, dict(in_view=in_view, attach=attach, has_instance=has_instance, has_pair=has_pair, touched=r.n_touched > 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--P", type=int, default=None)
    ap.add_argument("--view", default="room", choices=("room", "all"))
    args = ap.parse_args()
    import bench
    from oracle import oracle_lib as ol
    ol.build()
    cam, full, cfgd, P = bench.build_scene(args)
    pix_obj = oracle_pix_obj(ol, cam, full, cfgd["seed"] + 7)  # bench.build_problem's target seed
    out = dict(cfg=args.cfg, view=args.view, **zero_grad_rows(ol, cam, full, pix_obj))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
