"""Times the mesh depth render and Depth L1 (dqo_eval.mesh_render_depth, depth_l1; csrc/map_meshrender.hip, map_eval.hip) on the mesh
of tools/profile_tsdf.py's volume — a 256^3 grid of 2 cm voxels, a wall with a sphere in front integrated from `--frames` poses —
rendered into `--views` views of 1200 x 680 on tools/profile_mesh_eval.py's arc of poses, and compared with the scene's own ray-cast
depth.  Device events around the calls, warmed up; the library's per-launch timers give the three launches of the render and the two of
the comparison.  Yardsticks, in the same run on the same GPU:
    clear, resolve   the bytes they must move at the HBM peak (8.0 TB/s): 8 per pixel written; 8 read and 4 (8 with face_index) written.
    rasterise        no floor is claimed: the pairs, the pixels hit and the pairs the whole wave walked are printed beside the time.
    a second mesh    two wall-sized triangles in front of the scene (the ground-truth kind of face), alone and added to the mesh: the
                     whole-wave path's time, and a near surface that hides the rest.
    the clip         dqo_eval.mesh_render_depth_clip on the volume's mesh, run in turns with the plain entry in the same process: the
                     plain entry is the yardstick, and a mesh that hardly crosses the near planes runs the same statements per pair;
                     then a floor of two triangles that every camera stands on (each pair crosses its near plane), which the plain
                     entry drops and the clip rasterises by the whole wave.
    the face cull    dqo_eval.mesh_cull_visible (the clipped render with face_index, then dqo_mesh_cull_faces) on the volume's mesh and
                     on the mesh behind the two triangles, where two faces win most pixels; the pixels launch against the bytes it
                     must read at the HBM peak: 4 per pixel, 12 with the frames' depth.

`--lib` loads another build of the library — that is how the variants of profiles/mesh_render.txt were measured: map_meshrender.hip
compiled with MR_SMALL_MAX set to 16 and to 256, and once with the atomic filter (a plain load of the pixel's key in front of the min
atomic of mr_pixel, the atomic skipped where the stored key is not above the new one), which the library does not have and keeps no
switch for.

    python tools/profile_mesh_render.py [--n 256] [--frames 8] [--views 100] [--reps 10] [--lib PATH --label TEXT] >> profiles/mesh_render.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from profile_mesh_eval import spread
from profile_tsdf import HBM_PEAK, WARMUP, frame


def launches(N, run, names, reps=5):
    N.profile_enable(True)
    N.profile_collect()
    for _ in range(reps):
        run()
    prof = N.profile_collect()
    N.profile_enable(False)
    return {k: prof[k][0] / max(1, prof[k][1]) for k in names if k in prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="the library as built")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_mesh_render: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
    if a.lib is not None:
        N.LIB_PATH = os.path.abspath(a.lib)
    import dqo_eval
    dev = torch.device("cuda")
    n, L = a.n, 5.12 / a.n
    W, H, fx, fy, cx, cy = 1200, 680, 600.0, 600.0, 599.5, 339.5
    K = (fx, fy, cx, cy)
    vol = dqo_eval.TsdfVolume((-2.56, -2.56, 0.0), L, (n, n, n), 3 * L, dev)
    for k in range(a.frames):
        yaw, pos = -12.0 + 24.0 * k / max(1, a.frames - 1), (-0.6 + 1.2 * k / max(1, a.frames - 1), 0.0, 0.2)
        d, c, m = frame(W, H, fx, fy, cx, cy, yaw, pos, dev)
        vol.integrate(d, c, K, m, depth_trunc=30.0)
    mesh = vol.extract(6_000_000, 12_000_000)
    cnt = vol.counts()
    nv = a.views
    sensor = torch.empty((nv, H, W), dtype=torch.float32, device=dev)
    w2c = torch.empty((nv, 4, 4), dtype=torch.float32, device=dev)
    for k in range(nv):
        t = k / max(1, nv - 1)
        sensor[k], _, w2c[k] = frame(W, H, fx, fy, cx, cy, -20.0 + 40.0 * t, (-1.0 + 2.0 * t, 0.0, 0.2), dev)
    pixels = nv * H * W
    print(f"== {a.label} ==")
    print(f"device: {torch.cuda.get_device_name(0)}   grid {n}^3, {a.frames} poses; extract: " + "  ".join(f"{k}={v}" for k, v in cnt.items()))
    print(f"views: {nv} of {W} x {H} = {pixels} pixels; keys {pixels * 8 / 1e6:.1f} MB; pairs F x K = {cnt['faces'] * nv}")
    names = ("mesh_render_clear_kernel", "mesh_render_raster_kernel", "mesh_render_resolve_kernel")
    # two wall-sized triangles across the arc of cameras, nearer than the scene
    wall = dict(vertices=torch.tensor([[-6.0, -4.0, 0.9], [6.0, -4.0, 0.9], [6.0, 4.0, 0.9], [-6.0, 4.0, 0.9]], device=dev),
                faces=torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev))
    V, F = cnt["vertices"], cnt["faces"]
    both = dict(vertices=torch.cat([mesh["vertices"][:V], wall["vertices"]]), faces=torch.cat([mesh["faces"][:F], wall["faces"] + V]))
    outs = {}
    for name, m, fi in (("the volume's mesh", mesh, False), ("the volume's mesh, with face_index", mesh, True), ("two wall-sized triangles", wall, False),
                        ("the mesh behind the two triangles", both, False)):
        out = outs.setdefault(name, {})
        run = lambda m=m, fi=fi, out=out: dqo_eval.mesh_render_depth(m, w2c, K, W, H, want_face_index=fi, out=out)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, a.reps)
        print(f"mesh_render_depth, {name} (three launches): median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps}")
        print("  header: " + "  ".join(f"{k}={v}" for k, v in dqo_eval.mesh_counts(run()).items()))
        per = launches(N, run, names)
        print("  " + "  ".join(f"{k}: {v:.3f} ms" for k, v in per.items()) + "  (per launch, serialised by the timers)")
        wr = 12 if fi else 8
        print(f"  at {HBM_PEAK / 1e12:.1f} TB/s: clear {pixels * 8 / HBM_PEAK * 1e3:.3f} ms, resolve {pixels * (8 + wr - 4) / HBM_PEAK * 1e3:.3f} ms")
    # the clip beside the plain entry: in turns, so that both see the same clocks
    cnames = ("mesh_render_clear_kernel", "mesh_render_raster_clip_kernel", "mesh_render_resolve_kernel")
    plain_out, clip_out = {}, {}
    run_plain = lambda: dqo_eval.mesh_render_depth(mesh, w2c, K, W, H, out=plain_out)
    run_clip = lambda: dqo_eval.mesh_render_depth_clip(mesh, w2c, K, W, H, out=clip_out)
    for _ in range(WARMUP):
        run_plain(), run_clip()
    for turn in range(3):
        for name, run, nm in (("mesh_render_depth", run_plain, names), ("mesh_render_depth_clip", run_clip, cnames)):
            med, lo, hi = spread(run, a.reps)
            per = launches(N, run, nm)
            print(f"turn {turn}: {name}, the volume's mesh: median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps};  rasterise launch {per[nm[1]]:.3f} ms")
    print("  header, clipped: " + "  ".join(f"{k}={v}" for k, v in dqo_eval.mesh_counts(run_clip()).items()))
    print("  same depth bytes as the plain entry: " + str(bool(torch.equal(plain_out["depth"], clip_out["depth"]))))
    floor = dict(vertices=torch.tensor([[-6.0, 0.8, -6.0], [6.0, 0.8, -6.0], [6.0, 0.8, 6.0], [-6.0, 0.8, 6.0]], device=dev),
                 faces=torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev))
    for name, fn, nm in (("mesh_render_depth", dqo_eval.mesh_render_depth, names), ("mesh_render_depth_clip", dqo_eval.mesh_render_depth_clip, cnames)):
        out = {}
        run = lambda fn=fn, out=out: fn(floor, w2c, K, W, H, out=out)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, a.reps)
        per = launches(N, run, nm)
        print(f"{name}, a floor of two triangles under every camera: median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps};  rasterise launch {per[nm[1]]:.3f} ms")
        print("  header: " + "  ".join(f"{k}={v}" for k, v in dqo_eval.mesh_counts(run()).items()))
    # the face cull
    fnames = ("mesh_cull_finit_kernel", "mesh_cull_pixels_kernel", "mesh_cull_fpix_kernel", "mesh_cull_vcount_kernel", "mesh_cull_vscatter_kernel",
              "mesh_cull_fscatter_kernel")
    for name, m, dep in (("the volume's mesh", mesh, None), ("the volume's mesh, against the ray-cast depth", mesh, sensor),
                         ("the mesh behind the two triangles", both, None)):
        run = lambda m=m, dep=dep: dqo_eval.mesh_cull_visible(m, w2c, K, W, H, depth=dep, eps=0.05)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, a.reps)
        print(f"mesh_cull_visible, {name} (the clipped render, then six launches): median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps}")
        print("  header: " + "  ".join(f"{k}={v}" for k, v in dqo_eval.mesh_counts(run()).items()))
        per = launches(N, run, fnames)
        print("  " + "  ".join(f"{k}: {v:.3f} ms" for k, v in per.items()))
        print(f"  pixels launch at {HBM_PEAK / 1e12:.1f} TB/s: {pixels * (4 if dep is None else 12) / HBM_PEAK * 1e3:.3f} ms")
    rendered = outs["the volume's mesh"]["depth"]
    run = lambda: dqo_eval.depth_l1(sensor, rendered, depth_trunc=30.0)
    for _ in range(WARMUP):
        run()
    med, lo, hi = spread(run, a.reps)
    print(f"depth_l1, the ray-cast depth against the mesh's render (two launches): median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps}")
    per = launches(N, run, ("depth_l1_partial_kernel", "depth_l1_rows_kernel"))
    print("  " + "  ".join(f"{k}: {v:.3f} ms" for k, v in per.items()) + f"  (two stacks once at {HBM_PEAK / 1e12:.1f} TB/s: {pixels * 8 / HBM_PEAK * 1e3:.3f} ms)")
    print("  row of the set: " + "  ".join(f"{k}={v:.6g}" for k, v in dqo_eval.depth_l1_dict(run())["mean"].items()))


if __name__ == "__main__":
    main()
