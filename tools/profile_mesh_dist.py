"""Times the exact point-to-triangle distance (dqo_eval.nearest_on_mesh, eval_pcd_surface, eval_mesh_surface; csrc/knn.hip,
map_eval.hip) on the mesh of tools/profile_tsdf.py's volume — a 256^3 grid of 2 cm voxels, a wall with a sphere in front integrated from
`--frames` poses.  Device events around the calls, warmed up; the library's per-launch timers give the search's split.  In one run on
one GPU:
    mesh        `--queries` points (a second draw of the mesh's own samples, moved by N(0, 1 cm): a reconstruction's samples) against
                the mesh by its device counts.
    walls       the same queries against that mesh plus two wall-sized triangles behind it (50 x its extent): one huge face loosens
                the box of the run it sorts into, and every query near the wall's plane has it as a candidate.
    centred     two triangles of that size centred on the mesh: as huge, but their centroids do not stretch the Morton grid — the
                contrast that tells the faces' own cost from the grid's.
    yardstick   dqo_nn1 (dqo_eval.nearest) of the same queries against as many sampled points of the mesh: the search whose walk the
                face search shares, with a 16-byte candidate and three subtractions where a face has 48 bytes and the region walk.
    chain       eval_mesh (nearest sample) and eval_mesh_surface (nearest face) without views, `--samples` a side.
    floor       a mesh against ITSELF: its own samples lie on it, so the surface form's accuracy is rounding, and the sampled form's is
                the noise floor its numbers carry — beside the estimate 0.5 / sqrt(samples per square metre).

    python tools/profile_mesh_dist.py [--n 256] [--frames 8] [--queries 1000000] [--reps 10] > profiles/mesh_dist.txt
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from profile_tsdf import WARMUP, frame


def spread(f, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def timed(name, run, reps):
    for _ in range(WARMUP):
        run()
    med, lo, hi = spread(run, reps)
    print(f"{name}: median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {reps}")
    return med


def launches(run, N):
    N.profile_enable(True)
    N.profile_collect()
    for _ in range(3):
        run()
    prof = N.profile_collect()
    N.profile_enable(False)
    for kn, (ms, calls) in prof.items():
        print(f"  {kn}: {ms / max(1, calls):.3f} ms per launch ({calls} launches, serialised by the timers)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_mesh_dist: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
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
    cap_v, cap_f = 6_000_000, 12_000_000
    mesh = vol.extract(cap_v, cap_f)
    cnt = vol.counts()
    V, F = cnt["vertices"], cnt["faces"]
    sv, sf = mesh["vertices"][:V], mesh["faces"][:F]
    tri = sv[sf.long()]
    area = float(0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1).double().sum().item())
    print(f"device: {torch.cuda.get_device_name(0)}   grid {n}^3, {a.frames} poses, capacities {cap_v} vertices / {cap_f} faces")
    print("extract: " + "  ".join(f"{k}={v}" for k, v in cnt.items()) + f"   area {area:.2f} m^2")

    Q = a.queries
    torch.manual_seed(5)
    q = dqo_eval.sample_surface_counted(mesh, Q, seed=2)["points"].clone() + 0.01 * torch.randn((Q, 3), device=dev)
    ref = dqo_eval.sample_surface_counted(mesh, Q, seed=1)["points"].clone()

    run = lambda: dqo_eval.nearest_on_mesh(q, mesh)
    timed(f"nearest_on_mesh, {Q} queries against the mesh by its counts ({F} faces in a capacity of {cap_f})", run, a.reps)
    print("  header: " + "  ".join(f"{k}={v}" for k, v in zip(dqo_eval.MESH_NEAREST_HEADER, run()[3].cpu().tolist())))
    launches(run, N)
    tight = dict(vertices=sv.clone(), faces=sf.clone())
    run = lambda: dqo_eval.nearest_on_mesh(q, tight)
    t_mesh = timed(f"nearest_on_mesh, {Q} queries against the mesh in buffers of its own size ({F} faces)", run, a.reps)
    launches(run, N)
    d_mesh = run()[0].clone()

    lo, hi = sv.min(0).values, sv.max(0).values
    s, c = 50.0 * float((hi - lo).max().item()), (lo + hi) / 2
    z = float(hi[2].item()) + 0.5
    wall = torch.tensor([[-s, -s], [s, -s], [s, s], [-s, s]], device=dev) + c[:2]
    wall = torch.cat([wall, torch.full((4, 1), z, device=dev)], 1)
    walls = dict(vertices=torch.cat([sv, wall]).contiguous(),
                 faces=torch.cat([sf, torch.tensor([[V, V + 1, V + 2], [V, V + 2, V + 3]], dtype=torch.int32, device=dev)]).contiguous())
    run = lambda: dqo_eval.nearest_on_mesh(q, walls)
    t_walls = timed(f"nearest_on_mesh, the same queries against the mesh plus two triangles of {2 * s:.0f} m at z = {z:.2f}", run, a.reps)
    launches(run, N)
    d_walls = run()[0]
    print(f"  queries nearer to a wall triangle than to the mesh: {int((d_walls < d_mesh).sum().item())}; walls / mesh = {t_walls / t_mesh:.2f}")
    # the same two huge faces where they do not stretch the grid: equilateral, centred on the mesh, so their centroids are its centre
    ring = lambda phase: [[float(c[0]) + s * math.cos(phase + k * 2.0 * math.pi / 3.0), float(c[1]) + s * math.sin(phase + k * 2.0 * math.pi / 3.0),
                           float(c[2])] for k in range(3)]
    centred = dict(vertices=torch.cat([sv, torch.tensor(ring(0.0) + ring(1.0), device=dev)]).contiguous(),
                   faces=torch.cat([sf, torch.tensor([[V, V + 1, V + 2], [V + 3, V + 4, V + 5]], dtype=torch.int32, device=dev)]).contiguous())
    run = lambda: dqo_eval.nearest_on_mesh(q, centred)
    t_centred = timed(f"nearest_on_mesh, the same queries against the mesh plus two triangles of that size CENTRED on it (centroids at its centre)", run,
                      a.reps)
    print(f"  centred / mesh = {t_centred / t_mesh:.2f}, walls / centred = {t_walls / t_centred:.2f} (the share of the stretched grid)")

    run = lambda: dqo_eval.nearest(q, ref, want_idx=True)
    t_nn1 = timed(f"yardstick: dqo_nn1, {Q} queries against {Q} sampled points", run, a.reps)
    launches(run, N)
    print(f"  nearest_on_mesh / dqo_nn1 = {t_mesh / t_nn1:.2f} ({F} faces of 48 bytes against {Q} points of 16)")

    gt = dict(vertices=sv.clone(), faces=sf.clone())
    for name, fn in (("eval_mesh (nearest sample)", dqo_eval.eval_mesh), ("eval_mesh_surface (nearest face)", dqo_eval.eval_mesh_surface)):
        run = lambda fn=fn: fn(mesh, gt, a.samples, seed=1)
        timed(f"{name}, no views, {a.samples} samples a side", run, max(5, a.reps // 2))
        row = dqo_eval.eval_pcd_dict(run())
        print("  row (the mesh against itself): " + "  ".join(f"{k}={v:.6g}" for k, v in row.items()))
    sampled = dqo_eval.eval_mesh(mesh, gt, a.samples, seed=1).cpu().tolist()
    surface = dqo_eval.eval_mesh_surface(mesh, gt, a.samples, seed=1).cpu().tolist()
    rho = a.samples / area
    print(f"floor: sampled accuracy {sampled[0]:.4f} cm, surface accuracy {surface[0]:.6f} cm: the sampled form carries "
          f"{sampled[0] - surface[0]:.4f} cm; estimate 0.5 / sqrt({rho:.0f} samples per m^2) = {50.0 / rho ** 0.5:.4f} cm")
    print(f"       sampled completion {sampled[1]:.4f} cm, surface completion {surface[1]:.6f} cm")


if __name__ == "__main__":
    main()
