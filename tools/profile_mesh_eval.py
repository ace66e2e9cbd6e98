"""Times the mesh evaluation (dqo_eval.mesh_cull, sample_surface_counted, eval_mesh; csrc/map_meshcull.hip, map_meshsample.hip) on the
mesh of tools/profile_tsdf.py's volume — a 256^3 grid of 2 cm voxels, a wall with a sphere in front integrated from `--frames` poses —
culled to `--views` views of 1200 x 680 whose depth maps are the scene's own ray casts.  Device events around the calls, warmed up;
the library's per-launch timers give the cull's split.  Yardsticks, in the same run on the same GPU:
    cull      a torch restatement of the visibility rule — batched matmul, gather, reduce over views, `--chunk` views at a time so that
              its intermediates fit — which is what a user would write without the operator.  It covers the views launch only (no
              compaction), so the ratio is given against that launch and against the whole call; the two counts are compared vertex by
              vertex (a matmul contracts and reorders: a vertex within rounding of a test may differ).
              Least time of the views launch: V x K pairs, one gathered 4-byte pixel each (a 64-byte line when neighbours do not share
              one) and about 40 float operations; the depth maps are read at least once: K x H x W x 4 bytes at the HBM peak (8.0 TB/s).
    sampler   sample_surface (host counts) on the sliced mesh, alternated with sample_surface_counted on the capacities: the difference
              beside the spread of either; the counted grids are sized by the capacity, not the count.
    chain     eval_mesh with and without views against its parts.

    python tools/profile_mesh_eval.py [--n 256] [--frames 8] [--views 100] [--reps 20] > profiles/mesh_eval.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from profile_tsdf import HBM_PEAK, WARMUP, frame


def torch_views(p, w2c, K, W, H, depth, eps, chunk):
    """views(v) of dqo_mesh_cull's rule in torch: int32 [V].  p [V,3], w2c [n,4,4], depth [n,H,W] or None."""
    fx, fy, cx, cy = K
    ph = torch.cat([p, torch.ones_like(p[:, :1])], 1).t().contiguous()  # [4,V]
    views = torch.zeros((p.shape[0],), dtype=torch.int32, device=p.device)
    for a in range(0, w2c.shape[0], chunk):
        pc = torch.matmul(w2c[a:a + chunk, :3, :], ph)  # [k,3,V]
        z = pc[:, 2]
        uf, vf = pc[:, 0] * fx / z + cx + 0.5, pc[:, 1] * fy / z + cy + 0.5
        seen = (z > 0) & (uf >= 0.0001) & (uf < W - 0.0001) & (vf >= 0.0001) & (vf < H - 0.0001)
        if depth is not None:
            u, v = torch.where(seen, uf, 0).long(), torch.where(seen, vf, 0).long()
            d = torch.gather(depth[a:a + chunk].reshape(pc.shape[0], -1), 1, v * W + u)
            seen &= (d > 0) & (z <= d + eps)
        views += seen.sum(0, dtype=torch.int32)
    return views


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--samples", type=int, default=1000000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_mesh_eval: needs a GPU (there is nothing to time without one)")
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
    nv = a.views
    depth = torch.empty((nv, H, W), dtype=torch.float32, device=dev)
    w2c = torch.empty((nv, 4, 4), dtype=torch.float32, device=dev)
    for k in range(nv):  # the poses of the integration's arc, and beyond it on both sides
        t = k / max(1, nv - 1)
        depth[k], _, w2c[k] = frame(W, H, fx, fy, cx, cy, -20.0 + 40.0 * t, (-1.0 + 2.0 * t, 0.0, 0.2), dev)
    eps = 0.03
    print(f"device: {torch.cuda.get_device_name(0)}   grid {n}^3, {a.frames} poses, capacities {cap_v} vertices / {cap_f} faces")
    print("extract: " + "  ".join(f"{k}={v}" for k, v in cnt.items()))
    print(f"views: {nv} of {W} x {H}, depth maps {depth.numel() * 4 / 1e6:.1f} MB; pairs V x K = {V * nv}")

    views_kw = dict(w2c=w2c, K=K, W=W, H=H, eps=eps)
    cases = (("frustum only", dict(views_kw), False), ("with depth", dict(views_kw, depth=depth), False),
             ("with depth and vertex_views", dict(views_kw, depth=depth), True))
    floor = depth.numel() * 4 / HBM_PEAK * 1e3
    launch_ms = {}
    for name, kw, want in cases:
        run = lambda kw=kw, want=want: dqo_eval.mesh_cull(mesh, want_views=want, **kw)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, a.reps)
        print(f"mesh_cull, {name} (six launches): median {med:.3f} ms, least {lo:.3f}, most {hi:.3f} of {a.reps}")
        print("  out: " + "  ".join(f"{k}={v}" for k, v in dqo_eval.mesh_counts(run()).items()))
        N.profile_enable(True)
        N.profile_collect()
        for _ in range(5):
            run()
        prof = N.profile_collect()
        N.profile_enable(False)
        for kn, (ms, calls) in prof.items():
            print(f"  {kn}: {ms / max(1, calls):.3f} ms per launch ({calls} launches, serialised by the timers)")
        launch_ms[name] = prof["mesh_cull_views_kernel"][0] / max(1, prof["mesh_cull_views_kernel"][1])
        if "depth" in kw:
            print(f"  the depth maps once at {HBM_PEAK / 1e12:.1f} TB/s: {floor:.4f} ms; the views launch is {launch_ms[name] / floor:.1f} x that")

    # the yardstick: the same rule in torch
    p = mesh["vertices"][:V]
    for name, dep in (("frustum only", None), ("with depth", depth)):
        run = lambda dep=dep: torch_views(p, w2c, K, W, H, dep, eps, a.chunk)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, max(3, a.reps // 4))
        out = dqo_eval.mesh_cull(mesh, want_views=True, depth=dep, **views_kw)
        ours = out["vertex_views"][:V]
        differ = int((run() != ours).sum().item())
        key = name if dep is None else "with depth and vertex_views"
        whole = spread(lambda dep=dep: dqo_eval.mesh_cull(mesh, want_views=True, depth=dep, **views_kw), a.reps)[0]
        print(f"torch restatement of the views pass, {name} ({a.chunk} views at a time): median {med:.3f} ms, least {lo:.3f}, most {hi:.3f}; "
              f"{differ} of {V} vertices count differently")
        print(f"  against it: the whole mesh_cull with vertex_views {whole:.3f} ms = {med / whole:.1f} x faster; its views launch "
              f"{launch_ms.get(key, float('nan')):.3f} ms")

    # the sampler: host counts against device counts, alternated
    count = a.samples
    sv, sf = mesh["vertices"][:V], mesh["faces"][:F]
    host = lambda: dqo_eval.sample_surface(sv, sf, count, seed=1)
    counted = lambda: dqo_eval.sample_surface_counted(mesh, count, seed=1)
    for _ in range(WARMUP):
        host(), counted()
    same = torch.equal(host()["points"].view(torch.int32), counted()["points"].view(torch.int32))
    rows = [(spread(host, a.reps), spread(counted, a.reps)) for _ in range(3)]
    for k, (h, c) in enumerate(rows):
        print(f"sampler, round {k}: sample_surface on the slices median {h[0]:.3f} ms (least {h[1]:.3f}, most {h[2]:.3f}); sample_surface_counted on "
              f"capacities of {cap_f} faces median {c[0]:.3f} ms (least {c[1]:.3f}, most {c[2]:.3f}); points equal: {same}")
    tight = dict(vertices=sv.clone(), faces=sf.clone(), header=mesh["header"][:2].clone())
    c2 = spread(lambda: dqo_eval.sample_surface_counted(tight, count, seed=1), a.reps)
    print(f"sampler: sample_surface_counted with capacities equal to the counts ({F} faces): median {c2[0]:.3f} ms (least {c2[1]:.3f}, most {c2[2]:.3f})")

    # the chain
    gt = dict(vertices=sv.clone(), faces=sf.clone())
    for name, vw in (("no views", None), (f"{nv} views with depth", dict(views_kw, depth=depth))):
        run = lambda vw=vw: dqo_eval.eval_mesh(mesh, gt, count, seed=1, views=vw)
        for _ in range(WARMUP):
            run()
        med, lo, hi = spread(run, max(5, a.reps // 2))
        row = dqo_eval.eval_pcd_dict(run())
        print(f"eval_mesh, {name}, {count} samples a side: median {med:.3f} ms, least {lo:.3f}, most {hi:.3f}")
        print("  row: " + "  ".join(f"{k}={v:.6g}" for k, v in row.items()))


if __name__ == "__main__":
    main()
