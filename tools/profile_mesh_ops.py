"""Times the mesh clean-up (dqo_eval.mesh_components, mesh_simplify, mesh_smooth, mesh_normals; csrc/map_meshops.hip) on the mesh of
tools/profile_tsdf.py's volume — a 256^3 grid of 2 cm voxels, a wall with a sphere in front integrated from `--frames` poses — and the
extraction of that mesh for scale.  Device events around the calls, warmed up; the library's own per-launch timers give the split of
each operator's launches.  Next to each measurement stands the least time its compulsory memory traffic allows at the HBM peak
(8.0 TB/s), from the counts the run itself reports:
    components  faces read five times (prelink, hook, label, fcount, fscatter: 12 bytes each) and written once, vertices read and written once
                (24 bytes with colours each way), about 40 bytes of workspace a vertex and 15 a face
    simplify    vertices read by the cell pass (12 bytes, and 12 per probed occupant), again with colours by the average (24), faces read once
                (12), their rotated triples written and read by the table, keep and scatter passes (12 each time), the two tables
                cleared and probed (8 bytes a slot, two slots an entry), about 36 bytes of workspace a vertex and 12 a face; at
                voxel_size = 2 x and 4 x the voxel length, with the counts in and out
    smooth      per step and vertex: 24 bytes read and written, its neighbour list (4 bytes an entry) and a gathered 24 bytes a neighbour
                (from cache where neighbours share lines); the adjacency build: 12 bytes a face read twice, 24 written, read and rewritten
    normals     the adjacency build (12 bytes a face twice, 12 written, read and rewritten), then 12 bytes a vertex written and, per
                incident face, 4 + 12 + 36 gathered

    python tools/profile_mesh_ops.py [--n 256] [--frames 8] [--reps 20] > profiles/mesh_ops.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from profile_tsdf import HBM_PEAK, WARMUP, frame, timed


def split(N, f, label):
    """The per-launch split of f() by the library's timers."""
    N.profile_enable(True)
    N.profile_collect()
    for _ in range(5):
        f()
    prof = N.profile_collect()
    N.profile_enable(False)
    for name, (ms, calls) in prof.items():
        print(f"  {label} {name}: {ms / max(1, calls):.3f} ms per launch ({calls} launches, serialised by the timers)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_mesh_ops: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
    import dqo_eval
    dev = torch.device("cuda")
    n, L = a.n, 5.12 / a.n
    W, H, fx, fy, cx, cy = 1200, 680, 600.0, 600.0, 599.5, 339.5
    vol = dqo_eval.TsdfVolume((-2.56, -2.56, 0.0), L, (n, n, n), 3 * L, dev)
    for k in range(a.frames):
        yaw, pos = -12.0 + 24.0 * k / max(1, a.frames - 1), (-0.6 + 1.2 * k / max(1, a.frames - 1), 0.0, 0.2)
        d, c, m = frame(W, H, fx, fy, cx, cy, yaw, pos, dev)
        vol.integrate(d, c, (fx, fy, cx, cy), m, depth_trunc=30.0)
    cap_v, cap_f = 6_000_000, 12_000_000
    raw = vol.extract(cap_v, cap_f)
    cnt = vol.counts()
    V, F = cnt["vertices"], cnt["faces"]
    print(f"device: {torch.cuda.get_device_name(0)}   grid {n}^3, {a.frames} poses, capacities {cap_v} vertices / {cap_f} faces")
    print("extract: " + "  ".join(f"{k}={v}" for k, v in cnt.items()))
    for _ in range(WARMUP):
        vol.extract(cap_v, cap_f)
    med_x, lo_x = timed(lambda: vol.extract(cap_v, cap_f), a.reps)
    print(f"TsdfVolume.extract (four launches, for scale): median {med_x:.3f} ms, least {lo_x:.3f} ms of {a.reps}")

    def report(name, f, traffic, launches):
        for _ in range(WARMUP):
            f()
        med, lo = timed(f, a.reps)
        print(f"{name} ({launches} launches): median {med:.3f} ms, least {lo:.3f} ms of {a.reps}; {med / med_x:.2f} x the extract")
        print(f"traffic: about {traffic} bytes; at {HBM_PEAK / 1e12:.1f} TB/s: {traffic / HBM_PEAK * 1e3:.4f} ms")
        split(N, f, name.split("(")[0].strip())

    report("mesh_components(largest_only)", lambda: dqo_eval.mesh_components(raw, largest_only=True), F * (5 * 12 + 12 + 15) + V * (48 + 40), 11)
    clean = dqo_eval.mesh_components(raw, largest_only=True)
    cc = dqo_eval.mesh_counts(clean)
    print("components: " + "  ".join(f"{k}={v}" for k, v in cc.items()))
    V2, F2 = cc["vertices"], cc["faces"]
    for k in (2, 4):  # (before the smoothing, which moves `clean` in place)
        run = lambda k=k: dqo_eval.mesh_simplify(clean, k * L, origin=vol.origin)
        report(f"mesh_simplify(voxel_size = {k} x the voxel length)", run, V2 * (12 + 12 + 24 + 16 + 36) + F2 * (12 + 4 * 12 + 16 + 12), 12)
        sc = dqo_eval.mesh_counts(run())
        print(f"simplify {k} x: in vertices={V2} faces={F2}  out " + "  ".join(f"{n}={v}" for n, v in sc.items()))
    build = F2 * (24 + 24 * 3)
    step = V2 * (48 + 6 * 4 + 6 * 24 + 48)  # (about six neighbours a vertex)
    report("mesh_smooth(1 step, positions and colours)", lambda: dqo_eval.mesh_smooth(clean, 1, lam=0.5), build + step, 7)
    report("mesh_smooth(10 steps: mesh_smooth_iter 10, mesh_smooth_lambda 0.5)", lambda: dqo_eval.mesh_smooth(clean, 10, lam=0.5), build + 10 * step, 15)
    report("mesh_normals", lambda: dqo_eval.mesh_normals(clean), F2 * (24 + 12 * 3) + V2 * (12 + 6 * 52), 6)


if __name__ == "__main__":
    main()
