"""Times the TSDF volume (dqo_eval.TsdfVolume: dqo_tsdf_integrate, dqo_tsdf_extract, csrc/map_tsdf.hip) at the size of a room scan:
a 256^3 grid of 2 cm voxels and a 1200 x 680 frame of analytic depth and colour (a wall with a sphere in front), integrated from
`--frames` poses on an arc.  Device events around the calls, warmed up; the library's own per-launch timers give the split of the
extraction's four launches.  The least time the memory traffic allows, computed from the counts the run itself reports, is printed next
to each measurement:
    integrate   per touched voxel 20 bytes read (tsdf, weight, three colour planes) and 20 written, plus one gathered pixel of 16 bytes
                (an upper bound: neighbouring voxels share pixels); untouched voxels cost arithmetic only
    extract     flags: 8 bytes a voxel read (tsdf, weight; the other seven weights of a cube come from cache), 1 written; edges: 1 read,
                3 written; vertices: 4 read, 1 written, 24 written and about 32 read per vertex; faces: 1 read a voxel, 12 written a face
over the HBM peak (8.0 TB/s).

    python tools/profile_tsdf.py [--n 256] [--frames 8] [--reps 20] > profiles/tsdf.txt
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

import torch

HBM_PEAK = 8.0e12  # bytes / s
WARMUP = 3


def timed(f, reps):
    """Median and minimum of `reps` calls in ms, device events around each."""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def frame(W, H, fx, fy, cx, cy, yaw_deg, pos, dev):
    """(depth [H,W], color [3,H,W], w2c [4,4]) on the device: the wall z = 4.6 with a sphere of radius 0.8 at (0.2, 0, 3.2) in front."""
    y = math.radians(yaw_deg)
    R = torch.tensor([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]], dtype=torch.float64, device=dev)
    o = torch.tensor(pos, dtype=torch.float64, device=dev)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.stack([(u - cx) / fx, (v - cy) / fy, torch.ones_like(u)], -1)
    dw = dc @ R
    tp = (4.6 - o[2]) / dw[..., 2]
    oc = o - torch.tensor([0.2, 0.0, 3.2], dtype=torch.float64, device=dev)
    a, b, c = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - 0.8 ** 2
    disc = b * b - 4 * a * c
    ts = torch.where(disc > 0, (-b - disc.abs().sqrt()) / (2 * a), torch.zeros_like(a))
    depth = torch.where((ts > 0) & (ts < tp), ts, tp)
    color = torch.stack([0.5 + 0.5 * torch.sin(0.02 * u), 0.5 + 0.5 * torch.cos(0.03 * v), (u + v) / (W + H)])
    w2c = torch.eye(4, dtype=torch.float64, device=dev)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ o
    return depth.float().contiguous(), color.float().contiguous(), w2c.float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_tsdf: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
    import dqo_eval
    dev = torch.device("cuda")
    n, L = a.n, 5.12 / a.n
    W, H, fx, fy, cx, cy = 1200, 680, 600.0, 600.0, 599.5, 339.5
    vol = dqo_eval.TsdfVolume((-2.56, -2.56, 0.0), L, (n, n, n), 3 * L, dev)
    poses = [(-12.0 + 24.0 * k / max(1, a.frames - 1), (-0.6 + 1.2 * k / max(1, a.frames - 1), 0.0, 0.2)) for k in range(a.frames)]
    frames = [frame(W, H, fx, fy, cx, cy, yaw, pos, dev) for yaw, pos in poses]
    K = (fx, fy, cx, cy)
    print(f"device: {torch.cuda.get_device_name(0)}   grid {n}^3 of {L * 100:.2f} cm voxels, sdf_trunc {3 * L * 100:.2f} cm, frame {W} x {H}, {a.frames} poses")

    # how many voxels a frame touches: the weight's change over one integration
    touched = []
    for d, c, m in frames:
        before = vol.weight.clone()
        vol.integrate(d, c, K, m, depth_trunc=30.0)
        touched.append(int((vol.weight != before).sum()))
    del before
    N_vox = n ** 3
    print("touched voxels per frame: " + " ".join(str(t) for t in touched) + f"   of {N_vox}")
    d, c, m = frames[len(frames) // 2]
    t_mid = touched[len(frames) // 2]
    for _ in range(WARMUP):
        vol.integrate(d, c, K, m, depth_trunc=30.0)
    med, lo = timed(lambda: vol.integrate(d, c, K, m, depth_trunc=30.0), a.reps)
    floor = t_mid * 40
    print(f"TsdfVolume.integrate (one launch, the middle pose, {t_mid} touched voxels): median {med * 1e3:.1f} us, least {lo * 1e3:.1f} us of {a.reps}")
    print(f"traffic: {floor} bytes on the volume (40 x {t_mid}) + at most {16 * t_mid} gathered; volume alone at {HBM_PEAK / 1e12:.1f} TB/s: "
          f"{floor / HBM_PEAK * 1e6:.1f} us; achieved on the volume: {floor / (lo * 1e-3) / 1e12:.2f} TB/s")
    # a frame that touches nothing (depth 0 everywhere): the cost of the skips alone
    zero = torch.zeros_like(d)
    for _ in range(WARMUP):
        vol.integrate(zero, c, K, m)
    med0, lo0 = timed(lambda: vol.integrate(zero, c, K, m), a.reps)
    print(f"TsdfVolume.integrate of a frame without depth (every voxel skipped: arithmetic and one gathered pixel): median {med0 * 1e3:.1f} us, "
          f"least {lo0 * 1e3:.1f} us")

    # extraction of the volume the poses built (clear, integrate each once)
    vol.clear()
    for d, c, m in frames:
        vol.integrate(d, c, K, m, depth_trunc=30.0)
    cap_v, cap_f = 6_000_000, 12_000_000
    vol.extract(cap_v, cap_f)
    cnt = vol.counts()
    print("extract: " + "  ".join(f"{k}={v}" for k, v in cnt.items()))
    for _ in range(WARMUP):
        vol.extract(cap_v, cap_f)
    med, lo = timed(lambda: vol.extract(cap_v, cap_f), a.reps)
    V, F = cnt["vertices"], cnt["faces"]
    traffic = N_vox * (9 + 4 + 5 + 1) + V * (24 + 32) + F * 12
    print(f"TsdfVolume.extract (four launches): median {med:.3f} ms, least {lo:.3f} ms of {a.reps}")
    print(f"traffic: {traffic} bytes (19 x {N_vox} + 56 x {V} + 12 x {F}); at {HBM_PEAK / 1e12:.1f} TB/s: {traffic / HBM_PEAK * 1e3:.4f} ms")
    N.profile_enable(True)
    N.profile_collect()
    for _ in range(5):
        vol.extract(cap_v, cap_f)
    prof = N.profile_collect()
    N.profile_enable(False)
    for name, (ms, calls) in prof.items():
        print(f"  {name}: {ms / max(1, calls):.3f} ms per launch ({calls} launches, serialised by the timers)")


if __name__ == "__main__":
    main()
