"""Times the trajectory kernels (csrc/map_traj.hip): dqo_eval_ate at N = 2000 and N = 20000 (a room loop with 2 cm of noise), one
Trajectory.append (pose, camera tensors, keyframe test) and one 680 x 1200 world_maps (vertex and normal map).  Device events around the
calls, warmed up.

    python tools/profile_traj.py [--reps 10] [--trace] > profiles/traj_kernels.txt
--trace adds a child pass under `rocprofv3 --kernel-trace --stats` (the program after `--`) and prints the three kernels' rows.

The reference's side — Tracker.eval_total_ate's loop of eval_ate calls on a CPU — is timed by tests/golden/make_traj_golden.py, which runs
the reference's own function where the reference exists.
"""
import argparse
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

import numpy as np

H, W = 680, 1200


def trajectory(n, rng):
    s = np.linspace(0.0, 1.0, n)
    gt = np.stack([3.0 * np.cos(2 * np.pi * s), 2.0 * np.sin(2 * np.pi * s), 1.2 + 0.3 * np.sin(6 * np.pi * s)], 1)
    return gt, gt + 0.02 * rng.normal(size=gt.shape)


def timed(torch, fn, reps):
    out = []
    for rep in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= 3:
            out.append(a.elapsed_time(b) * 1e3)
    return out


def run(a):
    import torch
    import dqo_eval
    import dqo_icp
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    print(f"{torch.cuda.get_device_name(0)}: device events around the Python call (wrapper included), {a.reps} calls after 3 warm-up calls")
    line = lambda name, v: print(f"{name}: median {statistics.median(v):.1f} us, least {min(v):.1f} us")
    for n in (2000, 20000):
        gt, es = (torch.tensor(x, device=dev) for x in trajectory(n, rng))
        out = torch.empty((n,), dtype=torch.float64, device=dev)
        v = timed(torch, lambda: dqo_eval.eval_ate(es, gt, out=out), a.reps)
        line(f"eval_ate, N = {n} (the whole curve: {n} prefixes; ate[-1] = {float(out[-1]):.6f} cm)", v)
    proj = torch.eye(4, device=dev)
    rel = torch.eye(4, device=dev)
    rel[0, 3] = 0.01
    tr = dqo_icp.Trajectory(4096, dev, projection=proj, gaussian_update_frame=1)
    line("Trajectory.append (relative pose, camera tensors, keyframe test on every row)", timed(torch, lambda: tr.append(rel), a.reps))
    vc, nc = torch.rand((H, W, 3), device=dev), torch.rand((H, W, 3), device=dev)
    out = (torch.empty_like(vc), torch.empty_like(nc))
    v = timed(torch, lambda: tr.world_maps(vc, nc, out=out), a.reps)
    line(f"Trajectory.world_maps, {H} x {W} (vertex + normal map: {4 * vc.numel() * 4 / 1e6:.1f} MB read and written)", v)
    print(f"  = {4 * vc.numel() * 4 / 1e3 / statistics.median(v):.0f} GB/s at the median")
    if a.trace:  # a fresh child process under the profiler; the program after `--`
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "traj", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--reps", str(a.reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
            print(f"# rocprofv3 --kernel-trace --stats in a fresh process (exit {r.returncode}); eval_ate_kernel: {3 + a.reps} calls at N = 2000, then "
                  f"{3 + a.reps} at N = 20000 (MinNs / MaxNs are the two sizes)")
            if stats:
                lines = open(stats[0]).read().splitlines()
                for x in lines[:1] + [x for x in lines[1:] if any(k in x for k in ("eval_ate_kernel", "traj_append_kernel", "track_world_maps_kernel"))]:
                    print(x)
            else:
                print(r.stdout[-2000:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    run(ap.parse_args())
