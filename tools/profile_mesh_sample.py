"""Times the ground-truth mesh sampler (dqo_eval.sample_surface: dqo_mesh_sample, csrc/map_meshsample.hip) on a synthetic mesh of about
Replica's size — a bumpy height field of F triangles — and, for scale, the two exact 1-NN searches (dqo_eval.nearest: dqo_nn1) and the
whole dqo_eval.eval_pcd of the same evaluation: `count` sampled points against a reconstruction of as many points 1 cm off the surface.
Device events around the calls, warmed up; the least time the memory traffic allows, computed from the shapes, is printed next to the
measurement:
    read      area: 12 F index bytes + 36 F vertex bytes (a gather: an upper bound, neighbouring faces share vertices);
              quantise and scan: 8 F each; sample: per sample 48 bytes of its face and about log2(F) table entries of 8 bytes (a dependent
              chain, mostly cache hits near the root)
    written   area, quantise, scan: 8 F each; sample: 12 + 4 + 1 bytes per sample
over the HBM peak (8.0 TB/s).

    python tools/profile_mesh_sample.py [--F 2000000] [--count 1000000] [--reps 20] [--trace] > profiles/mesh_sample.txt
--trace adds a child pass under `rocprofv3 --kernel-trace --stats` (the program after `--`) and prints its kernel table.
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
import torch

HBM_PEAK = 8.0e12  # bytes / s
WARMUP = 3  # calls between the first one (whose header is printed) and the timed ones


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


def height_field(F, seed=0):
    """(vertices float32 [V,3], faces int32 [F,3]): an n x n grid of quads over 8 m x 8 m cut in two, z a sum of a few sines plus 5 mm of
    noise (no two triangles have the same area), the faces in a random order (a scanned mesh's faces are not sorted in space)."""
    n = int(np.ceil(np.sqrt(F / 2)))
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 8.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.3 * np.sin(1.7 * x) * np.cos(2.3 * y) + 0.1 * np.sin(9.1 * x + 4.0 * y) + rng.normal(0, 0.005, x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    a = i * (n + 1) + j
    b, c, d = a + (n + 1), a + (n + 1) + 1, a + 1
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v, f[rng.permutation(f.shape[0])[:F]].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=2000000)
    ap.add_argument("--count", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-sample", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_mesh_sample: needs a GPU (there is nothing to time without one)")
    import dqo_eval
    dev = torch.device("cuda")
    v_np, f_np = height_field(a.F)
    v, f = torch.tensor(v_np, device=dev), torch.tensor(f_np, device=dev)
    V, F, count = v.shape[0], f.shape[0], a.count
    ws = dqo_eval.mesh_sample_workspace(F, count, dev)

    def sample():
        return dqo_eval.sample_surface(v, f, count, seed=1, want_face_index=True, workspace_buffer=ws)

    d = sample()
    hdr = d["header"].cpu().tolist()
    print(f"device: {torch.cuda.get_device_name(0)}   height field: V = {V}, F = {F}, count = {count}")
    print("header: " + "  ".join(f"{k}={x}" for k, x in zip(dqo_eval.MESH_HEADER, hdr)))
    steps = int(np.ceil(np.log2(max(F, 2))))
    read = (12 + 36) * F + 8 * F + 8 * F + count * (48 + 8 * steps)
    written = 3 * 8 * F + count * 17
    for _ in range(WARMUP):
        sample()
    med, lo = timed(sample, a.reps)
    print(f"dqo_eval.sample_surface (with face_index; four launches): median {med:.3f} ms, least {lo:.3f} ms of {a.reps}")
    print(f"traffic: {read} bytes read (64 x {F} + {count} x (48 + 8 x {steps})), {written} written (24 x {F} + 17 x {count}); "
          f"at {HBM_PEAK / 1e12:.1f} TB/s: {(read + written) / HBM_PEAK * 1e3:.4f} ms")
    if not a.only_sample:
        gt = d["points"]
        rec = (dqo_eval.sample_surface(v, f, count, seed=2)["points"] + 0.01 * torch.randn((count, 3), device=dev)).contiguous()
        table = torch.zeros((1, 32), dtype=torch.float32, device=dev)
        thres = (0.01, 0.03)
        sides = (("dqo_eval.nearest, reconstruction -> ground truth", lambda: dqo_eval.nearest(rec, gt, want_idx=False)),
                 ("dqo_eval.nearest, ground truth -> reconstruction", lambda: dqo_eval.nearest(gt, rec, ref_keep=None, want_idx=False)),
                 ("dqo_eval.eval_pcd (both searches and the reduction)", lambda: dqo_eval.eval_pcd(gt, rec, thres, gt_keep=d["keep"], out=table)))
        reps = max(3, a.reps // 4)
        for name, fn in sides:
            for _ in range(2):
                fn()
            m, l = timed(fn, reps)
            print(f"{name} ({count} against {count}): median {m:.3f} ms, least {l:.3f} ms of {reps}")
        r = table.cpu().tolist()[0]
        names = ["accuracy", "completion", "chamfer"] + [f"{k}(<{th})" for th in thres for k in ("P", "R", "F1")]
        print("row: " + "  ".join(f"{k}={x:.6g}" for k, x in zip(names, r[:3] + r[4:10])))
    if a.trace:  # a fresh child process under the profiler; the program after `--`
        with tempfile.TemporaryDirectory() as tmp:
            child_reps = 5
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "mesh_sample", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--F", str(a.F), "--count", str(a.count), "--reps", str(child_reps), "--only-sample"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
            print(f"# rocprofv3 --kernel-trace --stats, {1 + WARMUP + child_reps} calls (exit {r.returncode})")
            if stats:
                lines = open(stats[0]).read().splitlines()
                for line in lines[:1] + [x for x in lines[1:] if "mesh_" in x]:  # (the call's own launches)
                    print(line)
            else:
                print(r.stdout[-2000:])


if __name__ == "__main__":
    main()
