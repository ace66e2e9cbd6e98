"""Times geometry evaluation (dqo_eval.eval_pcd: two dqo_nn1 searches + one reduction, csrc/knn.hip and csrc/map_eval.hip) at N x N points —
the surfel room of dqo_harness/scenes.py as the ground truth, a jittered copy as the reconstruction — against two baselines on the same
inputs:
    knn3   what the library offered before dqo_nn1: two dqo_knn3_query calls (one wave per query, K = 3, of which column 0 is used) and
           the torch reductions of SLAM/eval.py:190-226 on the device, one .tolist() at the end;
    host   the reference's own statements: scipy's cKDTree built and queried on the host, 4 + 2 T times (tests/pcd_oracle.py holds the
           same statements to two builds; here they run as written), single-threaded.  `--host-reps` passes (default 1: it takes seconds).
The two device sides alternate, five runs each; every run is the median of `--reps` calls between two synchronisations.

    python tools/profile_pcd.py [--N 1000000] [--reps 5] [--trace] > profiles/eval_pcd.txt
--trace adds a child pass under `rocprofv3 --kernel-trace --stats` (the program after `--`) and prints its kernel table.

    python tools/profile_pcd.py --objects [--gt-per-object 1000000] [--rec-per-object 100000] > profiles/eval_pcd_objects.txt
--objects times the per-object evaluation at metric_obj.py's workload instead — four box-shaped objects, `--gt-per-object` ground-truth
samples each, a stable cloud of 4 x `--rec-per-object` rows plus a tenth as many rows without an object — dqo_eval.eval_pcd_objects (two
grouped searches + one reduction) against the loop it replaces: four dqo_eval.eval_pcd calls with that object's keep masks, each of
which sorts and scans every row of both sets.  Same alternation and medians; then one evaluation of each side under the library's own
per-kernel brackets (dqo_profile_enable), which serialise the launches: the split, not the total.
"""
import argparse
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

import numpy as np
import torch

THRES = (0.01, 0.03)


def torch_metrics(d_rec, d_gt, thres):
    """eval.py:190-226 / :263-281 from the two distance arrays, on the device; one host read."""
    vals = [d_rec.mean() * 100, d_gt.mean() * 100, d_rec.mean() + d_gt.mean()]
    for th in thres:
        P, R = (d_rec < th).float().mean() * 100, (d_gt < th).float().mean() * 100
        vals += [P, R, 2 * P * R / (P + R)]
    return torch.stack(vals).tolist()


def host_eval_pcd(gt, rec, thres):
    """The reference's statements as written (SLAM/eval.py:190-226, 253-281): a KDTree per statement."""
    from scipy.spatial import cKDTree as KDTree
    chamfer = np.mean(KDTree(gt).query(rec)[0]) + np.mean(KDTree(rec).query(gt)[0])
    acc, comp = np.mean(KDTree(gt).query(rec)[0]), np.mean(KDTree(rec).query(gt)[0])
    out = [acc * 100, comp * 100, chamfer]
    for th in thres:
        P = np.mean((KDTree(gt).query(rec)[0] < th).astype(np.float32)) * 100
        R = np.mean((KDTree(rec).query(gt)[0] < th).astype(np.float32)) * 100
        out += [P, R, 2 * P * R / (P + R)]
    return out


def objects_mode(a):
    import _dqo_native as N
    import dqo_eval
    dev = torch.device("cuda")
    rng = np.random.default_rng(6)
    boxes = {0: ((0.0, 0.0, 0.0), (0.6, 0.4, 0.08)), 5: ((0.1, 0.1, 0.08), (0.2, 0.2, 0.22)), 17: ((0.5, -0.1, 0.0), (1.1, 0.35, 0.05)),
             63: ((1.5, 0.2, 0.0), (2.0, 0.8, 0.9))}  # a book, a cup on it, a laptop whose box cuts the book's, a chair apart

    def faces(n, lo, hi):
        lo, hi = np.asarray(lo), np.asarray(hi)
        p = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
        axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
        p[np.arange(n), axis] = np.where(side == 1, hi[axis], lo[axis])
        return p

    G, Rn = a.gt_per_object, a.rec_per_object
    gt_np = np.concatenate([faces(G, *boxes[g]) for g in boxes]).astype(np.float32)
    gt_obj = np.repeat(np.int32(list(boxes)), G)
    rec_np = np.concatenate([faces(Rn, *boxes[g]) + rng.normal(0, 0.004, (Rn, 3)) for g in boxes]
                            + [rng.uniform(-0.2, 2.2, (4 * Rn // 10, 3))]).astype(np.float32)
    rec_obj = np.concatenate([np.repeat(np.int32(list(boxes)), Rn), np.full((4 * Rn // 10,), -1, np.int32)])
    pg, pr = rng.permutation(gt_np.shape[0]), rng.permutation(rec_np.shape[0])
    gt, gt_o = torch.tensor(gt_np[pg], device=dev), torch.tensor(gt_obj[pg], device=dev)
    rec, rec_o = torch.tensor(rec_np[pr], device=dev), torch.tensor(rec_obj[pr], device=dev)
    masks = {g: (gt_o == g, rec_o == g) for g in boxes}
    table, rows = torch.zeros((64, 32), dtype=torch.float32, device=dev), torch.zeros((4, 32), dtype=torch.float32, device=dev)
    th = (0.01,)

    def grouped():
        return dqo_eval.eval_pcd_objects(gt, gt_o, rec, rec_o, th, out=table, row=0)

    def masked():
        for k, g in enumerate(boxes):
            dqo_eval.eval_pcd(gt, rec, th, gt_keep=masks[g][0], rec_keep=masks[g][1], out=rows, row=k)
        return rows

    t, m = grouped().cpu().numpy(), masked().cpu().numpy()
    for k, g in enumerate(boxes):
        print(f"object {g:2d}  eval_pcd_objects " + "  ".join(f"{v:.6g}" for v in t[g, :7]) + "   masked eval_pcd " + "  ".join(f"{v:.6g}" for v in m[k, :7]))
    sides = {"eval_pcd_objects (2 grouped searches + 1 reduction)": grouped, "4 x eval_pcd with keep masks (8 searches + 4 reductions)": masked}
    times = {k: [] for k in sides}
    for run in range(5):
        for name, f in sides.items():
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            times[name].append(statistics.median(ts))
    print(f"device: {torch.cuda.get_device_name(0)}   4 objects, ground truth 4 x {G}, reconstruction 4 x {Rn} + {4 * Rn // 10} rows without an object, "
          f"threshold {th}")
    for name, ts in times.items():
        print(f"{name:58s} ms per evaluation, five runs (median of {a.reps} calls each): " + "  ".join(f"{v:.3f}" for v in ts))
    for name, f in sides.items():  # the split: one evaluation, every launch bracketed (serialised: the sum is not the time above)
        torch.cuda.synchronize()
        N.profile_enable(True)
        f()
        prof = N.profile_collect()
        N.profile_enable(False)
        print(f"# per kernel, one evaluation of: {name}   (sum {sum(v[0] for v in prof.values()):.3f} ms)")
        for k, (ms, calls) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
            print(f"    {k:32s} {ms:9.3f} ms  {calls:4d} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--only", choices=["nn1", "knn3"], default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--objects", action="store_true")
    ap.add_argument("--gt-per-object", type=int, default=1000000)
    ap.add_argument("--rec-per-object", type=int, default=100000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_pcd: needs a GPU (there is nothing to time without one)")
    if a.objects:
        return objects_mode(a)
    from dqo_harness import scenes
    from dqo_mapgrowth import knn_points_k3
    import dqo_eval
    dev = torch.device("cuda")
    gt_np = np.asarray(scenes.surfel_room(3, a.N)["xyz"], np.float32)
    rng = np.random.default_rng(4)
    rec_np = (gt_np[rng.permutation(a.N)] + rng.normal(0, 0.01, (a.N, 3))).astype(np.float32)
    gt, rec = torch.tensor(gt_np, device=dev), torch.tensor(rec_np, device=dev)
    table = torch.zeros((1, 32), dtype=torch.float32, device=dev)

    def nn1():
        return dqo_eval.eval_pcd(gt, rec, THRES, out=table, row=0)

    def knn3():
        d_rec = knn_points_k3(rec, gt, int32_idx=True)[0][:, 0].sqrt()
        d_gt = knn_points_k3(gt, rec, int32_idx=True)[0][:, 0].sqrt()
        return torch_metrics(d_rec, d_gt, THRES)

    names = ["accuracy", "completion", "chamfer"] + [f"{n}(<{th})" for th in THRES for n in ("P", "R", "F1")]
    sides = {"nn1": nn1, "knn3": knn3}
    if a.only:
        sides = {a.only: sides[a.only]}
    if "nn1" in sides:
        row = nn1().cpu().tolist()
        print("eval_pcd           " + "  ".join(f"{n}={v:.6g}" for n, v in zip(names, row[:3] + row[4:10])))
    if "knn3" in sides:
        print("knn3_query + torch " + "  ".join(f"{n}={v:.6g}" for n, v in zip(names, knn3())))
    if a.only is None:
        d1 = dqo_eval.nearest(rec, gt, want_idx=False)[0]
        d3 = knn_points_k3(rec, gt, int32_idx=True)[0][:, 0]
        print(f"dqo_nn1 against dqo_knn3_query column 0, rec -> gt: {int((d1.view(torch.int32) != d3.contiguous().view(torch.int32)).sum())} of {a.N} differ")
    times = {k: [] for k in sides}
    for run in range(5):  # alternated: every side sees the same drift
        for name, f in sides.items():
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            times[name].append(statistics.median(ts))
    print(f"device: {torch.cuda.get_device_name(0)}   N = {a.N} x {a.N}   thresholds {THRES}")
    what = {"nn1": "dqo_eval.eval_pcd (2 x dqo_nn1 + 1 reduction)", "knn3": "2 x dqo_knn3_query + torch reductions + 1 read"}
    for name, ts in times.items():
        print(f"{what[name]:48s} ms per evaluation, five runs (median of {a.reps} calls each): " + "  ".join(f"{t:.3f}" for t in ts))
    if a.only is None and a.host_reps > 0:
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host = host_eval_pcd(gt_np, rec_np, THRES)
            ts.append(time.perf_counter() - t0)
        print("host cKDTree       " + "  ".join(f"{n}={v:.6g}" for n, v in zip(names, host)))
        print(f"{'reference statements, scipy cKDTree on the host':48s} s per evaluation ({a.host_reps} pass): " + "  ".join(f"{t:.2f}" for t in ts))
    if a.trace:  # a fresh child process under the profiler; the program after `--`
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "pcd", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--N", str(a.N), "--reps", "2", "--only", "nn1"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
            print(f"# rocprofv3 --kernel-trace --stats, 11 evaluations (exit {r.returncode})")
            if stats:
                for line in open(stats[0]).read().splitlines()[:24]:
                    print(line)
            else:
                print(r.stdout[-2000:])


if __name__ == "__main__":
    main()
