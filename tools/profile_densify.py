"""Times the densified surfel cloud (dqo_eval.densify: dqo_surfel_densify, csrc/map_densify.hip) on the map of a BASELINE configuration,
all rows kept, and the whole geometry evaluation on it (FusedMapper.evaluate_geometry_densified) beside evaluate_geometry's one point per
Gaussian.  Device events around the calls, warmed up; the least time the memory traffic allows, computed from the shapes, is printed next
to the measurement:
    read      P row_keep bytes per pass that looks at every virtual point (three histogram passes when cap < P * M, the count pass, the
              emit pass) + 41 bytes per kept row in the emit pass (ten floats and the keep byte; an upper bound: only rows with a chosen
              point are loaded)
    written   n * 32 (12 point, 12 normal, 8 index) + cap keep bytes
over the HBM peak (8.0 TB/s).  The hashes — P * M keys per pass — are arithmetic, not traffic: the call is far from that floor.

    python tools/profile_densify.py [--cfg 3] [--sample-nums 1000000] [--reps 20] [--trace] > profiles/densify.txt
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
SIGMA, CIRCLE_NUM, LEVELS = 1, 30, 5
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--P", type=int, default=None)
    ap.add_argument("--sample-nums", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-densify", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_densify: needs a GPU (there is nothing to time without one)")
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    import dqo_eval
    dev = torch.device("cuda")
    cam, sc = scenes.make_config(a.cfg, P=a.P)
    fm = FusedMapper(sc, mapping.make_settings(cam, dev), dev)
    P, M = fm.P, SIGMA * CIRCLE_NUM * LEVELS
    cap = min(P * M, a.sample_nums)
    kw = dict(sigma=SIGMA, circle_num=CIRCLE_NUM, levels=LEVELS, sample_nums=a.sample_nums, seed=1, theta=dqo_eval.densify_theta(CIRCLE_NUM, 1))
    ws = torch.empty((N_ws(P),), dtype=torch.uint8, device=dev)

    def densify():
        return fm.densify(rows="all", want_index=True, workspace_buffer=ws, **kw)

    d = densify()
    hdr = d["header"].cpu().tolist()
    print(f"device: {torch.cuda.get_device_name(0)}   config {a.cfg}: P = {P}, M = {M}, P * M = {P * M}, cap = {cap}")
    print("header: " + "  ".join(f"{k}={v}" for k, v in zip(dqo_eval.DENSIFY_HEADER, hdr)))
    n = hdr[3]
    passes = 2 + (3 if cap < P * M else 0)
    read, written = passes * P + 41 * P, n * 32 + cap
    floor_ms = (read + written) / HBM_PEAK * 1e3
    for _ in range(WARMUP):
        densify()
    med, lo = timed(densify, a.reps)
    print(f"dqo_eval.densify (with normals and index, upload of the angle table included): median {med:.3f} ms, least {lo:.3f} ms of {a.reps}")
    print(f"traffic: {read} bytes read ({passes} passes x {P} keep bytes + 41 x {P}), {written} written ({n} x 32 + {cap}); "
          f"at {HBM_PEAK / 1e12:.1f} TB/s: {floor_ms:.4f} ms;  {P * M * passes} keys hashed")
    if not a.only_densify:
        rng = np.random.default_rng(4)
        gt_np = np.asarray(sc["xyz"], np.float32)
        gt = torch.tensor((gt_np[rng.permutation(P)[:min(P, 1000000)]] + rng.normal(0, 0.01, (min(P, 1000000), 3))).astype(np.float32), device=dev)
        table = torch.zeros((2, 32), dtype=torch.float32, device=dev)
        thres = (0.01, 0.03)
        dens = lambda: fm.evaluate_geometry_densified(gt, thres, out=table, row=0, densify=dict(rows="all", **kw))
        plain = lambda: fm.evaluate_geometry(gt, thres, out=table, row=1)
        for f in (dens, plain):
            for _ in range(2):
                f()
        reps = max(3, a.reps // 4)
        m1, l1 = timed(dens, reps)
        m2, l2 = timed(plain, reps)
        rows = table.cpu().tolist()
        names = ["accuracy", "completion", "chamfer"] + [f"{k}(<{th})" for th in thres for k in ("P", "R", "F1")]
        for what, r in (("densified", rows[0]), ("one point per Gaussian", rows[1])):
            print(f"{what:24s}" + "  ".join(f"{k}={v:.6g}" for k, v in zip(names, r[:3] + r[4:10])))
        print(f"evaluate_geometry_densified ({n} of {hdr[1]} points against {gt.shape[0]}): median {m1:.3f} ms, least {l1:.3f} ms of {reps}")
        print(f"evaluate_geometry ({P} points against {gt.shape[0]}): median {m2:.3f} ms, least {l2:.3f} ms of {reps}")
    if a.trace:  # a fresh child process under the profiler; the program after `--`
        with tempfile.TemporaryDirectory() as tmp:
            child_reps = 5
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "densify", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--cfg", str(a.cfg), "--sample-nums", str(a.sample_nums), "--reps", str(child_reps),
                   "--only-densify"]
            if a.P is not None:
                cmd += ["--P", str(a.P)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
            print(f"# rocprofv3 --kernel-trace --stats, {1 + WARMUP + child_reps} calls (exit {r.returncode})")
            if stats:
                lines = open(stats[0]).read().splitlines()
                for line in lines[:1] + [x for x in lines[1:] if "densify_" in x or "zero_words" in x]:  # (the call's own launches)
                    print(line)
            else:
                print(r.stdout[-2000:])


def N_ws(P):
    import _dqo_native as N
    return N.lib().dqo_surfel_densify_workspace_bytes(P, CIRCLE_NUM, LEVELS, SIGMA)


if __name__ == "__main__":
    main()
