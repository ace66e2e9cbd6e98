"""Times the object stage (dqo_quadrics.ObjectMap: dqo_objmap_frame, dqo_objmap_optimize; csrc/map_objects.hip) on a synthetic frame: a
1200 x 680 depth image, a table of `--objects` objects of distinct categories on a grid of 60-pixel cells (built through the stage itself,
32 new detections a frame), then a frame whose `--M` detections each match one stored object, followed by the optimise launch over the
rows that frame flagged.  Device events around the two calls, warmed up.

    python tools/profile_objects.py [--objects 200] [--M 32] [--cap-obj 256] [--reps 10] [--trace] > profiles/objects.txt
--trace adds a child pass under `rocprofv3 --kernel-trace --stats` (the program after `--`) and prints the two kernels' rows.

    python tools/profile_objects.py --reference ROOT [--objects 200] [--M 32] [--reps 10]
times, on the CPU and without any GPU, the host stage the launch replaces — the reference's detections_filter, Occlusions_Check,
MatchObject and remove_outlier (ROOT/SLAM/multiprocess/quadrics.py, driven as mapper.py:155-163 drives them) — on the same scene, with the
depth map as a host tensor (in the reference it is a device tensor and each of the 30 samples per detection is a device read, so this
is a lower bound of its cost).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

W, H, CELL, BOX = 1200, 680, 60, 40
K = np.array([[600.0, 0, 600.0], [0, 600.0, 340.0], [0, 0, 1]], np.float32)
RT = np.eye(4, dtype=np.float32)[:3]
SEED = 5


def depth_image():
    return (np.float32(2.0) + (np.arange(W) % 8 / 128.0).astype(np.float32))[None, :].repeat(H, 0).copy()


def detections(cells):
    cols = W // CELL
    bbox = np.array([[(c % cols) * CELL + 10, (c // cols) * CELL + 10, (c % cols) * CELL + 10 + BOX, (c // cols) * CELL + 10 + BOX] for c in cells],
                    np.float32)
    ell = np.stack([(bbox[:, 0] + bbox[:, 2]) / 2, (bbox[:, 1] + bbox[:, 3]) / 2, bbox[:, 2] - bbox[:, 0], bbox[:, 3] - bbox[:, 1],
                    np.zeros(len(cells), np.float32)], 1)
    return dict(bbox=bbox, ellipse=ell.astype(np.float32), cat=np.array([c + 1 for c in cells], np.int32), score=np.full(len(cells), 0.9, np.float32))


def build_frames(n_objects):
    return [detections(range(i, min(i + 32, n_objects))) for i in range(0, n_objects, 32)]


def run_gpu(a):
    import torch
    import dqo_quadrics as dq
    assert a.objects <= (W // CELL) * (H // CELL) and a.M <= min(a.objects, 64)
    om = dq.ObjectMap(a.cap_obj, 64, 64, device="cuda:0")
    depth = torch.from_numpy(depth_image()).cuda()
    Kd, Rtd = torch.from_numpy(K).cuda(), torch.from_numpy(RT).cuda()
    for fi, d in enumerate(build_frames(a.objects)):
        om.frame(d, depth, Kd, Rtd, fi, SEED)
    d = {k: torch.as_tensor(v).cuda() for k, v in detections(range(a.M)).items()}
    times = {"frame": [], "optimize": []}
    hdr = None
    for rep in range(3 + a.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        out = om.frame(d, depth, Kd, Rtd, 100 + rep, SEED)
        ev[1].record()
        om.optimize(100 + rep, SEED)
        ev[2].record()
        torch.cuda.synchronize()
        if rep >= 3:
            times["frame"].append(ev[0].elapsed_time(ev[1]))
            times["optimize"].append(ev[1].elapsed_time(ev[2]))
        hdr = out["header"].cpu().tolist()
    print(f"{torch.cuda.get_device_name(0)}: table of {int(om.state[0])} objects (cap_obj {a.cap_obj}, cap_views 64), M = {a.M}, {W} x {H}")
    print("last frame header: " + ", ".join(f"{k} {v}" for k, v in zip(dq.FRAME_HEADER, hdr)) + f"; rows flagged {int(om.opt_flag.sum())}")
    for k, v in times.items():
        print(f"ObjectMap.{k}: median {statistics.median(v) * 1e3:.1f} us, least {min(v) * 1e3:.1f} us of {len(v)} calls (device events, wrapper included)")
    if a.trace:  # a fresh child process under the profiler; the program after `--`
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "objects", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--objects", str(a.objects), "--M", str(a.M), "--cap-obj", str(a.cap_obj), "--reps", str(a.reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
            print(f"# rocprofv3 --kernel-trace --stats in a fresh process (exit {r.returncode}); objmap_frame_kernel: {len(build_frames(a.objects))} "
                  f"building frames + {3 + a.reps} frames of M = {a.M}")
            if stats:
                lines = open(stats[0]).read().splitlines()
                for line in lines[:1] + [x for x in lines[1:] if "objmap_" in x]:
                    print(line)
            else:
                print(r.stdout[-2000:])


def run_reference(a):
    import platform
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("make_object_stage_golden", os.path.join(ROOT, "tests", "golden", "make_object_stage_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    Q = gen.load_reference(a.reference)
    import random
    Q.random = random
    depth = torch.from_numpy(depth_image())
    Kd, Rt = K.astype(np.float64), RT.astype(np.float64)

    def info(d):
        return dict(detections=[dict(ellipse=[float(x) for x in d["ellipse"][i]], category_id=int(d["cat"][i]), bbox=[float(x) for x in d["bbox"][i]],
                                     detection_score=float(d["score"][i]), color=[0, 0, 0]) for i in range(len(d["cat"]))])

    def stage(Map_global, d, frame_id):  # mapper.py:155-163
        dets = Q.get_2dim_quarics(info(d))
        cur, cur_depth = Q.detections_filter(dets, depth, W, H)
        if Map_global is None:
            return Q.ObjectsInitialization(cur, cur_depth, Rt, Kd)
        proj = Q.Occlusions_Check(Map_global, Kd, Rt, W, H, frame_id)
        Q.MatchObject(Map_global, cur, cur_depth, proj, frame_id, torch.zeros(H, W, 3), Kd, Rt)
        return Q.remove_outlier(Map_global, Kd, Rt, False)

    Map_global = None
    for fi, d in enumerate(build_frames(a.objects)):
        Map_global = stage(Map_global, d, fi)
    d, times = detections(range(a.M)), []
    for rep in range(1 + a.reps):
        t0 = time.perf_counter()
        Map_global = stage(Map_global, d, 100 + rep)
        if rep:
            times.append(time.perf_counter() - t0)
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), platform.processor())
    print(f"reference host stage on a CPU ({cpu}; depth map as a host tensor, save_img as in the reference): {len(Map_global)} objects, M = {a.M}: "
          f"median {statistics.median(times) * 1e3:.1f} ms, least {min(times) * 1e3:.1f} ms of {len(times)} frames")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=200)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--cap-obj", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    run_reference(a) if a.reference else run_gpu(a)
