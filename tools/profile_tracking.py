"""Times one tracking frame at 1200x680 on the GPU: preprocess_frame (frame geometry), the current frame's pyramids, the model-depth
fill, the model-depth pyramids, 3 levels x 5 Gauss-Newton iterations and the failure test — i.e. what DQO-MAP's tracker does per frame
around the rasteriser — eager and as one replayed torch.cuda.graph.

    python tools/profile_tracking.py [--frames N] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o track -- python tools/profile_tracking.py --frames 50   (GPU time per kernel)

Prints one JSON object: wall time per frame eager / replayed, and GPU time per kernel from the library's own event brackets
(dqo_profile_enable; a separate pass, so the brackets do not disturb the wall times)."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dqo-map_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _dqo_native as N  # noqa: E402
import dqo_icp as M  # noqa: E402

ARGS = types.SimpleNamespace(icp_downscales=[0.25, 0.5, 1.0], icp_downscale_iters=[5, 5, 5], icp_damping=1e-4, icp_distance_threshold=0.1,
                             icp_normal_threshold=20, icp_sample_distance_threshold=0.01, icp_sample_normal_threshold=0.01,
                             icp_fail_threshold=0.02, icp_use_model_depth=True, icp_warmup_frames=0, verbose=False)


def depth_map(H, W, shift, seed):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    z = 2.0 + 0.4 * np.sin((jj + shift) / 53.0) + 0.3 * np.cos(ii / 37.0) + 0.5 * (jj + shift > W // 2) + 0.003 * rng.normal(size=(H, W))
    z[rng.uniform(size=(H, W)) < 0.03] = 0.0
    return torch.tensor(z.astype(np.float32), device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = 680, 1200
    # DQO-MAP passes a new GPU intrinsic tensor every frame (frame.get_intrinsic): a fresh device copy per call here as well
    K_gpu = torch.tensor([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]], device="cuda")
    K = K_gpu.clone()
    d0, d1 = depth_map(H, W, 0.0, 1), depth_map(H, W, 3.0, 2)
    tr = M.IcpTracker(ARGS)
    f0 = M.preprocess_frame(d0, K, 0.3, 5.0, 0.2)
    tr.update_curr_status(f0["depth_map"], K)
    tr.move_last_status()
    render = (f0["depth_map"] + 0.005).contiguous()

    def step():
        f1 = M.preprocess_frame(d1, K_gpu.clone(), 0.3, 5.0, 0.2)
        tr.update_curr_status(f1["depth_map"], K_gpu.clone())
        tr.update_last_status(None, render, f0["depth_map"], f0["normal_map_c"], f0["normal_map_c"])
        return tr.predict_pose_async({"K": K_gpu.clone(), "frame_id": 1})

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(a.frames):
        step()
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t) / a.frames * 1e3

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(a.frames):
        g.replay()
    torch.cuda.synchronize()
    replay_ms = (time.perf_counter() - t) / a.frames * 1e3

    N.profile_enable(True)
    N.profile_collect(reset=True)
    for _ in range(a.frames):
        step()
    prof = N.profile_collect(reset=True)
    N.profile_enable(False)
    per_kernel = {k: dict(ms_per_frame=round(v[0] / a.frames, 5), launches_per_frame=v[1] / a.frames) for k, v in sorted(prof.items())}
    res = dict(shape=[H, W], frames=a.frames, eager_wall_ms_per_frame=round(eager_ms, 4), graph_replay_wall_ms_per_frame=round(replay_ms, 4),
               library_launches_per_frame=sum(v["launches_per_frame"] for v in per_kernel.values()),
               gpu_ms_per_frame_event_brackets=round(sum(v["ms_per_frame"] for v in per_kernel.values()), 5), per_kernel=per_kernel,
               pose=step()[0].cpu().numpy().round(6).tolist())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
