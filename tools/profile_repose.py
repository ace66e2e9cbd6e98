"""Times a pose correction (FusedMapper.update_poses, csrc/map_repose.hip) against the path there was before it, at 1200 x 680 on the
map of dqo_harness.scenes (config 3), on the same GPU: a keyframe bank of 40 and a window of five, every one of the 45 cameras bound to
a trajectory row and moved by the correction.

    (a) one launch   fm.update_poses(traj, new_poses): the store, the trajectory's own camera, five window graphs' settings tensors and
                     forty bank rows in ONE dqo_traj_repose launch
    (b) 45 calls     per camera: Trajectory.append(pose, relative=False) on a scratch trajectory, then bank_set(slot, settings=...) /
                     set_frame(k, settings=...) — four small device copies each (and the store's rows are not rewritten at all)

For both: host wall time of the call(s) as issued (time.perf_counter around them, nothing synchronised inside) and GPU time (HIP events
around them, which for host-issued launches includes the gaps the host leaves); `--samples` samples each, median and min .. max.
(a) also replayed from a captured graph of `--burst` launches: the launch's own GPU time.  Nothing further is started after a failure.

    python tools/profile_repose.py [--P 100000] [--samples 30]      # writes profiles/repose.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WINDOW, BANK = 5, 40


def spread(xs, unit="us", scale=1e3):
    xs = [x * scale for x in xs]
    return f"median {statistics.median(xs):9.2f} {unit}   min .. max {min(xs):9.2f} .. {max(xs):9.2f}   ({len(xs)} samples)"


def timed(torch, issue, samples, before=None):
    """(host ms, GPU ms) per call of `issue`: perf_counter around the call as issued, HIP events around it."""
    host, gpu = [], []
    for _ in range(samples + 3):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        issue()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        host.append((t1 - t0) * 1e3), gpu.append(e0.elapsed_time(e1))
    return host[3:], gpu[3:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repose.txt"))
    a = ap.parse_args()
    import numpy as np
    from profile_window_bank import cameras, problem
    torch, dev, cam, scene, frames = problem(a.P, 2)  # two keyframes' images serve every slot: a camera does not read them
    import dqo_icp
    from dqo_harness import mapping
    from dqo_harness.fused_mapping import FusedMapper
    cams = cameras(cam, WINDOW + BANK, 0.5, 0.01)
    poses = np.stack([np.linalg.inv(c.Rt) for c in cams])
    rng = np.random.default_rng(1)
    new = poses.copy()
    new[:, :3, 3] += rng.uniform(-0.01, 0.01, size=(len(cams), 3))
    projection = torch.tensor(cam.projection_matrix, device=dev)
    settings = [mapping.make_settings(c, dev) for c in cams]
    frame = lambda i, row=None: dict(frames[i % 2], settings=settings[i], **({} if row is None else {"row": row}))
    lines = [f"device: {torch.cuda.get_device_name(0)}   P = {a.P}   {cam.W} x {cam.H}   window of {WINDOW}, bank of {BANK}: {WINDOW + BANK} cameras"]

    def mapper(rows):
        fm = FusedMapper(scene, settings[0], dev)
        fm.begin_mapping_call(reset_optimizer=True)
        fm.capture_window([frame(i, i if rows else None) for i in range(WINDOW)], loss_tap=True, fused_tail=True)
        fm.capture_bank([frame(WINDOW + i, WINDOW + i if rows else None) for i in range(BANK)], loss_tap=True, fused_tail=True)
        return fm

    # (a) the one launch
    fm = mapper(True)
    traj = dqo_icp.Trajectory(64, dev, projection=projection)
    P0, P1 = torch.tensor(poses, device=dev), torch.tensor(new, device=dev)
    for i in range(len(cams)):
        traj.append(P0[i], relative=False)
    turn = [0]

    def one_launch():
        turn[0] += 1
        fm.update_poses(traj, P1 if turn[0] % 2 else P0)

    one_launch()
    stats = traj.repose_stats.tolist()
    assert stats == [WINDOW + BANK, WINDOW + BANK + 1, 0, 0], stats
    host_a, gpu_a = timed(torch, one_launch, a.samples)
    lines.append("(a) fm.update_poses, one launch: host wall time        " + spread(host_a))
    lines.append("(a) fm.update_poses, one launch: GPU time (events)     " + spread(gpu_a))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(a.burst):
            fm.update_poses(traj, P1)
    _, rep = timed(torch, graph.replay, a.samples)
    lines.append(f"(a) the launch replayed from a graph of {a.burst}, per launch  " + spread([t / a.burst for t in rep]))
    del fm

    # (b) the 45-call path
    fm2 = mapper(False)
    scratch = dqo_icp.Trajectory(WINDOW + BANK, dev, projection=projection)
    empty = scratch.header.clone()

    def reset():
        scratch.header.copy_(empty)
        scratch._n = 0
        turn[0] += 1

    def calls():
        P = P1 if turn[0] % 2 else P0
        for i in range(WINDOW + BANK):
            scratch.append(P[i], relative=False)
            st = scratch.settings(settings[i])
            if i < WINDOW:
                fm2.set_frame(i, settings=st)
            else:
                fm2.bank_set(i - WINDOW, settings=st)

    host_b, gpu_b = timed(torch, calls, a.samples, before=reset)
    lines.append(f"(b) {WINDOW + BANK} x (append + set_frame / bank_set): host wall time  " + spread(host_b))
    lines.append(f"(b) {WINDOW + BANK} x (append + set_frame / bank_set): GPU time       " + spread(gpu_b))
    ha, hb = statistics.median(host_a) * 1e3, statistics.median(host_b) * 1e3
    lines.append(f"    host: one launch {ha:.1f} us against {hb:.1f} us ({hb / ha:.1f} x); faster on the host side: {ha < hb}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
