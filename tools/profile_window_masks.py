"""Times the loop that opens a mapping call — evaluate_render_range over the five frames of the window (SLAM/multiprocess/mapper.py:549-555)
— at 1200 x 680 on the 500 k map of dqo_harness.scenes (config 3), two ways on the same GPU:

    refresh   FusedMapper.refresh_window: per frame one render on the persistent context and one dqo_window_masks launch, in place
    chain     what a caller did before it existed: mapping.render of the trained cloud through the drop-in operator (its default mode reads
              a header back per call), dqo_tilemask.evaluate_render_range, FusedMapper.set_frame(k, render_mask=, tile_mask=)

Each side runs in a process of its own under its own time limit; the second is not started if the first fails.  A side reports the
median wall time of `--reps` passes over the window between two synchronisations, five runs.

    python tools/profile_window_masks.py [--P 500000] [--reps 10] [--limit 300]      # writes profiles/window_masks.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

FRAMES = 5


def side(name, P, reps, mode):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("profile_window_masks: needs a GPU (there is nothing to time without one)")
    import dqo_tilemask
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam, scene = scenes.make_config(3, P=P)
    cams = [scenes.replica_camera(cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy, yaw=12.0 + 1.5 * (k - FRAMES // 2), pitch=4.0 + 0.5 * (k % 3 - 1))
            for k in range(FRAMES)]
    settings = [mapping.make_settings(c, dev) for c in cams]
    H, W = cam.H, cam.W
    frames = []
    for k, st in enumerate(settings):
        t = mapping.perturbed_target(scene, st, dev, 100 + k)
        frames.append(dict(gt_color=t["gt_color"], gt_depth=t["gt_depth"], settings=st, render_mask=torch.ones((H, W), dtype=torch.bool, device=dev),
                           tile_mask=torch.ones(((H + 15) // 16, (W + 15) // 16), dtype=torch.int32, device=dev)))
    fm = FusedMapper(scene, settings[0], dev)
    fm.capture_window(frames, loss_tap=True, fused_tail=True)
    kw = dict(global_opt=True, sample_ratio=0.4) if mode == "error" else dict()

    def refresh():
        fm.refresh_window(**kw)

    def chain():
        opacity, scales, rotations = fm.activate()
        data = dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs)  # (every row is trained here: the whole map)
        for k, fr in enumerate(frames):
            out = mapping.render(fr["settings"], data)
            rm, tm, _ = dqo_tilemask.evaluate_render_range(out["T_map"], out["render"], fr["gt_color"], **kw)
            fm.set_frame(k, render_mask=rm, tile_mask=tm)

    f = refresh if name == "refresh" else chain
    with torch.no_grad():
        f()
        if name == "refresh" and fm.maintain_overflowed():
            f()
        runs = []
        for _ in range(5):
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            runs.append(statistics.median(ts))
    ok = name != "refresh" or not fm.maintain_overflowed()
    what = {"refresh": "FusedMapper.refresh_window", "chain": "mapping.render + evaluate_render_range + set_frame"}[name]
    print(f"device: {torch.cuda.get_device_name(0)}   P = {P}   {FRAMES} frames   {W} x {H}   mode = {mode}")
    print(f"{what:52s} ms per window of {FRAMES}, five runs (median of {reps} passes each): " + "  ".join(f"{t:.3f}" for t in runs)
          + ("" if ok else "   A FRAME OUTGREW THE RENDER CONTEXT"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds a side may take")
    ap.add_argument("--side", choices=["refresh", "chain"], default=None, help="(internal) run one side in this process")
    ap.add_argument("--mode", choices=["local", "error"], default="local")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_masks.txt"))
    a = ap.parse_args()
    if a.side:
        return side(a.side, a.P, a.reps, a.mode)
    lines = []
    for mode in ("local", "error"):
        for name in ("refresh", "chain"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--side", name, "--mode", mode, "--P", str(a.P),
                   "--reps", str(a.reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"profile_window_masks: side {name} ({mode}) ended with status {r.returncode}; nothing further was started")
            lines += [l for l in r.stdout.splitlines() if l.startswith(("device:", "FusedMapper", "mapping.render")) and l not in lines]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
