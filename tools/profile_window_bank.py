"""Times the keyframe bank (FusedMapper.capture_bank / run_bank, csrc/map_window_bank.hip) against the per-frame path it stands beside
(capture_window / run_window / set_frame) at 1200 x 680 on the 500 k map of dqo_harness.scenes (config 3), on the same GPU:

    (a) select     GPU time of ONE dqo_window_bank_select launch with both groups changing, and with nothing changing
    (b) set_frame  GPU time of the device copies FusedMapper.set_frame issues for the same parts (camera, targets, render mask, tile
                   mask): as the host issues them, and the same copies replayed from a captured graph (no host in between)
    (c) loop       ms per iteration of run_bank at unroll 1 and 4, beside capture_window + run_window on the same schedule (bench.py's
                   window of five, local_optimize's schedule), run_unroll 1 and 4
    (d) capture    wall time and allocated bytes of capture_bank(40 keyframes), beside capture_window of the same 40

(a) and (b): 50 samples of `--burst` launches between two events each — replayed from one captured graph, so that the host's issue
rate is not what is timed; median, and the spread as min .. max.  (c): five runs of the
schedule each, median and min .. max.  Every part runs in a process of its own under its own time limit; nothing further is started
after a part that fails.

    python tools/profile_window_bank.py [--P 500000] [--limit 280]      # writes profiles/window_bank.txt
"""
import argparse
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))

WINDOW, BANK = 5, 40


def cameras(cam, k, yaw_step, pos_step):
    """k poses along an arc that ends at the configuration's own camera (bench.py's window_cameras at yaw_step 2.5, pos_step 0.06)."""
    from dqo_harness import scenes
    out = []
    for j in range(k):
        back = k - 1 - j
        out.append(scenes.replica_camera(W=cam.W, H=cam.H, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, yaw=12.0 - yaw_step * back,
                                         pitch=4.0 + 0.2 * yaw_step * back, pos=(0.3 - pos_step * back, 0.1, -1.85 + 0.5 * pos_step * back)))
    return out


def problem(P, k, yaw_step=2.5, pos_step=0.06):
    import torch
    from dqo_harness import mapping, scenes, sharding
    if not torch.cuda.is_available():
        raise SystemExit("profile_window_bank: needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda")
    cam, scene = scenes.make_config(3, P=P)
    frames = []
    for c in cameras(cam, k, yaw_step, pos_step):
        st = mapping.make_settings(c, dev)
        tgt = mapping.perturbed_target(scene, st, dev, 107)
        mask = tgt["pix_obj"] >= 0
        frames.append(dict(settings=st, gt_color=tgt["gt_color"].contiguous(), gt_depth=tgt["gt_depth"].contiguous(),
                           render_mask=mask.to(torch.uint8).contiguous(),
                           tile_mask=torch.tensor(sharding.tile_mask_from_pixel_mask(mask.cpu().numpy()), device=dev)))
    return torch, dev, cam, scene, frames


def spread(xs, unit="us", scale=1e3):
    xs = [x * scale for x in xs]
    return f"median {statistics.median(xs):9.2f} {unit}   min .. max {min(xs):9.2f} .. {max(xs):9.2f}   ({len(xs)} samples)"


def timed_bursts(torch, issue, burst, samples=50, before=None):
    """GPU time per call of `issue` in ms: `samples` bursts of `burst` calls between two events (before: run ahead of each burst, untimed)."""
    out = []
    for _ in range(samples + 3):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            issue()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / burst)
    return out[3:]


def part_select(a):
    import _dqo_native as N
    torch, dev, cam, scene, frames = problem(a.P, 2)
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(scene, frames[-1]["settings"], dev)
    fm.begin_mapping_call(reset_optimizer=True)
    fm.capture_bank(frames, loss_tap=True, fused_tail=True)
    bank, g = fm._bank, fm._bank.graph
    stream = N.current_stream()
    print(f"device: {torch.cuda.get_device_name(0)}   P = {a.P}   {cam.W} x {cam.H}   bytes of a keyframe without a gate: "
          f"{sum(getattr(bank, n)[0].numel() * getattr(bank, n)[0].element_size() for n in ('camera', 'gt_color', 'gt_depth', 'render_mask', 'tile_mask'))}")

    def armed(entries):
        def arm():
            bank.schedule[:len(entries)].copy_(torch.tensor(entries, dtype=torch.int32).reshape(-1, 2))
            bank.arm(len(entries), stream)
        return arm

    # (launches issued one by one from the host are bound by the host's issue rate, about 16 us each here: the GPU time of a launch is
    # taken from a captured graph of `burst` of them, as (b)'s second figure is)
    select = lambda: bank.select(g, stream)
    selects = torch.cuda.CUDAGraph()
    with torch.cuda.graph(selects):
        for _ in range(a.burst):
            bank.select(g, N.current_stream())
    both = timed_bursts(torch, selects.replay, 1, before=armed([(i % 2, i % 2) for i in range(a.burst)]))
    none = timed_bursts(torch, selects.replay, 1, before=lambda: (armed([(0, 0)] * (a.burst + 1))(), select()))
    both, none = [t / a.burst for t in both], [t / a.burst for t in none]
    print("(a) dqo_window_bank_select, both groups change      " + spread(both))
    print("(a) dqo_window_bank_select, nothing changes         " + spread(none))
    # (b) the per-frame path's way to the same end: set_frame on a captured frame
    fm2 = FusedMapper(scene, frames[-1]["settings"], dev)
    fm2.begin_mapping_call(reset_optimizer=True)
    fm2.capture_window([frames[0]], loss_tap=True, fused_tail=True)
    turn = [0]

    def set_frame():
        fr = frames[turn[0] % 2]
        turn[0] += 1
        fm2.set_frame(0, gt_color=fr["gt_color"], gt_depth=fr["gt_depth"], render_mask=fr["render_mask"], tile_mask=fr["tile_mask"],
                      settings=fr["settings"])

    host = timed_bursts(torch, set_frame, a.burst)
    print("(b) set_frame's eight device copies, host-issued    " + spread(host))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        set_frame()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        for _ in range(a.burst):
            set_frame()
    replayed = [t / a.burst for t in timed_bursts(torch, graph.replay, 1)]
    print("(b) the same eight copies, one captured graph       " + spread(replayed))
    ok = statistics.median(both) <= statistics.median(replayed)
    print(f"    (a, both groups) <= (b, captured): {ok}   ({statistics.median(both) * 1e3:.2f} us against {statistics.median(replayed) * 1e3:.2f} us; "
          f"against the host-issued copies {statistics.median(host) * 1e3:.2f} us)")


def part_loop(a):
    torch, dev, cam, scene, frames = problem(a.P, WINDOW)
    from dqo_harness.fused_mapping import FusedMapper
    sched = FusedMapper.window_schedule(a.iters, WINDOW, random.Random(0))
    print(f"(c) window of {WINDOW}, local_optimize's schedule of {a.iters} iterations (random.Random(0)), check_every 64, five runs each")
    res = {}
    for kind, unroll in (("window", 1), ("bank", 1), ("window", 4), ("bank", 4)):
        fm = FusedMapper(scene, frames[-1]["settings"], dev)
        fm.begin_mapping_call(reset_optimizer=True)
        if kind == "bank":
            fm.capture_bank(frames, loss_tap=True, fused_tail=True, unroll=unroll)
            run = lambda: fm.run_bank(sched)
        else:
            fm.capture_window(frames, loss_tap=True, fused_tail=True, run_unroll=unroll)
            run = lambda: fm.run_window(sched)
        run()
        ts, redone = [], 0
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / len(sched))
            redone += len(r) if isinstance(r, list) else int(r)
        res[(kind, unroll)] = ts
        name = f"capture_bank + run_bank, unroll {unroll}" if kind == "bank" else f"capture_window + run_window, run_unroll {unroll}"
        print(f"(c) {name:48s} ms per iteration: " + spread(ts, "ms", 1e3) + ("" if not redone else f"   RETRIES / RE-CAPTURES: {redone}"))
        del fm, run
        torch.cuda.empty_cache()
    w, b = res[("window", 1)], res[("bank", 1)]
    print(f"    unroll 1: bank - per-frame = {(statistics.median(b) - statistics.median(w)) * 1e6:.2f} us per iteration; the per-frame figure's "
          f"run-to-run spread {(max(w) - min(w)) * 1e6:.2f} us")


def part_capture(a):
    torch, dev, cam, scene, frames = problem(a.P, BANK, yaw_step=0.6, pos_step=0.015)
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(scene, frames[-1]["settings"], dev)
    fm.begin_mapping_call(reset_optimizer=True)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    if a.part == "capture_bank":
        fm.capture_bank(frames, loss_tap=True, fused_tail=True)
    else:
        fm.capture_window(frames, loss_tap=True, fused_tail=True)
    torch.cuda.synchronize()
    dt, dm = time.perf_counter() - t0, torch.cuda.memory_allocated() - m0
    name = f"capture_bank({BANK} keyframes)" if a.part == "capture_bank" else f"capture_window({BANK} frames)"
    print(f"(d) {name:32s} wall {dt:8.3f} s   allocated {dm / 2**20:10.1f} MiB   (the {BANK} keyframes' own images, which both are given: "
          f"{sum(t.numel() * t.element_size() for fr in frames for t in fr.values() if torch.is_tensor(t)) / 2**20:.1f} MiB)")


PARTS = dict(select=part_select, loop=part_loop, capture_bank=part_capture, capture_window=part_capture)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500000)
    ap.add_argument("--burst", type=int, default=10, help="launches between two events of (a) and (b)")
    ap.add_argument("--iters", type=int, default=400, help="iterations of (c)'s schedule")
    ap.add_argument("--limit", type=int, default=280, help="seconds a part may take")
    ap.add_argument("--part", choices=sorted(PARTS), default=None, help="(internal) run one part in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bank.txt"))
    a = ap.parse_args()
    if a.part:
        return PARTS[a.part](a)
    lines = []
    for name in ("select", "loop", "capture_bank", "capture_window"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--part", name, "--P", str(a.P), "--burst", str(a.burst),
               "--iters", str(a.iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"profile_window_bank: part {name} ended with status {r.returncode}; nothing further was started")
        lines += [l for l in r.stdout.splitlines() if l.startswith(("device:", "(a)", "(b)", "(c)", "(d)", "    "))]
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.stdout.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
