"""A/B of FusedMapper's whole-map operators between two versions of the PYTHON beside one libdqoraster.so (the split of
dqo_harness/fused_mapping.py into the core and dqo_harness/map_operators.py changed no kernel): the same fixed-seed job on both sides,

    a window of two frames captured, eight replays, then every operator twice — the first call sizes its scratch, the second is the
    steady state — and `--reps` more calls of each for the host's time,

and per side
  * sha1 of every tensor an operator returned (both calls), of fm._maintain_ctx.out after each, of every row buffer at the end, of the
    parameters, moments and loss after the replays, and of the bytes of every file written;
  * per operator the change of torch.cuda.memory_stats()["allocation.all.allocated"] over its SECOND call (the parent's number is the
    yardstick, not zero: refresh_window makes a temporary for ~rows);
  * per operator the host's wall time of a call issued on an idle stream (the stream is drained before and after; operators that
    synchronise themselves — the checkpoints — include what they wait for).
The sides alternate, `--rounds` times each, every run in a process of its own under its own time limit; nothing further is started once
one fails.  Ends with status 1 if a hash or an allocation count differs; a change's median outside the parent's min .. max is reported.

    python tools/ab_map_operators.py --old PARENT/dqo-map_amd/dqo_harness/fused_mapping.py      # writes profiles/map_operators_split.txt
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_side(old, reps, where):
    if old:  # dqo_harness is a namespace package: a directory in front that holds only the parent's fused_mapping.py shadows this tree's
        os.makedirs(os.path.join(where, "old", "dqo_harness"))
        shutil.copy(old, os.path.join(where, "old", "dqo_harness", "fused_mapping.py"))
        sys.path.insert(0, os.path.join(where, "old"))
    sys.path.insert(1 if old else 0, os.path.join(ROOT, "dqo-map_amd"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ab_map_operators: needs a GPU")
    import dqo_eval
    from dqo_harness import fused_mapping, mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    assert os.path.dirname(fused_mapping.__file__).startswith(where if old else ROOT), fused_mapping.__file__
    dev = torch.device("cuda")
    hashes, allocs, times = {}, {}, {}
    RENDERED = (0, 1, 2, 3, 6, 7)  # the outputs the operators read: colour, depth, the two hit indices, T_map, n_touched

    def h(*ts):
        m = hashlib.sha1()
        for t in ts:
            m.update(t.detach().contiguous().cpu().numpy().tobytes() if torch.is_tensor(t) else t)
        return m.hexdigest()[:16]

    def flat(r):
        """The tensors (and file contents) of what an operator returned, in a fixed order."""
        if torch.is_tensor(r):
            return [r]
        if isinstance(r, dict):
            return [x for k in sorted(r, key=str) for x in flat(r[k])]
        if isinstance(r, (tuple, list)):
            return [x for v in r for x in flat(v)]
        if isinstance(r, dqo_eval.TsdfVolume):
            return [r.tsdf, r.weight, r.color]
        return [repr(r).encode()]

    def files():
        out = []
        for f in sorted(os.listdir(where)):
            p = os.path.join(where, f)
            if os.path.isfile(p) and f.endswith(".ply"):
                out += [f.encode(), open(p, "rb").read()]
        return out

    def run(name, f, wrote_files=False, view=lambda r: r):
        """f() twice (hashes of view(what it returned); the second call's allocation count), then `reps` more for the host's time."""
        for call in (1, 2):
            torch.cuda.synchronize()
            n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            r = f()
            n1 = torch.cuda.memory_stats()["allocation.all.allocated"]
            torch.cuda.synchronize()
            hashes[f"{name} call {call}"] = h(*flat(view(r)), *(files() if wrote_files else []))
            if fm._maintain_ctx is not None:
                hashes[f"{name} call {call}: _maintain_ctx.out"] = h(*[fm._maintain_ctx.out[i] for i in RENDERED])
            if call == 2:
                allocs[name] = n1 - n0
            del r
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
        if ts:
            times[name] = ts

    P = 20000
    cam, scene = scenes.make_config(3, P=P)
    settings = mapping.make_settings(cam, dev)
    with torch.no_grad():
        tgt = mapping.render(settings, mapping.GaussianParams(scene, dev).activated())
    gt_color, gt_depth = tgt["render"].clone(), tgt["depth"].clone()
    H, W = gt_depth.shape[-2:]
    gt_d = gt_depth.clone()
    gt_d[:, :H // 3] += 0.5 * (gt_d[:, :H // 3] > 0)
    gt_c = gt_color.clone()
    gt_c[:, 2 * H // 3:] += 0.3
    gen = torch.Generator(device="cpu").manual_seed(1)
    fm = FusedMapper(scene, settings, dev).reserve(P // 8)
    fm.track_lifecycle(stable_mask=(torch.rand((fm.P,), generator=gen) < 0.5).to(dev), tick=0, frame_id=3)
    fm.frame_id[:P] = (3 + torch.arange(P, device=dev) % 4).to(torch.int32)
    fm.set_training_rows(trainable=~fm.stable_rows())
    fm.begin_mapping_call()
    tiles = ((H + 15) // 16, (W + 15) // 16)
    window = [dict(gt_color=c, gt_depth=d, settings=settings, render_mask=(torch.rand((H, W), generator=gen) < 0.6).to(dev),
                   tile_mask=torch.ones(tiles, dtype=torch.int32, device=dev)) for c, d in ((gt_color, gt_depth), (gt_c, gt_d))]
    fm.capture_window(window, capacity_margin=2.0)
    for k in range(8):
        fm.replay(frame=k % 2)
    torch.cuda.synchronize()
    assert not fm.graph_overflowed(fm._frames[0]) and not fm.graph_overflowed(fm._frames[1])
    hashes["capture + 8 replays: parameters, moments, loss"] = h(*[v for _, v in sorted(fm._params().items())],
                                                                 *[m for _, ms in sorted(fm.state.items()) for m in ms], fm.loss)

    rng = np.random.default_rng(0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    frame_map = dict(depth_map=gt_d.permute(1, 2, 0).contiguous(), color_map=gt_c.permute(1, 2, 0).contiguous(),
                     vertex_map_w=up(rng.uniform(-3, 3, (H, W, 3))), normal_map_w=up(rng.normal(size=(H, W, 3))), instance_img=None)
    frames = [(None, gt_color, gt_depth), (settings, gt_c, gt_d)]
    ms = torch.zeros((2, 20), dtype=torch.float32, device=dev)
    xyz = np.asarray(scene["xyz"], np.float32)
    gt_points = up(xyz[::4] + rng.normal(0, 0.02, (P // 4, 3)))
    gt_object = torch.tensor(np.asarray(scene["obj_id"], np.int32)[::4], device=dev)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    quad = lambda z: (up([[lo[0], lo[1], z], [hi[0], lo[1], z], [hi[0], hi[1], z], [lo[0], hi[1], z]]),
                      torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev))
    mid, low, high = quad(float(np.median(xyz[:, 2]))), quad(float(lo[2])), quad(float(hi[2]))
    vol = dqo_eval.TsdfVolume((float(lo[0]), float(lo[1]), float(lo[2])), float((hi - lo).max()) / 32, (32, 32, 32), 0.3, dev)
    projection = torch.tensor(cam.projection_matrix, dtype=torch.float32, device=dev)
    dens = dict(sample_nums=20000, rows="all")
    th = dict(stable_confidence_thres=2.0, unstable_time_window=100, add_color_thres=0.1, add_depth_thres=0.1, delete_thresh=3)
    prefix = os.path.join(where, "iter")
    tick = [10]

    def maintain():
        tick[0] += 1
        return fm.maintain(tick[0], gt_c, gt_d, **th)

    with torch.no_grad():
        run("refresh_window", lambda: fm.refresh_window())
        run("refresh_window(error mode)", lambda: fm.refresh_window(global_opt=True, sample_ratio=0.4))
        run("sample_new", lambda: (fm.sample_new(frame_map, seed=5, tick=1), fm.sample_header))
        run("evaluate", lambda: fm.evaluate(frames))
        run("evaluate_ms_ssim", lambda: (fm.evaluate_ms_ssim(frames, ms), ms))
        run("make_mesh", lambda: fm.make_mesh([None, settings], vol))
        run("densify", lambda: fm.densify(**dens))
        run("evaluate_geometry", lambda: fm.evaluate_geometry(gt_points, (0.02, 0.05)))
        run("evaluate_geometry_densified", lambda: fm.evaluate_geometry_densified(gt_points, (0.02, 0.05), densify=dens))
        run("evaluate_geometry_mesh", lambda: fm.evaluate_geometry_mesh(*mid, sample_nums=20000, seed=2))
        run("evaluate_geometry_mesh(densify)", lambda: fm.evaluate_geometry_mesh(*low, sample_nums=20000, seed=2, densify=dens))
        run("pack_rows", lambda: fm.pack_rows(), view=lambda r: (r[0][:int(r[1].sum().item())], r[1]))  # (rows behind U + S keep their bytes)
        run("save_model", lambda: fm.save_model(prefix), wrote_files=True)
        fm.set_object_gate(np.concatenate([np.asarray(scene["obj_id"], np.int32), np.zeros(fm.P - P, np.int32)]), np.zeros((H, W), np.int32))
        run("evaluate_geometry_objects", lambda: fm.evaluate_geometry_objects(gt_points, gt_object, (0.02, 0.05)))
        run("evaluate_geometry_objects_mesh", lambda: fm.evaluate_geometry_objects_mesh({1: low, 3: high}, 5000, seed=4))
        run("save_model_objects", lambda: fm.save_model_objects(prefix), wrote_files=True)
        fm.set_object_gate(None, None)
        fm.add_tick[1:P:50] = -200
        run("maintain", maintain)
        run("prune_floaters", lambda: fm.prune_floaters(gt_depth, (4, 6), projection=projection))
        torch.cuda.synchronize()
        assert not fm.maintain_overflowed() and not fm.prune_overflowed()
        fm.save_model(prefix, save_sibr=False, save_merge=False)
        run("load_model", lambda: [a.clone() for _, a in fm.load_model(prefix + ".ply", prefix + "_stable.ply", tick=7)._rows()])
        twin = FusedMapper.from_model_ply(prefix + ".ply", prefix + "_stable.ply", settings, dev, spare_rows=100, tick=7)
        hashes["from_model_ply: row buffers"] = h(*[a for _, a in twin._rows()])
    torch.cuda.synchronize()
    for b, a in fm._rows():
        hashes[f"row buffer {b.name} at the end"] = h(a)
    return dict(file=fused_mapping.__file__, device=torch.cuda.get_device_name(0), hashes=hashes, allocs=allocs, times=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="the parent's dqo_harness/fused_mapping.py")
    ap.add_argument("--reps", type=int, default=20, help="timed calls per operator and run, after the two hashed ones")
    ap.add_argument("--rounds", type=int, default=2, help="runs per side; the sides alternate")
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    ap.add_argument("--side", default=None, help="(internal) run one side in this process and print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_operators_split.txt"))
    a = ap.parse_args()
    if a.side:
        where = tempfile.mkdtemp(prefix="dqo_ab_operators_")
        try:
            print(json.dumps(one_side(a.old if a.side == "parent" else None, a.reps, where)))
        finally:
            shutil.rmtree(where, ignore_errors=True)
        return 0
    if not a.old or not os.path.isfile(a.old):
        raise SystemExit("ab_map_operators: --old must name the parent's dqo_harness/fused_mapping.py")
    runs = {"parent": [], "change": []}
    for rnd in range(a.rounds):
        for side in ("parent", "change"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--side", side, "--old", a.old, "--reps", str(a.reps)]
            print(f"ab_map_operators: round {rnd + 1} of {a.rounds}, {side}", file=sys.stderr, flush=True)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit(f"ab_map_operators: the {side} run ended with status {r.returncode}; nothing further was started")
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    p, c = runs["parent"], runs["change"]
    lines = [f"device: {p[0]['device']}   one libdqoraster.so, {a.rounds} runs per side, alternating",
             f"parent: a copy of {a.old} in front of this tree's dqo_harness", f"change: {os.path.relpath(c[0]['file'], ROOT)}", ""]
    bad = []
    for side, rs in runs.items():  # a side repeats itself bit for bit
        bad += [f"{side} run {i + 1} differs from run 1: {k}" for i, r in enumerate(rs) for k in r["hashes"] if r["hashes"][k] != rs[0]["hashes"].get(k)]
    keys = list(p[0]["hashes"])
    if keys != list(c[0]["hashes"]):
        bad.append("the sides hashed different things")
    lines.append(f"hashes ({len(keys)}): sha1[:16] of the parent | of the change")
    for k in keys:
        hp, hc = p[0]["hashes"][k], c[0]["hashes"].get(k)
        lines.append(f"  {k:62s} {hp} | {hc}{'' if hp == hc else '   DIFFERENT'}")
        if hp != hc:
            bad.append(f"hash differs: {k}")
    lines += ["", "allocations during an operator's second call (allocation.all.allocated): parent | change"]
    for k in p[0]["allocs"]:
        ap_, ac = p[0]["allocs"][k], c[0]["allocs"].get(k)
        lines.append(f"  {k:34s} {ap_:4d} | {ac:4d}{'' if ap_ == ac else '   DIFFERENT'}")
        if ap_ != ac:
            bad.append(f"allocation count differs: {k}")
    lines += ["", f"host time of a call on an idle stream, us, {a.rounds} x {a.reps} calls per side: median (min .. max)"]
    outside = []
    for k in p[0]["times"]:
        tp, tc = [t for r in p for t in r["times"][k]], [t for r in c for t in r["times"][k]]
        ok = statistics.median(tc) <= max(tp)
        lines.append(f"  {k:34s} parent {statistics.median(tp):9.1f} ({min(tp):9.1f} .. {max(tp):9.1f})   change {statistics.median(tc):9.1f} "
                     f"({min(tc):9.1f} .. {max(tc):9.1f})   {'inside the parent range or below' if ok else 'ABOVE the parent range'}")
        if not ok:
            outside.append(k)
    lines += ["", "all hashes and allocation counts equal" if not bad else "NOT EQUAL: " + "; ".join(bad),
              "every median inside the parent's min .. max or below it" if not outside else "medians above the parent's range: " + ", ".join(outside)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
