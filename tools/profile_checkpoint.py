"""Times a map checkpoint — the six files of gaussian_map.save_model (SLAM/multiprocess/mapper.py:1580-1608) — on the maps of
dqo_harness.scenes' config 3 (500 k Gaussians, 16 SH coefficients) and on a 2 M map, two ways on the same GPU:

    (a) indexed   what a caller had to do before FusedMapper.save_model existed: per cloud index every buffer by its mask in torch, .cpu(),
                  and dqo_ply.save_model_ply for the file with and the file without the confidence column; the merged files from the two
                  clouds' host arrays concatenated (cheaper than the reference's merge_ply, which reads the two files back)
    (b) packed    FusedMapper.save_model, and its three parts timed apart: pack (dqo_map_pack_rows, both column sets), the device-to-host
                  copies into the pinned staging buffer, the file writes

and the two kernels' times from the library's own event brackets, with the pack kernel's achieved bandwidth over its own traffic (the
bytes it has to move, computed from the shapes and the masks — not a counter).  The map has an eighth of its rows spare and half of its
Gaussians stable, so all six files are written.  The two ways alternate, `--reps` times; the wall times end in a synchronisation.
Files go to --dir (default: a fresh temporary directory, removed at the end); what the write costs depends on that file system.

Each size runs in a process of its own under its own time limit; the next is not started if one fails.

    python tools/profile_checkpoint.py [--sizes 500000 2000000] [--reps 5] [--limit 420]      # writes profiles/checkpoint.txt
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))


def one_size(P, reps, where):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("profile_checkpoint: needs a GPU (there is nothing to time without one)")
    import _dqo_native as N
    import dqo_ply
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam, scene = scenes.make_config(3, P=P)
    fm = FusedMapper(scene, mapping.make_settings(cam, dev), dev)
    fm.reserve(P // 8)
    g = torch.Generator(device="cpu").manual_seed(1)
    fm._free_rows(torch.nonzero((torch.rand((fm.P,), generator=g) < 0.02).to(dev) & (fm.alive != 0)).reshape(-1))  # holes among the live rows
    fm.track_lifecycle(stable_mask=(torch.rand((fm.P,), generator=g) < 0.5).to(dev))
    fm.confidence.copy_(torch.rand((fm.P,), generator=g).to(dev) * 700 * (fm.alive != 0))
    M, rows = fm.M, fm.P
    prefix = os.path.join(where, "iter")

    def clean():
        for f in os.listdir(where):
            os.remove(os.path.join(where, f))

    def indexed():
        live, st = fm.alive != 0, fm.stable != 0
        host = []
        for sel in (live & ~st, live & st):
            host.append([a[sel].cpu().numpy() for a in (fm.xyz, fm.shs, fm.opacity_raw, fm.scaling_raw, fm.rotation_raw, fm.confidence)])
        merged = [np.concatenate([a, b]) for a, b in zip(*host)]
        for tag, with_conf in (("", True), ("_sibr", False)):
            for name, arrays in ((prefix + tag + ".ply", host[0]), (prefix + "_stable" + tag + ".ply", host[1]),
                                 (prefix + "_merge" + tag + ".ply", merged)):
                dqo_ply.save_model_ply(name, *arrays, include_confidence=with_conf)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def parts():
        """save_model's steps, one timed after the other (the same calls in the same order)."""
        t = dict(pack=0.0, copy=0.0, write=0.0)
        k = fm._checkpoint
        n = rows
        for with_conf, tag in ((True, ""), (False, "_sibr")):
            C = 6 + 3 * M + 8 + (1 if with_conf else 0)
            out = []
            t["pack"] += wall(lambda: out.append(fm.pack_rows(include_confidence=with_conf)))
            table, header = out[0]

            def copy():
                k["host"][:n * C].copy_(table.view(-1)[:n * C], non_blocking=True)
                k["host_header"].copy_(header, non_blocking=True)
            t["copy"] += wall(copy)
            U, S = int(k["host_header"][0]), int(k["host_header"][1])
            n = U + S
            part = k["host"][:n * C].view(n, C)
            t0 = time.perf_counter()
            for name, p in ((prefix + tag + ".ply", part[:U]), (prefix + "_stable" + tag + ".ply", part[U:]), (prefix + "_merge" + tag + ".ply", part)):
                dqo_ply.write_vertex_table(name, p, 3 * (M - 1), with_conf)
            t["write"] += (time.perf_counter() - t0) * 1e3
        return t, (U, S)

    with torch.no_grad():
        # warm-up of every shape: both ways once (this also allocates save_model's buffers), and the files must agree
        indexed()
        want = {f: open(os.path.join(where, f), "rb").read() for f in sorted(os.listdir(where))} if rows <= 700000 else None
        sizes = {f: os.path.getsize(os.path.join(where, f)) for f in sorted(os.listdir(where))}
        clean()
        written = fm.save_model(prefix)
        assert sorted(os.path.basename(f) for f in written) == sorted(sizes), (sorted(written), sorted(sizes))
        for f in sizes:
            assert os.path.getsize(os.path.join(where, f)) == sizes[f], f
            if want is not None:
                assert open(os.path.join(where, f), "rb").read() == want[f], f
        del want
        clean()
        ta, tb, tp = [], [], []
        for rep in range(reps):
            print(f"profile_checkpoint: P = {P}, pass {rep + 1} of {reps}", file=sys.stderr, flush=True)
            ta.append(wall(indexed))
            clean()
            tb.append(wall(lambda: fm.save_model(prefix)))
            clean()
            p, (U, S) = parts()
            tp.append(p)
            clean()
        # the kernels alone
        N.profile_enable(True)
        N.profile_collect(reset=True)
        kreps = 20
        for _ in range(kreps):
            fm.pack_rows(include_confidence=True)
        prof = N.profile_collect(reset=True)
        N.profile_enable(False)
    C = 6 + 3 * M + 9
    quarters = torch.nn.functional.pad(fm.alive, (0, (-rows) % 64)).view(-1, 64).any(1).sum().item()
    moved = quarters * 64 * (12 + 3 * M) * 4 + (U + S) * C * 4 + 2 * rows + 2 * rows  # rows loaded, rows stored, the flags read by both kernels
    med = statistics.median
    rng = lambda ts: f"{med(ts):9.1f}  ({min(ts):.1f} .. {max(ts):.1f})"
    print(f"device: {torch.cuda.get_device_name(0)}   rows = {rows} ({U} unstable + {S} stable Gaussians, {rows - U - S} spare)   M = {M}   "
          f"six files, {sum(sizes.values()) / 1e6:.0f} MB, in {'a temporary directory' if where.startswith(tempfile.gettempdir()) else where}")
    print(f"P = {P}: ms per checkpoint, median of {reps} (min .. max), the two ways alternating")
    print(f"  (a) indexed: torch index + .cpu() + save_model_ply   {rng(ta)}")
    print(f"  (b) packed:  FusedMapper.save_model                  {rng(tb)}")
    for key, what in (("pack", "pack_rows, both column sets"), ("copy", "device-to-host copies"), ("write", "file writes")):
        print(f"      its parts, timed apart: {what:30s} {rng([p[key] for p in tp])}")
    for name in ("map_pack_count_kernel", "map_pack_rows_kernel"):
        ms, calls = prof[name]
        line = f"  {name:24s} {1e3 * ms / calls:8.1f} us per launch ({calls} launches, with the confidence column)"
        if name == "map_pack_rows_kernel":
            line += f"; {moved / 1e6:.0f} MB of its own traffic: {moved / (ms / calls * 1e-3) / 1e12:.2f} TB/s"
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500000, 2000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a fresh temporary directory)")
    ap.add_argument("--one", type=int, default=None, help="(internal) run one size in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint.txt"))
    a = ap.parse_args()
    if a.one:
        where = tempfile.mkdtemp(prefix="dqo_checkpoint_", dir=a.dir)
        try:
            return one_size(a.one, a.reps, where)
        finally:
            shutil.rmtree(where, ignore_errors=True)
    lines = []
    for P in a.sizes:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(P), "--reps", str(a.reps)]
        if a.dir:
            cmd += ["--dir", a.dir]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # (its progress lines go to this process's stderr)
        if r.returncode != 0:
            raise SystemExit(f"profile_checkpoint: P = {P} ended with status {r.returncode}; nothing further was started")
        lines += r.stdout.splitlines()
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        with open(a.out, "w") as f:  # (what is done so far, should a later size fail)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
