"""The op pair on cfg 3 with each entry: rasterize_gaussians fed with torch's activated copies (what DQO-MAP's render.py does) against
rasterize_gaussian_params fed with the raw parameters.      python tools/profile_op_params.py [--pairs N] [--no-captured]
'deferred' mode on pooled contexts, the two entries alternated in blocks in one process.  Per entry: GPU milliseconds per forward +
backward pair (events around a block), the library's launches per pair (dqo_profile_collect) and, unless --no-captured, iter/s of the
reference loop (render, masked_mapping_loss, backward, DqoAdam(capturable=True)) captured in one torch.cuda.graph.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/profile_op_params.py --pairs 50 --no-captured` for every kernel per pair, torch's
included (the stats count 2 x 3 warm-up + 2 x pairs pairs)."""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + "/dqo-map_amd"]
import torch
import bench
import _dqo_native as N
import diff_gaussian_rasterization_depth as dgr
from dqo_harness import fused_ops, mapping

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=200)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--no-captured", action="store_true")
a = ap.parse_args()

args = argparse.Namespace(cfg=3, P=None, view="room", scaling="strong", shard_by="work", no_object_gate=True, as_shard=None)
dev = torch.device("cuda")
prob = bench.build_problem(args, 0, 1, dev)
params = mapping.GaussianParams({k: v for k, v in prob["scene"].items() if k != "normals"}, dev)
st, tm = prob["settings"], prob["tile_mask"]
gC, gD = torch.randn(3, st.image_height, st.image_width, device=dev), torch.randn(1, st.image_height, st.image_width, device=dev)


def render(entry):
    p = params
    if entry == "activated":
        act = p.activated()
        return dgr.rasterize_gaussians(act["xyz"], act["shs"], torch.empty(0, device=dev), act["opacity"], act["scales"], act["rotations"],
                                       torch.empty(0, device=dev), tm, st)
    return dgr.rasterize_gaussian_params(p._xyz, p._features_dc, p._features_rest, p._opacity, p._scaling, p._rotation, tm, st)


def pair(entry):
    out = render(entry)
    torch.autograd.backward([out[0], out[1]], [gC, gD])
    for grp in params.param_groups():
        grp["params"][0].grad = None


dgr.set_sync_mode("deferred")
for e in ("activated", "params"):
    for _ in range(3):
        pair(e)
dgr.verify_pending()
res = {e: dict(ms_per_pair=[]) for e in ("activated", "params")}
for _ in range(a.blocks):
    for e in ("activated", "params"):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.pairs):
            pair(e)
        t1.record()
        torch.cuda.synchronize()
        res[e]["ms_per_pair"].append(round(t0.elapsed_time(t1) / a.pairs, 4))
        dgr.verify_pending()
for e in ("activated", "params"):
    N.profile_enable(True)
    N.profile_collect(reset=True)
    pair(e)
    torch.cuda.synchronize()
    prof = N.profile_collect(reset=True)
    N.profile_enable(False)
    res[e]["library_launches"] = {k: v[1] for k, v in prof.items()}
    res[e]["library_us"] = {k: round(v[0] * 1e3, 1) for k, v in prof.items()}
    dgr.verify_pending()

if not a.no_captured:
    rng = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        tgt = render("activated")
    gt_c, gt_d = tgt[0].clone(), tgt[1].clone()
    mask = (torch.rand(st.image_height, st.image_width, device=dev, generator=rng) < 0.8) & (tgt[3][0] >= 0)
    for e in ("activated", "params"):
        opt = fused_ops.DqoAdam(params.param_groups(), lr=0.0, eps=1e-15, capturable=True)

        def iteration():
            r = render(e)
            out = {"render": r[0], "depth": r[1], "depth_index_map": r[3]}
            loss, _ = fused_ops.masked_mapping_loss(out, gt_c, gt_d, mask)
            loss.backward()
            opt.step()

        cap = fused_ops.CapturedIteration(iteration, opt, warmup=3)
        for _ in range(20):
            cap.replay()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        n = 500
        for _ in range(n):
            cap.replay()
        t1.record()
        torch.cuda.synchronize()
        cap.check()
        res[e]["captured_iter_per_s"] = round(n * 1e3 / t0.elapsed_time(t1), 1)
        del cap
dgr.set_sync_mode("exact")
print(json.dumps(res))
