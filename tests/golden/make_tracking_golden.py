"""Generates tests/golden/tracking_golden.npz by importing the REFERENCE modules /root/reference/SLAM/utils.py and SLAM/icp.py in the
authoring container (CPU, no GPU) and running the tracker's per-frame chain on seeded synthetic depth frames:

  - the geometry half of Tracker.map_preprocess (SLAM/multiprocess/tracker.py:135-156), restated as glue around the reference's own
    bilateralFilter_torch / compute_vertex_map / compute_normal_map / compute_confidence_map, with the depth filter off and on;
  - IcpTracker.update_curr_status's vertex / normal pyramids (ImagePyramids "max", build_vertex_pyramid, build_normal_pyramid);
  - IcpTracker.update_last_status's model-depth fill;
  - IcpTracker.predict_pose over a frame pair, with icp_use_model_depth true and false.

Only runs where /root/reference exists; the produced .npz (inputs + expected outputs = data) is committed, the reference source never is.
The modules are loaded as in make_icp_golden.py.  compute_confidence_map and predict_pose move tensors with `.cuda()`; inside
`cpu_only()` that method returns the tensor itself, so they run on the CPU unchanged.  predict_pose ends in a `print`; its p2p loss
is recomputed here with the reference's point2plane_loss on the same operands.  Inputs are float16-exact to keep the fixture small.
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

from make_icp_golden import import_reference_icp

ARGS = dict(icp_downscales=[0.25, 0.5, 1.0], icp_downscale_iters=[5, 5, 5], icp_damping=1e-4, icp_distance_threshold=0.1,
            icp_normal_threshold=20, icp_sample_distance_threshold=0.01, icp_sample_normal_threshold=0.01, icp_warmup_frames=0,
            verbose=False)
FAIL_THRESH = (0.02, 1.0)  # base.yaml's threshold fails this pixel-aligned loss; the second case passes
MIN_DEPTH, MAX_DEPTH, CONF_THRESH = 0.3, 5.0, 0.2
SIZES = ((48, 64), (36, 60))


@contextlib.contextmanager
def cpu_only():
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = saved


def raycast(H, W, K, c2w, rng):
    """Depth of the height field z = 2.4 + 0.35 sin(x / 0.45) + 0.25 cos(y / 0.6) + 0.15 sin((x + y) / 0.3) seen by a camera at c2w,
    with holes and a few far / near outliers so that the range mask and the min / max rule have work to do."""
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_c = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones_like(jj)], -1)
    R, C = c2w[:3, :3].astype(np.float64), c2w[:3, 3].astype(np.float64)
    d_w = d_c @ R.T
    f = lambda x, y: 2.4 + 0.35 * np.sin(x / 0.45) + 0.25 * np.cos(y / 0.6) + 0.15 * np.sin((x + y) / 0.3)
    s = np.full((H, W), 2.0)
    for _ in range(60):
        x, y = C[0] + s * d_w[..., 0], C[1] + s * d_w[..., 1]
        s = (f(x, y) - C[2]) / d_w[..., 2]
    depth = s  # d_c has unit z: the ray parameter is the camera-frame depth
    depth[rng.uniform(size=(H, W)) < 0.03] = 0.0
    depth[rng.uniform(size=(H, W)) < 0.004] = 6.0
    depth[rng.uniform(size=(H, W)) < 0.004] = 0.2
    return depth.astype(np.float16).astype(np.float32)


def frame_geometry(u, depth, K, smooth):
    """The geometry of one frame as the reference's tracker prepares it (tracker.py:135-156), composed here from the reference's own
    map functions: returns {depth, vertex, normal, conf, invalid} with every map cleared at the invalid pixels."""
    d = u.bilateralFilter_torch(depth.clone(), 5, 2, 2) if smooth else depth.clone()
    d = torch.where((d > MIN_DEPTH) & (d < MAX_DEPTH), d, torch.zeros_like(d))
    maps = {"depth": d, "vertex": u.compute_vertex_map(d, K)}
    maps["normal"] = u.compute_normal_map(maps["vertex"])
    with cpu_only():
        maps["conf"] = u.compute_confidence_map(maps["normal"], K)
    no_normal = (maps["normal"] == 0).all(dim=-1)
    maps["invalid"] = no_normal | (maps["conf"][..., 0] < CONF_THRESH)
    keep = (~maps["invalid"])[..., None]
    for name in ("depth", "vertex", "normal", "conf"):
        maps[name] = maps[name] * keep
    return maps


def main():
    icp = import_reference_icp()
    u = sys.modules["SLAM.utils"]
    rng = np.random.default_rng(20251016)
    out = {}
    for ci, (H, W) in enumerate(SIZES):
        K = np.array([[W * 0.8, 0, (W - 1) / 2.0], [0, W * 0.8, (H - 1) / 2.0], [0, 0, 1]], np.float32)
        Kt = torch.from_numpy(K)
        c2w0 = np.eye(4)
        ang = 0.02
        c2w1 = np.eye(4)
        c2w1[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        c2w1[:3, 3] = [0.03, -0.01, 0.02]
        d0, d1 = raycast(H, W, K, c2w0, rng), raycast(H, W, K, c2w1, rng)
        out[f"c{ci}_K"], out[f"c{ci}_depth0_f16"], out[f"c{ci}_depth1_f16"] = K, d0.astype(np.float16), d1.astype(np.float16)
        out[f"c{ci}_c2w1"] = c2w1.astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        for filt in (0, 1):
            pp = frame_geometry(u, t(d0)[..., None], Kt, bool(filt))
            # size: with the filter on only depth and mask are kept (the rest is the same code on that depth); the vertex map of
            # the filter-off run is the finest pyramid level's (compute_vertex_map of the same depth map)
            for k in (("depth", "normal", "conf", "invalid") if filt == 0 else ("depth", "invalid")):
                out[f"c{ci}_pre{filt}_{k}"] = pp[k].numpy()
        f0 = frame_geometry(u, t(d0)[..., None], Kt, False)
        f1 = frame_geometry(u, t(d1)[..., None], Kt, False)
        # model depth: the frame-0 depth disturbed as a render would be (noise, holes, a bent normal patch)
        render_depth = f0["depth"].clone()
        noise = rng.normal(scale=0.02, size=(H, W, 1)).astype(np.float32)
        render_depth = (render_depth + t(noise)).to(torch.float16).to(torch.float32)
        render_depth[t(rng.uniform(size=(H, W)) < 0.05)] = 0.0
        render_normal = f0["normal"].clone()
        render_normal[H // 3:H // 2, W // 4:W // 2] = torch.tensor([0.0, 0.6, -0.8])
        render_normal = render_normal.to(torch.float16).to(torch.float32)
        out[f"c{ci}_render_depth_f16"] = render_depth.numpy().astype(np.float16)
        out[f"c{ci}_render_normal_f16"] = render_normal.numpy().astype(np.float16)
        for use_model in (0, 1):
            args = types.SimpleNamespace(**ARGS, icp_use_model_depth=bool(use_model), icp_fail_threshold=FAIL_THRESH[ci])
            tr = icp.IcpTracker(args)
            tr.update_curr_status(f0["depth"], Kt)
            if use_model == 0:
                for L in range(3):
                    out[f"c{ci}_pyr_vertex{L}"] = tr.vertex_pyramid_t1[L].numpy()
                    out[f"c{ci}_pyr_normal{L}"] = tr.normal_pyramid_t1[L].numpy()
                    if L < 2:  # size: the coarse levels keep z only (= the max-pooled depth); x, y follow from it and K
                        out[f"c{ci}_pyr_vertex{L}"] = out[f"c{ci}_pyr_vertex{L}"][..., 2]
            tr.move_last_status()
            rd = render_depth.clone()
            tr.update_last_status(types.SimpleNamespace(get_intrinsic=Kt), rd, f0["depth"], render_normal, f0["normal"])
            if use_model == 1:
                out[f"c{ci}_filled_depth"] = rd.numpy()
            tr.update_curr_status(f1["depth"], Kt)
            # predict_pose returns the pose and the flag; its valid ratio stays local, so the last level's ICP is instrumented
            ratios = []
            orig = icp.ICP.icp

            def icp_spy(self, *a, **k):
                pose, ratio = orig(self, *a, **k)
                ratios.append(float(ratio))
                return pose, ratio
            icp.ICP.icp = icp_spy
            try:
                with cpu_only(), contextlib.redirect_stdout(open(os.devnull, "w")):
                    pose, ok = tr.predict_pose({"K": Kt, "frame_id": 1})
            finally:
                icp.ICP.icp = orig
            pt = torch.from_numpy(pose).float()
            loss = icp.point2plane_loss(tr.vertex_pyramid_t0[-1], tr.vertex_pyramid_t1[-1] @ pt[:3, :3].T + pt[:3, 3], tr.normal_pyramid_t0[-1])
            out[f"c{ci}_m{use_model}_pose"] = pose.astype(np.float32)
            out[f"c{ci}_m{use_model}_success"] = np.bool_(ok)
            out[f"c{ci}_m{use_model}_loss"] = np.float32(loss)
            out[f"c{ci}_m{use_model}_valid_ratio"] = np.float32(ratios[-1])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracking_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    for ci in range(2):
        for m in range(2):
            print(ci, m, out[f"c{ci}_m{m}_success"], out[f"c{ci}_m{m}_loss"], out[f"c{ci}_m{m}_valid_ratio"])
            print(out[f"c{ci}_m{m}_pose"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
