"""GPU: the tracker's device chain (dqo_icp.preprocess_frame / IcpTracker; csrc/track.hip and the Gauss-Newton kernel of csrc/icp.hip)
against goldens from the reference's own SLAM/utils.py + SLAM/icp.py, against the numpy oracle (tests/tracking_oracle.py) at
tracking resolution, against the host ICP loop, on a rendered frame pair, run to run and under graph capture."""
import types

import numpy as np
import pytest

import tracking_oracle as to
from test_oracle_icp import CASES as ICP_CASES, G as ICP_G, case as icp_case
from test_tracking_oracle import (CASES, CONF_THRESH, FAIL_THRESH, G, MAP_TOL, MAX_DEPTH, MIN_DEPTH, SAMPLE_DIST, SAMPLE_NORMAL, args,
                                  frame_pair, inputs, map_close, mask_close)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trk():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()
    import dqo_icp
    return torch, dqo_icp


def cuda(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def np_(t):
    return t.detach().cpu().numpy()


def check_preprocess(out, ref, golden_depth_only=False, filtered=False):
    inv = np_(out["invalid_confidence_mask"])
    assert mask_close(inv, ref["invalid"])
    flip = inv != np.asarray(ref["invalid"]).reshape(inv.shape)
    assert map_close(np_(out["depth_map"]), ref["depth"], mismatch=flip)
    if not golden_depth_only:
        for k, r in (("normal_map_c", "normal"), ("confidence_map", "conf"), ("vertex_map_c", "vertex")):
            if filtered and k != "vertex_map_c":
                # the filtered depth differs from numpy's by the last bits of exp, and a Sobel normal over fine pixel spacing turns
                # an ulp of depth into ~1e-5: the normal stage itself is held to MAP_TOL by the unfiltered runs; here 1e-3, with
                # ill-conditioned pixels (cancelling cross products) counted like threshold flips
                bad = np.abs(np_(out[k]).reshape(ref[r].shape) - ref[r]).reshape(inv.shape[0], inv.shape[1], -1).max(-1) > 1e-3
                assert (bad & ~flip).mean() <= 2e-3, k
                assert map_close(np_(out[k]), ref[r], tol=1e-3, mismatch=flip | bad), k
                continue
            assert map_close(np_(out[k]), ref[r], mismatch=flip), k


def test_preprocess_vs_goldens_and_oracle(trk):
    torch, M = trk
    for c in CASES:
        x = inputs(c)
        for filt in (0, 1):
            d = cuda(torch, x["depth0"])
            d_before = d.clone()
            out = M.preprocess_frame(d, torch.tensor(x["K"]), MIN_DEPTH, MAX_DEPTH, CONF_THRESH, depth_filter=bool(filt))
            assert torch.equal(d, d_before)  # the input is not modified
            g = {k: G[f"{c}_pre{filt}_{k}"] for k in ("depth", "invalid")}
            if filt == 0:
                g.update(normal=G[f"{c}_pre0_normal"], conf=G[f"{c}_pre0_conf"], vertex=G[f"{c}_pyr_vertex2"])
            check_preprocess(out, g, golden_depth_only=filt == 1)
            check_preprocess(out, to.preprocess(x["depth0"], x["K"], MIN_DEPTH, MAX_DEPTH, CONF_THRESH, depth_filter=bool(filt)),
                             filtered=bool(filt))


def pyramid_on_gpu(torch, M, depth, K, use_model=False):
    tr = M.IcpTracker(args("c0", use_model))
    tr.update_curr_status(cuda(torch, depth), torch.tensor(K))
    torch.cuda.synchronize()
    return tr, [(np_(v), np_(n)) for v, n in zip(tr.vertex_pyramid_t1, tr.normal_pyramid_t1)]


def test_pyramid_vs_goldens(trk):
    torch, M = trk
    for c in CASES:
        _, pyr = pyramid_on_gpu(torch, M, G[f"{c}_pre0_depth"], G[f"{c}_K"])
        for L, (V, Nm) in enumerate(pyr):
            gv = G[f"{c}_pyr_vertex{L}"]
            assert map_close(V if gv.ndim == 3 else V[..., 2], gv), (c, L)
            assert map_close(Nm, G[f"{c}_pyr_normal{L}"]), (c, L)


def test_fill_vs_goldens(trk):
    torch, M = trk
    for c in CASES:
        x = inputs(c)
        tr = M.IcpTracker(args(c, True))
        rd = cuda(torch, x["render_depth"])
        tr.update_last_status(None, rd, cuda(torch, G[f"{c}_pre0_depth"]), cuda(torch, x["render_normal"]), cuda(torch, G[f"{c}_pre0_normal"]))
        assert tr.last_model_depth is rd
        assert mask_close(np_(rd), G[f"{c}_filled_depth"])


def synthetic_depth(H, W, seed):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    z = 2.0 + 0.4 * np.sin(jj / 53.0) + 0.3 * np.cos(ii / 37.0) + 0.5 * (jj > W // 2) + 0.003 * rng.normal(size=(H, W))
    z[rng.uniform(size=(H, W)) < 0.03] = 0.0
    z[rng.uniform(size=(H, W)) < 0.002] = 7.0
    return z.astype(np.float32)


def test_full_resolution_vs_oracle(trk):
    torch, M = trk
    H, W = 680, 1200
    K = np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]], np.float32)
    d = synthetic_depth(H, W, 7)
    for filt in (False, True):
        out = M.preprocess_frame(cuda(torch, d), torch.tensor(K), MIN_DEPTH, MAX_DEPTH, CONF_THRESH, depth_filter=filt)
        check_preprocess(out, to.preprocess(d, K, MIN_DEPTH, MAX_DEPTH, CONF_THRESH, depth_filter=filt), filtered=filt)
    _, pyr = pyramid_on_gpu(torch, M, d, K)
    for (V, Nm), (oV, oN) in zip(pyr, to.pyramid(d, K)):
        assert map_close(V, oV) and map_close(Nm, oN)
    rn = np.random.default_rng(3).normal(size=(H, W, 3)).astype(np.float32)
    rd = cuda(torch, d + 0.02)
    tr = M.IcpTracker(args("c0", True))
    tr.update_last_status(None, rd, cuda(torch, d), cuda(torch, rn), cuda(torch, -rn))
    assert mask_close(np_(rd), to.fill(d + 0.02, d, rn, -rn, SAMPLE_DIST, SAMPLE_NORMAL))


def gauss_newton_on_gpu(torch, M, v0, v1, n0, n1, pose, K, iters, dist, nthr, damping):
    import _dqo_native as N
    lib = N.lib()
    p = cuda(torch, pose).float().contiguous()
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.dqo_icp_workspace_bytes(), dtype=torch.uint8, device="cuda")
    t = [cuda(torch, a) for a in (v0, v1, n0, n1)]
    Kd = cuda(torch, np.asarray(K, np.float32))
    H, W = v0.shape[:2]
    for _ in range(iters):
        N.check(lib.dqo_icp_gauss_newton(H, W, *[N.ptr(a) for a in t], N.ptr(p), N.ptr(Kd), 1.0, dist, nthr, damping, N.ptr(cnt),
                                         N.ptr(ws), ws.numel(), N.current_stream()))
    return p, cnt


def test_device_gauss_newton_vs_host_icp(trk):
    torch, M = trk
    for c in ICP_CASES:
        v0, v1, n0, n1, pose, K = icp_case(c)
        for damping in (1e-4, 1e-6):  # the goldens' damping last
            host = M.ICP(max_iter=3, damping=damping, distance_threshold=0.2, normal_threshold=20)
            hp, ratio = host.icp(cuda(torch, pose), cuda(torch, v0), cuda(torch, v1), cuda(torch, n0), cuda(torch, n1), torch.tensor(K))
            dp, cnt = gauss_newton_on_gpu(torch, M, v0, v1, n0, n1, pose, K, 3, 0.2, float(host.normal_threshold), damping)
            np.testing.assert_allclose(np_(dp), np_(hp), rtol=0, atol=1e-6)
            assert abs(int(cnt) / v0.shape[0] / v0.shape[1] - float(ratio)) < 1e-6
        np.testing.assert_allclose(np_(dp), ICP_G[f"{c}_pose_out"], rtol=0, atol=2e-4)
    # nothing valid (no depth in frame 0): H == 0, xi == 0, the pose stays bit for bit
    v0, v1, n0, n1, pose, K = icp_case(ICP_CASES[0])
    dp, cnt = gauss_newton_on_gpu(torch, M, np.zeros_like(v0), v1, n0, n1, pose, K, 2, 0.2, 0.9, 1e-4)
    assert int(cnt) == 0 and np.array_equal(np_(dp), pose)


def run_pair(torch, M, c, use_model, fail=None):
    """The golden frame pair through preprocess_frame -> update_curr_status / move_last_status / update_last_status -> predict_pose."""
    x = inputs(c)
    K = torch.tensor(x["K"])
    a = args(c, use_model)
    if fail is not None:
        a.icp_fail_threshold = fail
    tr = M.IcpTracker(a)
    f0 = M.preprocess_frame(cuda(torch, x["depth0"]), K, MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    tr.update_curr_status(f0["depth_map"], K)
    pose0, ok0 = tr.predict_pose({"K": K, "frame_id": 0})
    assert np.array_equal(pose0, np.eye(4, dtype=np.float32)) and ok0 is True
    tr.move_last_status()
    tr.update_last_status(None, cuda(torch, x["render_depth"]), f0["depth_map"], cuda(torch, x["render_normal"]), f0["normal_map_c"])
    f1 = M.preprocess_frame(cuda(torch, x["depth1"]), K, MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    tr.update_curr_status(f1["depth_map"], K)
    pose, ok = tr.predict_pose({"K": K, "frame_id": 1})
    _, _, loss, ratio = tr.predict_pose_async({"K": K, "frame_id": 1})
    return tr, pose, ok, float(loss), float(ratio)


def test_predict_pose_vs_goldens_and_oracle(trk):
    torch, M = trk
    for c in CASES:
        for m in (0, 1):
            tr, pose, ok, loss, ratio = run_pair(torch, M, c, bool(m))
            assert pose.dtype == np.float32 and pose.shape == (4, 4) and isinstance(ok, bool)
            np.testing.assert_allclose(pose, G[f"{c}_m{m}_pose"], rtol=0, atol=2e-4)
            assert ok == bool(G[f"{c}_m{m}_success"])
            assert abs(loss - G[f"{c}_m{m}_loss"]) <= 1e-3 * G[f"{c}_m{m}_loss"]
            assert abs(ratio - G[f"{c}_m{m}_valid_ratio"]) < 5e-3
            x, _, _, p0, p1 = frame_pair(c, bool(m))
            opose, ook, oloss, oratio = to.predict_pose(p0, p1, x["K"], fail_threshold=FAIL_THRESH[c])
            np.testing.assert_allclose(pose, opose, rtol=0, atol=1e-4)
            assert ok == ook and abs(loss - oloss) <= 1e-4 * oloss
    # the failure test is `loss > threshold` on the device
    _, _, ok, loss, _ = run_pair(torch, M, "c0", False, fail=1e9)
    assert ok is True
    _, _, ok, loss, _ = run_pair(torch, M, "c1", False, fail=0.0)
    assert ok is False


def test_bitwise_reproducible(trk):
    torch, M = trk
    a = run_pair(torch, M, "c1", True)
    b = run_pair(torch, M, "c1", True)
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_predict_pose_async_graph_replay_is_bitwise(trk):
    torch, M = trk
    tr, pose, ok, loss, ratio = run_pair(torch, M, "c1", True)
    K = torch.tensor(inputs("c1")["K"])
    frame = {"K": K, "frame_id": 1}
    eager = [t.clone() for t in tr.predict_pose_async(frame)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.predict_pose_async(frame)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = tr.predict_pose_async(frame)
    for t in outs:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, outs):
        assert torch.equal(e, r)
    assert np.array_equal(np_(outs[0]), pose)


def test_rendered_frame_pair(trk):
    """Depth and normal rendered by the mapping harness at two poses a known small motion apart; the tracker must agree with the
    oracle and recover the motion."""
    torch, M = trk
    from dqo_harness import mapping, scenes
    W, H = 640, 480
    cam0 = scenes.replica_camera(W, H, 525.0, 525.0, 319.5, 239.5)
    scene = scenes.surfel_room(2, 300_000)
    R1 = scenes.rot_yx(13.0, 4.5)  # 1 degree of yaw, half a degree of pitch more
    pos1 = np.array([0.3, 0.1, -1.85]) + np.array([0.02, -0.01, 0.03])
    cam1 = scenes.Camera(W, H, 525.0, 525.0, 319.5, 239.5, R1, -R1 @ pos1)
    gp = mapping.GaussianParams(scene, "cuda").activated()
    with torch.no_grad():
        r0 = mapping.render(mapping.make_settings(cam0, "cuda"), gp)
        r1 = mapping.render(mapping.make_settings(cam1, "cuda"), gp)
    K = torch.tensor(cam0.K.astype(np.float32))
    a = args("c0", True)
    tr = M.IcpTracker(a)
    f0 = M.preprocess_frame(r0["depth"][0].contiguous(), K, MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    tr.update_curr_status(f0["depth_map"], K)
    tr.predict_pose({"K": K, "frame_id": 0})
    tr.move_last_status()
    Rw2c0 = torch.tensor(cam0.Rw2c.astype(np.float32), device="cuda")
    rn = (Rw2c0 @ r0["normal"].reshape(3, -1)).T.reshape(H, W, 3).contiguous()  # world -> camera-0 normals
    rd = r0["depth"][0].clone().contiguous()
    tr.update_last_status(None, rd, f0["depth_map"], rn, f0["normal_map_c"])
    f1 = M.preprocess_frame(r1["depth"][0].contiguous(), K, MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    tr.update_curr_status(f1["depth_map"], K)
    pose, ok = tr.predict_pose({"K": K, "frame_id": 1})
    # oracle on the same device inputs
    Kn = cam0.K.astype(np.float32)
    p0 = to.pyramid(np_(rd), Kn)
    p1 = to.pyramid(np_(f1["depth_map"]), Kn)
    opose, _, _, _ = to.predict_pose(p0, p1, Kn, fail_threshold=a.icp_fail_threshold)
    np.testing.assert_allclose(pose, opose, rtol=0, atol=1e-4)
    # truth: camera-1 points into camera 0 = w2c0 @ c2w1
    T_true = cam0.Rt @ np.linalg.inv(cam1.Rt)
    t_err = np.linalg.norm(pose[:3, 3] - T_true[:3, 3]) / np.linalg.norm(T_true[:3, 3])
    ang = lambda R: np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    r_err = ang(pose[:3, :3].astype(np.float64) @ T_true[:3, :3].T) / ang(T_true[:3, :3])
    assert t_err < 0.1 and r_err < 0.1, (t_err, r_err, pose, T_true)


def test_unfiltered_geometry_reproduces_the_reference_cpu_run(trk):
    """Without the bilateral filter, frame geometry and pyramids are the reference's (its CPU run, the goldens) to the last bit."""
    torch, M = trk
    for c in CASES:
        x = inputs(c)
        out = M.preprocess_frame(cuda(torch, x["depth0"]), torch.tensor(x["K"]), MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
        for k, g in (("depth_map", "pre0_depth"), ("normal_map_c", "pre0_normal"), ("confidence_map", "pre0_conf"),
                     ("invalid_confidence_mask", "pre0_invalid"), ("vertex_map_c", "pyr_vertex2")):
            assert np.array_equal(np_(out[k]).reshape(G[f"{c}_{g}"].shape), G[f"{c}_{g}"]), (c, k)
        _, pyr = pyramid_on_gpu(torch, M, G[f"{c}_pre0_depth"], G[f"{c}_K"])
        for L, (V, Nm) in enumerate(pyr):
            gv = G[f"{c}_pyr_vertex{L}"]
            assert np.array_equal(V if gv.ndim == 3 else V[..., 2], gv) and np.array_equal(Nm, G[f"{c}_pyr_normal{L}"]), (c, L)


def test_fresh_gpu_intrinsics_every_frame_no_host_sync(trk):
    """DQO-MAP hands the tracker a NEW GPU intrinsic tensor every frame (frame.get_intrinsic).  The per-frame chain must then issue
    no host synchronisation, give what a host K gives, and capture / replay with such a K."""
    torch, M = trk
    c = "c1"
    x = inputs(c)
    fresh = [torch.tensor(x["K"], device="cuda") for _ in range(9)]  # a new device tensor for every use (made ahead: the upload
    gK = fresh.pop                                                     # from the host is the caller's, and it synchronises)
    ref = run_pair(torch, M, c, True)  # host K
    tr = M.IcpTracker(args(c, True))
    f0 = M.preprocess_frame(cuda(torch, x["depth0"]), gK(), MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    tr.update_curr_status(f0["depth_map"], gK())
    tr.predict_pose({"K": gK(), "frame_id": 0})
    tr.move_last_status()
    rd, fn, d1 = cuda(torch, x["render_depth"]), cuda(torch, x["render_normal"]), cuda(torch, x["depth1"])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call raises
    try:
        tr.update_last_status(None, rd, f0["depth_map"], fn, f0["normal_map_c"])
        f1 = M.preprocess_frame(d1, gK(), MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
        tr.update_curr_status(f1["depth_map"], gK())
        outs = tr.predict_pose_async({"K": gK(), "frame_id": 1})
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(np_(outs[0]), ref[1]) and bool(outs[1]) == ref[2] and float(outs[2]) == ref[3] and float(outs[3]) == ref[4]
    eager = [t.clone() for t in outs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.predict_pose_async({"K": gK(), "frame_id": 1})
    torch.cuda.current_stream().wait_stream(s)
    Kcap = gK()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = tr.predict_pose_async({"K": Kcap, "frame_id": 1})
    for t in outs:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, outs):
        assert torch.equal(e, r)
