"""GPU: the trajectory kernels (csrc/map_traj.hip; dqo_icp.Trajectory, dqo_icp.world_maps, dqo_eval.eval_ate) against values recorded from
the reference's own functions (tests/golden/traj_golden.npz), against the numpy restatement (tests/traj_oracle.py), run to run, in place,
past a full store, under graph replay, and as the tracker -> trajectory -> mapper chain inside a graph capture (no host synchronisation).

Bars: the ATE curve within 1e-10 cm of the reference (coordinates below 10 m: a double rounding is ~1e-13 cm per coordinate; the reference
and a float64 restatement differ by 2e-13 cm at most on these trajectories); poses and world maps bit for bit the oracle's; the camera
tensors within one float32 ulp of the float64 truth, and within the reference's own recorded distance from that truth plus that ulp of
the reference's tensors; theta within 1e-9 degrees (acos amplifies a 1e-15 error of the cosine by less than 120 at 0.5 degrees), l2
within 1e-12."""
import os

import numpy as np
import pytest

import traj_oracle as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "traj_golden.npz"))
NAMES = [str(n) for n in G["ate_names"]]
CHAINS = 3
ATE_BAR_CM = 1e-10
DEGENERATE_FIT = ("line", "plane", "still")  # the optimal rotation is not unique: only the error is compared
KF, TESTED = TO.TESTED | TO.KEYFRAME | TO.LISTED, TO.TESTED


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()
    import dqo_eval
    import dqo_icp
    return torch, dqo_icp, dqo_eval


def cuda(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def np_(t):
    return t.detach().cpu().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- ATE ----------------------------------------------------------------------------------------------------------------------------

def test_ate_curves_vs_reference(env):
    torch, _, E = env
    worst = 0.0
    for name in NAMES:
        gt, es, ref = G[f"ate_{name}_gt"], G[f"ate_{name}_es"], G[f"ate_{name}_curve"]
        fit = torch.full((12,), float("nan"), dtype=torch.float64, device="cuda")
        a = E.eval_ate(cuda(torch, es), cuda(torch, gt), fit=fit)
        curve = np_(a)
        assert curve.shape == (257,) and curve.dtype == np.float64 and np.isfinite(curve).all(), name
        worst = max(worst, np.abs(curve - ref).max())
        assert np.abs(curve - ref).max() <= ATE_BAR_CM, (name, np.abs(curve - ref).max(), int(np.abs(curve - ref).argmax()) + 1)
        # the same bytes on every run, and from the translation column of [N,4,4] pose stacks read in place
        b = E.eval_ate(cuda(torch, es), cuda(torch, gt))
        assert torch.equal(a, b), name
        stack = lambda p: cuda(torch, np.concatenate([np.tile(np.eye(4)[None, :, :3], (len(p), 1, 1)), np.concatenate([p, np.ones((len(p), 1))], 1)[:, :, None]], 2))
        c = E.eval_ate(stack(es), stack(gt))
        assert torch.equal(a, c), name
        if not name.startswith(DEGENERATE_FIT):
            f = np_(fit)
            assert np.abs(f[:9].reshape(3, 3) - G[f"ate_{name}_rot"]).max() <= 1e-12 and np.abs(f[9:] - G[f"ate_{name}_trans"]).max() <= 1e-12, name
        if name == "same":
            assert (curve < ATE_BAR_CM).all()
            assert E.eval_ate_dict(a) == {"ate": curve[-1]}
    print("dqo_eval_ate vs the reference's eval_ate, worst |difference|:", worst, "cm")


def test_ate_with_more_prefixes_than_blocks(env):
    """N past the grid's cap (16384 blocks): a block then walks several prefixes.  Held to the restatement on prefixes of both rounds."""
    torch, _, E = env
    N = 16384 + 300
    rng = np.random.default_rng(5)
    s = np.linspace(0.0, 1.0, N)
    gt = np.stack([3.0 * np.cos(9 * s), 2.0 * np.sin(7 * s), 1.0 + 0.3 * np.sin(31 * s)], 1)
    es = gt + 0.02 * rng.normal(size=gt.shape)
    curve = np_(E.eval_ate(cuda(torch, es), cuda(torch, gt)))
    assert np.isfinite(curve).all()
    for i in (1, 299, 300, 301, 16384, 16385, 16600, N):
        assert abs(curve[i - 1] - TO.ate_prefix(gt[:i], es[:i])[0]) <= ATE_BAR_CM, i


# ---- append: poses, cameras, keyframes ----------------------------------------------------------------------------------------------

def run_chain(torch, M, c, guf=1, theta=None, trans=None, cap=12):
    kw = {}
    if theta is not None:
        kw = dict(keyframe_theta_thes=theta, keyframe_trans_thes=trans)
    tr = M.Trajectory(cap, "cuda", projection=cuda(torch, G["projection"]), gaussian_update_frame=guf,
                      init_pose=cuda(torch, G[f"chain{c}_init"]) if c == 2 else None, **kw)
    rel = cuda(torch, G[f"chain{c}_rel"])
    cams = []
    for i in range(12):
        tr.append(rel[i])
        cams.append({k: getattr(tr, k).clone() for k in ("c2w", "viewmatrix", "projmatrix", "campos")})
    return tr, [{k: np_(v) for k, v in cam.items()} for cam in cams]


def oracle_chain(c, guf=1, theta=0.0, trans=0.0):
    o = TO.Trajectory(12, projection=G["projection"], gaussian_update_frame=guf, theta_thres=theta, trans_thres=trans,
                      init_pose=G[f"chain{c}_init"] if c == 2 else None)
    cams = []
    for i in range(12):
        o.append(G[f"chain{c}_rel"][i])
        cams.append(o.cam)
    return o, cams


def test_append_poses_and_cameras(env):
    torch, M, _ = env
    for c in range(CHAINS):
        tr, cams = run_chain(torch, M, c)
        o, ocams = oracle_chain(c)
        pose = np_(tr.poses())
        assert len(tr) == 12 and pose.shape == (12, 4, 4) and pose.dtype == np.float64 and not tr.overflowed()
        assert np.array_equal(pose, o.pose)  # bit for bit the oracle's
        rel = G[f"chain{c}_rel"].astype(np.float64)
        for i in range(1, 12):  # numpy's product: the dot-product rounding bound for two 4-term sums
            assert np.all(np.abs(pose[i] - pose[i - 1] @ rel[i]) <= 8 * 2.0 ** -53 * (np.abs(pose[i - 1]) @ np.abs(rel[i]))), (c, i)
        for i in range(12):
            cam, v64, f64 = cams[i], G[f"chain{c}_view64"][i], G[f"chain{c}_full64"][i]
            for k in ("c2w", "viewmatrix", "projmatrix", "campos"):
                assert np.array_equal(cam[k].reshape(-1), np.asarray(ocams[i][k]).reshape(-1)), (c, i, k)
            assert np.all(np.abs(cam["c2w"] - pose[i]) <= ulp32(pose[i]))
            assert np.all(np.abs(cam["viewmatrix"] - v64) <= ulp32(v64)), (c, i)
            assert np.all(np.abs(cam["viewmatrix"] - G[f"chain{c}_view"][i]) <= G[f"chain{c}_view_dist"] + ulp32(v64)), (c, i)
            assert np.all(np.abs(cam["projmatrix"] - f64) <= ulp32(f64)), (c, i)
            assert np.all(np.abs(cam["projmatrix"] - G[f"chain{c}_full"][i]) <= G[f"chain{c}_full_dist"] + ulp32(f64)), (c, i)
            assert np.array_equal(cam["campos"], pose[i][:3, 3].astype(np.float32))


def test_keyframe_decisions_and_metrics(env):
    torch, M, _ = env
    for c in range(CHAINS):
        # against row 0 (thresholds no row reaches): the metrics rot_compare / trans_compare gave
        tr, _ = run_chain(torch, M, c, theta=1e9, trans=1e9)
        flags, metric = np_(tr.flags), np_(tr.kf_metric)
        assert flags[0] == TO.TESTED | TO.LISTED and (flags[1:] == TESTED).all()  # row 0 is listed but not reported
        assert np.abs(metric[1:, 0] - G[f"chain{c}_theta"][1:]).max() <= 1e-9 and np.abs(metric[1:, 1] - G[f"chain{c}_l2"][1:]).max() <= 1e-12
        # check_keyframe's sequence with the fixture's thresholds: the keyframe row moves on
        th, tt = float(G[f"chain{c}_theta_thres"]), float(G[f"chain{c}_l2_thres"])
        tr, _ = run_chain(torch, M, c, theta=th, trans=tt)
        flags, metric, kf = np_(tr.flags), np_(tr.kf_metric), G[f"chain{c}_seq_kf"]
        assert flags[0] == TO.TESTED | TO.LISTED and np.array_equal(flags[1:], np.where(kf[1:], KF, TESTED)), (c, flags)
        assert np.abs(metric[1:, 0] - G[f"chain{c}_seq_theta"][1:]).max() <= 1e-9
        assert np.abs(metric[1:, 1] - G[f"chain{c}_seq_l2"][1:]).max() <= 1e-12
        assert int(np_(tr.header)[1]) == int(np.nonzero(kf)[0][-1])
        assert tr.is_keyframe() == bool(kf[-1]) and int(np_(tr.keyframe())[0]) == flags[-1]
    tr, _ = run_chain(torch, M, 0, guf=4, theta=1e9, trans=1e9)
    assert [i for i, f in enumerate(np_(tr.flags)) if f & TO.TESTED] == [0, 3, 7, 11]
    tr, _ = run_chain(torch, M, 0, guf=0)
    assert not np_(tr.flags).any()


def test_identical_poses_absolute_mode_and_ground_truth(env):
    """Two appends of one world pose: the decision only — NaN, 0 and the few hundredths of a degree a float32-orthonormal rotation leaves
    all say "no keyframe".  Absolute mode stores the pose as given; the ground-truth pose is stored beside it."""
    torch, M, _ = env
    th = min(float(G[f"chain{c}_theta_thres"]) for c in range(CHAINS))
    tt = min(float(G[f"chain{c}_l2_thres"]) for c in range(CHAINS))
    tr = M.Trajectory(4, "cuda", gaussian_update_frame=1, keyframe_theta_thes=th, keyframe_trans_thes=tt)
    P, gt = cuda(torch, G["same_pose"]), cuda(torch, G["chain0_pose"][3])
    tr.append(P, relative=False, pose_gt=gt), tr.append(P, relative=False, pose_gt=gt)
    assert np_(tr.flags)[:2].tolist() == [TO.TESTED | TO.LISTED, TO.TESTED] and not tr.is_keyframe()
    assert not G["same_theta"] > th and not G["same_l2"] > tt  # the reference's decision
    assert np.array_equal(np_(tr.poses()), np.stack([G["same_pose"]] * 2)) and np.array_equal(np_(tr.poses_gt()), np.stack([G["chain0_pose"][3]] * 2))
    assert np.array_equal(np_(tr.c2w), G["same_pose"].astype(np.float32))


def test_full_store_writes_nothing(env):
    """13 appends into a store of capacity 12 (through the C entry, on buffers two rows longer than the capacity it is told): 12 rows, the
    overflow word set, nothing written past the end."""
    torch, M, _ = env
    import _dqo_native as N
    cap = 12
    pose = torch.full((cap + 2, 16), -7.0, dtype=torch.float64, device="cuda")
    metric = torch.full((cap + 2, 2), -7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((cap + 2,), -7, dtype=torch.int32, device="cuda")
    header = torch.tensor([0, -1, 0, 0], dtype=torch.int32, device="cuda")
    cam = torch.zeros((16,), dtype=torch.float32, device="cuda")
    rel = cuda(torch, G["chain0_rel"])
    for i in range(13):
        if i == 12:
            before = cam.clone()
        N.check(N.lib().dqo_traj_append(cap, pose.data_ptr(), None, flags.data_ptr(), metric.data_ptr(), header.data_ptr(), rel[i % 12].data_ptr(),
                                        None, None, None, None, cam.data_ptr(), None, None, None, 1, 1e9, 1e9, N.current_stream()))
    assert np_(header).tolist() == [12, 0, 1, 0]
    assert (np_(pose)[cap:] == -7.0).all() and (np_(metric)[cap:] == -7.0).all() and (np_(flags)[cap:] == -7).all()
    assert np.array_equal(np_(pose)[:cap].reshape(cap, 4, 4), oracle_chain(0)[0].pose) and torch.equal(cam, before)
    tr, _ = run_chain(torch, M, 0)
    tr.append(rel[0])
    assert len(tr) == 12 and tr.overflowed() and np.array_equal(np_(tr.poses()), oracle_chain(0)[0].pose)


def test_appends_replayed_from_one_graph_fill_consecutive_rows(env):
    torch, M, _ = env
    rel = cuda(torch, G["chain1_rel"])
    M.Trajectory(2, "cuda", projection=cuda(torch, G["projection"])).append(rel[0])  # the kernel is loaded before the capture
    tr = M.Trajectory(12, "cuda", projection=cuda(torch, G["projection"]), gaussian_update_frame=1,
                      keyframe_theta_thes=float(G["chain1_theta_thres"]), keyframe_trans_thes=float(G["chain1_l2_thres"]))
    static = rel[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.append(static)  # (counts the first replay in the host's mirror)
    for i in range(12):
        static.copy_(rel[i])
        g.replay()
    tr.advance(11)
    torch.cuda.synchronize()
    o, ocams = oracle_chain(1, theta=float(G["chain1_theta_thres"]), trans=float(G["chain1_l2_thres"]))
    assert len(tr) == 12 and np_(tr.header).tolist() == [12, o.last_keyframe, 0, 0]
    assert np.array_equal(np_(tr.poses()), o.pose) and np.array_equal(np_(tr.flags), o.flags)
    assert np.array_equal(np_(tr.viewmatrix), ocams[-1]["viewmatrix"]) and np.array_equal(np_(tr.projmatrix), ocams[-1]["projmatrix"])


# ---- world maps ---------------------------------------------------------------------------------------------------------------------

def test_world_maps(env):
    torch, M, _ = env
    for mi in range(2):
        v, n, c2w = G[f"map{mi}_vertex_c"], G[f"map{mi}_normal_c"], G[f"map{mi}_c2w"]
        ov, on = TO.world_maps(v, n, c2w)
        vc, nc, cw = cuda(torch, v), cuda(torch, n), cuda(torch, c2w)
        vw, nw = M.world_maps(vc, nc, cw)
        assert np.array_equal(np_(vw), ov) and np.array_equal(np_(nw), on)  # bit for bit the float32 oracle
        A = np.abs(c2w.astype(np.float64))
        for got, ref, src, t in ((ov, G[f"map{mi}_vertex_w"], v, 1.0), (on, G[f"map{mi}_normal_w"], n, 0.0)):
            mag = np.abs(src.astype(np.float64)) @ A[:3, :3].T + t * A[:3, 3]
            assert np.all(np.abs(got.astype(np.float64) - ref) <= 8 * 2.0 ** -24 * mag)
        hole = (v == 0).all(-1)
        assert hole.any() and np.array_equal(np_(vw)[hole], np.broadcast_to(c2w[:3, 3], (int(hole.sum()), 3)))  # a zero vertex maps to t
        # in place, the vertex map alone, and maps that are not 16-byte aligned (the 4-byte path): the same bytes
        a, b = vc.clone(), nc.clone()
        M.world_maps(a, b, cw, out=(a, b))
        assert torch.equal(a, vw) and torch.equal(b, nw)
        only, none = M.world_maps(vc, None, cw)
        assert none is None and torch.equal(only, vw)
        H, W = v.shape[:2]
        off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(H, W, 3)
        a, b = off(vc), off(nc)
        assert a.data_ptr() % 16 == 4
        c, d = M.world_maps(a, b, cw, out=(off(vc), off(nc)))
        assert torch.equal(c, vw) and torch.equal(d, nw)
        a, b = M.world_maps(a, b, cw, out=(a, b))
        assert torch.equal(a, vw) and torch.equal(b, nw)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def test_tracker_to_mapper_chain_inside_a_graph_capture(env):
    """predict_pose_async -> append -> world_maps -> settings -> FusedMapper.set_frame on the 48x64 frame pair of tracking_golden.npz,
    issued inside a torch.cuda.graph capture — a synchronising call (.cpu(), .item(), .tolist()) there raises — and replayed once: the
    mapper's frame ends with the camera tensors the host computes from the read-back pose, within the camera bars."""
    torch, M, _ = env
    from dqo_harness.fused_mapping import FusedMapper
    from test_gpu_tracking import run_pair
    from test_gpu_window import _window_problem
    from test_tracking_oracle import inputs
    trk, _, _, _, _ = run_pair(torch, M, "c0", True)
    assert trk.vertex_pyramid_t1[-1].shape == (48, 64, 3)
    frame = {"K": torch.tensor(inputs("c0")["K"]), "frame_id": 1}
    vc, nc = trk.vertex_pyramid_t1[-1].clone(), trk.normal_pyramid_t1[-1].clone()  # the current frame's camera-frame maps
    sc, cams, frames, dev = _window_problem(torch, 3000, 1)
    template = frames[0]["settings"]
    fm = FusedMapper(sc, template, dev)
    fm.capture_window([frames[0]], loss_tap=True, fused_tail=True, capacity_margin=2.0)
    proj = cuda(torch, G["projection"])

    def chain(tr, out):
        pose, ok, _, _ = trk.predict_pose_async(frame)
        tr.append(pose)
        tr.world_maps(vc, nc, out=out)
        fm.set_frame(0, settings=tr.settings(template))

    def fresh():
        tr = M.Trajectory(8, dev, projection=proj, gaussian_update_frame=1)
        tr.append(trk.predict_pose_async(frame)[0])  # the first frame: row 0 takes the identity whatever the tracker says
        return tr, (torch.empty_like(vc), torch.empty_like(nc))

    tr, out = fresh()
    chain(tr, out)  # eager once: every kernel is loaded before the capture
    tr, out = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(tr, out)
    g.replay()
    torch.cuda.synchronize()
    pose10 = np_(trk.predict_pose_async(frame)[0])
    world = np.eye(4) @ pose10.astype(np.float64)
    assert len(tr) == 2 and np.array_equal(np_(tr.poses())[1], world)
    v64 = np.linalg.inv(world).T
    f64 = v64 @ G["projection"].astype(np.float64)
    st = fm._frames[0].settings
    assert torch.equal(st.viewmatrix.reshape(-1), tr.viewmatrix.reshape(-1)) and torch.equal(st.projmatrix.reshape(-1), tr.projmatrix.reshape(-1))
    assert torch.equal(st.campos.reshape(-1), tr.campos)
    assert np.all(np.abs(np_(st.viewmatrix).reshape(4, 4) - v64) <= ulp32(v64))
    assert np.all(np.abs(np_(st.projmatrix).reshape(4, 4) - f64) <= ulp32(f64))
    assert np.array_equal(np_(st.campos).reshape(-1), world[:3, 3].astype(np.float32))
    ov, on = TO.world_maps(np_(vc), np_(nc), world.astype(np.float32))
    assert np.array_equal(np_(out[0]), ov) and np.array_equal(np_(out[1]), on)
