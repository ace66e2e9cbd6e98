"""Generates tests/golden/traj_golden.npz by importing the REFERENCE modules SLAM/utils.py, utils/graphics_utils.py and scene/cameras.py in
the authoring container (CPU, no GPU) and running the reference's own functions:

  - eval_ate (SLAM/utils.py:486-532) over every prefix of 16 trajectories of 257 points — a room loop, a line, a plane and a camera that
    stands still, each with noise 0 / 1e-3 / 0.02 / 0.3 m on a rigidly moved estimate — in Tracker.eval_ate's argument order
    (tracker.py:429: eval_ate(pose_gt, pose_es)), plus one case with es == gt; and align (utils.py:449-483) of the full trajectories;
  - chains of 12 relative float32 poses (rotations of 0.5-5 degrees): numpy's float64 products (tracker.py:324), Camera.updatePose's
    world_view_transform / full_proj_transform (scene/cameras.py:165-183) for a Replica projection (getProjectionMatrix), the float64
    truth of both and the reference's own largest distance from it;
  - rot_compare / trans_compare (utils.py:42-54) of every chain row against a keyframe row as check_keyframe calls them
    (mapper.py:749-754), check_keyframe's sequence of decisions (:757-773: the keyframe row moves on) with thresholds at least 1e-6
    away from every value, and one pair of identical poses;
  - transform_map (utils.py:56-63) on 36x60 and 17x23 maps with holes.

Only runs where /root/reference exists; the produced .npz (inputs + expected outputs = data) is committed, the reference source never
is.  SLAM/utils.py is loaded as in make_icp_golden.py; `.cuda()` returns the tensor itself inside make_tracking_golden.py's cpu_only().
It also prints the reference's CPU time for the ATE curve of a 2000-frame trajectory (Tracker.eval_total_ate's loop)."""
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch

from make_icp_golden import REF, import_reference_utils
from make_tracking_golden import cpu_only

N_ATE, CHAINS, CHAIN_LEN = 257, 3, 12


def import_reference_cameras(u):
    pkg = types.ModuleType("SLAM")
    pkg.__path__ = [os.path.join(REF, "SLAM")]
    sys.modules["SLAM"], sys.modules["SLAM.utils"] = pkg, u
    sys.modules["SLAM.multiprocess"] = types.ModuleType("SLAM.multiprocess")
    q = types.ModuleType("SLAM.multiprocess.quadrics")
    q.get_2dim_quarics = None
    sys.modules["SLAM.multiprocess.quadrics"] = q
    mods = {}
    for name, rel in (("utils.graphics_utils", "utils/graphics_utils.py"), ("scene.cameras", "scene/cameras.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["utils.graphics_utils"], mods["scene.cameras"]


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def trajectories(rng):
    s = np.linspace(0.0, 1.0, N_ATE)
    shapes = dict(
        room=np.stack([3.0 * np.cos(2 * np.pi * s), 2.0 * np.sin(2 * np.pi * s), 1.2 + 0.3 * np.sin(6 * np.pi * s)], 1),
        line=np.stack([4.0 * s - 2.0, 0.5 * (4.0 * s - 2.0) + 1.0, -0.25 * (4.0 * s - 2.0)], 1),
        plane=np.stack([3.0 * np.cos(2 * np.pi * s), 2.0 * np.sin(4 * np.pi * s), np.full_like(s, 0.7)], 1),
        still=np.tile(np.array([[1.5, -0.4, 0.9]]), (N_ATE, 1)))
    R0, t0 = rot([0.2, -0.5, 0.8], 17.0), np.array([0.3, -0.2, 0.1])
    for name, gt in shapes.items():
        for noise in (0.0, 1e-3, 0.02, 0.3):
            es = gt @ R0.T + t0 + noise * rng.normal(size=gt.shape)
            yield f"{name}_{noise:g}", gt, es
    gt = shapes["room"] + 0.01 * rng.normal(size=(N_ATE, 3))
    yield "same", gt, gt.copy()


def main():
    u = import_reference_utils()
    gu, cams = import_reference_cameras(u)
    rng = np.random.default_rng(20251019)
    out = {}

    # ---- ATE curves ----
    names = []
    for name, gt, es in trajectories(rng):
        names.append(name)
        out[f"ate_{name}_gt"], out[f"ate_{name}_es"] = gt, es
        out[f"ate_{name}_curve"] = np.array([u.eval_ate(gt[:i], es[:i]) for i in range(1, N_ATE + 1)])  # (pose_estimate=gt: tracker.py:429)
        r, t, _ = u.align(np.matrix(gt.T), np.matrix(es.T))
        out[f"ate_{name}_rot"], out[f"ate_{name}_trans"] = np.asarray(r), np.asarray(t).reshape(3)
    out["ate_names"] = np.array(names)

    # ---- pose chains, cameras, keyframe metrics ----
    W_, H_, fx = 1200, 680, 600.0  # Replica
    fovx, fovy = 2 * np.arctan(W_ / (2 * fx)), 2 * np.arctan(H_ / (2 * fx))
    proj = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
    out["projection"] = proj.numpy().copy()
    truth = lambda P: (np.linalg.inv(P).T, np.linalg.inv(P).T @ out["projection"].astype(np.float64))
    for c in range(CHAINS):
        rel = np.tile(np.eye(4, dtype=np.float32), (CHAIN_LEN, 1, 1))
        for i in range(CHAIN_LEN):
            rel[i, :3, :3] = rot(rng.normal(size=3), rng.uniform(0.5, 5.0)).astype(np.float32)  # orthonormal to float32 only
            rel[i, :3, 3] = rng.uniform(-0.08, 0.08, size=3).astype(np.float32)
        init = np.eye(4)
        if c == 2:  # a chain that starts from a given pose
            init[:3, :3], init[:3, 3] = rot([0.3, 0.9, -0.1], 40.0), [1.0, -2.0, 0.5]
        poses, views, fulls, views64, fulls64 = [], [], [], [], []
        for i in range(CHAIN_LEN):
            poses.append(init.copy() if i == 0 else poses[-1] @ rel[i])  # tracker.py:318, :324 (rel[0] is the first frame's unused answer)
            cam = types.SimpleNamespace(Rt=np.eye(3, 4), trans=np.array([0.0, 0.0, 0.0]), scale=1.0, projection_matrix=proj)
            cam.update = types.MethodType(cams.Camera.update, cam)
            with cpu_only():
                cams.Camera.updatePose(cam, poses[-1])
            views.append(cam.world_view_transform.numpy().copy()), fulls.append(cam.full_proj_transform.numpy().copy())
            v64, f64 = truth(poses[-1])
            views64.append(v64), fulls64.append(f64)
            if i == 0:
                key_R, key_T = cam.R.T.copy(), cam.T.copy()  # keyframe_list[-1].R.T, .T (mapper.py:749-750)
                out[f"chain{c}_theta"], out[f"chain{c}_l2"] = [0.0], [0.0]
            else:
                out[f"chain{c}_theta"].append(u.rot_compare(key_R, cam.R.T)[1]), out[f"chain{c}_l2"].append(u.trans_compare(key_T, cam.T)[1])
        out[f"chain{c}_rel"], out[f"chain{c}_init"], out[f"chain{c}_pose"] = rel, init, np.stack(poses)
        out[f"chain{c}_view"], out[f"chain{c}_full"] = np.stack(views), np.stack(fulls)
        out[f"chain{c}_view64"], out[f"chain{c}_full64"] = np.stack(views64), np.stack(fulls64)
        out[f"chain{c}_view_dist"] = np.abs(out[f"chain{c}_view"] - out[f"chain{c}_view64"]).max()
        out[f"chain{c}_full_dist"] = np.abs(out[f"chain{c}_full"] - out[f"chain{c}_full64"]).max(axis=0)  # per entry: the columns differ in scale
        th, l2 = np.array(out[f"chain{c}_theta"]), np.array(out[f"chain{c}_l2"])
        out[f"chain{c}_theta"], out[f"chain{c}_l2"] = th, l2
        # check_keyframe's sequence (mapper.py:749-773) with base.yaml-like thresholds: the keyframe row moves on with every keyframe
        thr_theta, thr_l2 = 4.0, 0.12
        kR, kT = np.linalg.inv(poses[0])[:3, :3], np.linalg.inv(poses[0])[:3, 3]
        seq_theta, seq_l2, seq_kf = [0.0], [0.0], [False]
        for i in range(1, CHAIN_LEN):
            w = np.linalg.inv(poses[i])  # updatePose: frame.R.T, frame.T
            th_i, l2_i = u.rot_compare(kR, w[:3, :3])[1], u.trans_compare(kT, w[:3, 3])[1]
            is_kf = bool(th_i > thr_theta or l2_i > thr_l2)
            if is_kf:
                kR, kT = w[:3, :3], w[:3, 3]
            seq_theta.append(th_i), seq_l2.append(l2_i), seq_kf.append(is_kf)
        out[f"chain{c}_seq_theta"], out[f"chain{c}_seq_l2"], out[f"chain{c}_seq_kf"] = np.array(seq_theta), np.array(seq_l2), np.array(seq_kf)
        out[f"chain{c}_theta_thres"], out[f"chain{c}_l2_thres"] = thr_theta, thr_l2
        assert np.abs(np.array(seq_theta[1:]) - thr_theta).min() > 1e-6 and np.abs(np.array(seq_l2[1:]) - thr_l2).min() > 1e-6
        assert any(seq_kf) and not all(seq_kf[1:])
    # identical poses: acos of a cosine that may exceed 1 by a rounding -> NaN or 0, either way "no keyframe"
    P = out["chain1_pose"][5]
    W = np.linalg.inv(P)
    out["same_pose"] = P
    with np.errstate(invalid="ignore"):
        out["same_theta"], out["same_l2"] = u.rot_compare(W[:3, :3], W[:3, :3])[1], u.trans_compare(W[:3, 3], W[:3, 3])[1]

    # ---- world maps ----
    for mi, (H, Wd) in enumerate(((36, 60), (17, 23))):
        z = (2.0 + rng.uniform(-0.5, 0.5, size=(H, Wd))).astype(np.float32)
        jj, ii = np.meshgrid(np.arange(Wd, dtype=np.float32), np.arange(H, dtype=np.float32))
        v = np.stack([(jj - Wd / 2) / (0.8 * Wd) * z, (ii - H / 2) / (0.8 * Wd) * z, z], -1).astype(np.float32)
        n = rng.normal(size=(H, Wd, 3))
        n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        hole = rng.uniform(size=(H, Wd)) < 0.1
        v[hole], n[hole] = 0.0, 0.0
        c2w = out["chain2_pose"][4 + mi].astype(np.float32)
        t = torch.from_numpy
        out[f"map{mi}_vertex_c"], out[f"map{mi}_normal_c"], out[f"map{mi}_c2w"] = v, n, c2w
        out[f"map{mi}_vertex_w"] = u.transform_map(t(v), t(c2w)).numpy()
        out[f"map{mi}_normal_w"] = u.transform_map(t(n), u.get_rot(t(c2w))).numpy()

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traj_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")

    # ---- the reference's CPU time for a 2000-frame curve (Tracker.eval_total_ate) ----
    s = np.linspace(0.0, 1.0, 2000)
    gt = np.stack([3.0 * np.cos(2 * np.pi * s), 2.0 * np.sin(2 * np.pi * s), 1.2 + 0.3 * np.sin(6 * np.pi * s)], 1)
    es = gt + 0.02 * rng.normal(size=gt.shape)
    t0 = time.perf_counter()
    for i in range(1, 2001):
        u.eval_ate(gt[:i], es[:i])
    print(f"reference eval_total_ate, N = 2000: {time.perf_counter() - t0:.2f} s on this CPU")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
