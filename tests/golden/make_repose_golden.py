"""Generates tests/golden/repose_golden.npz by importing the REFERENCE modules utils/graphics_utils.py and scene/cameras.py in the
authoring container (CPU, no GPU), as make_traj_golden.py does, and running the reference's own Camera.updatePose
(scene/cameras.py:165-183) — what Mapping.update_poses (SLAM/multiprocess/mapper.py:256-263) and the evaluation drivers (metric.py:181,
make_mesh.py:199, metric_obj.py:212) hand every corrected pose to:

  - 70 seeded ABSOLUTE world poses along a room loop, whose rotations are float32-rounded products of float32-rounded rotations
    (orthonormal only to float32, as the poses an ORB-style back end returns are), translations of a few metres;
  - for each: world_view_transform and full_proj_transform for a Replica projection (getProjectionMatrix), the float64 truth of both
    and the reference's own largest distance from it (view: one number; full: per entry, the columns differ in scale).

Only runs where the reference checkout exists (make_icp_golden.REF); the produced .npz (inputs + expected outputs = data) is committed, the reference source never
is."""
import os
import sys
import types

import numpy as np

from make_icp_golden import import_reference_utils
from make_tracking_golden import cpu_only
from make_traj_golden import import_reference_cameras, rot

N_POSES = 70


def main():
    u = import_reference_utils()
    gu, cams = import_reference_cameras(u)
    rng = np.random.default_rng(20261021)
    W_, H_, fx = 1200, 680, 600.0  # Replica
    fovx, fovy = 2 * np.arctan(W_ / (2 * fx)), 2 * np.arctan(H_ / (2 * fx))
    proj = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
    projection = proj.numpy().copy()
    poses, views, fulls, views64, fulls64 = [], [], [], [], []
    R = rot([0.1, 0.9, 0.3], 25.0).astype(np.float32)
    for i in range(N_POSES):
        R = (R @ rot(rng.normal(size=3), rng.uniform(0.5, 12.0)).astype(np.float32)).astype(np.float32)  # a float32 product: drifts as ORB's do
        s = i / N_POSES
        P = np.eye(4)
        P[:3, :3] = R.astype(np.float64)
        P[:3, 3] = np.array([3.0 * np.cos(2 * np.pi * s), 2.0 * np.sin(2 * np.pi * s), 1.2 + 0.3 * np.sin(6 * np.pi * s)]) + rng.uniform(-0.05, 0.05, size=3)
        cam = types.SimpleNamespace(Rt=np.eye(3, 4), trans=np.array([0.0, 0.0, 0.0]), scale=1.0, projection_matrix=proj)
        cam.update = types.MethodType(cams.Camera.update, cam)
        with cpu_only():
            cams.Camera.updatePose(cam, P)
        poses.append(P)
        views.append(cam.world_view_transform.numpy().copy()), fulls.append(cam.full_proj_transform.numpy().copy())
        v64 = np.linalg.inv(P).T
        views64.append(v64), fulls64.append(v64 @ projection.astype(np.float64))
    out = dict(projection=projection, pose=np.stack(poses), view=np.stack(views), full=np.stack(fulls), view64=np.stack(views64),
               full64=np.stack(fulls64))
    out["view_dist"] = np.abs(out["view"] - out["view64"]).max()
    out["full_dist"] = np.abs(out["full"] - out["full64"]).max(axis=0)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "repose_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; view_dist", out["view_dist"], "full_dist max", out["full_dist"].max())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
