"""dqo_traj_repose (include/dqo_raster.h, csrc/map_repose.hip) restated in numpy, statement by statement: the store's rows below
min(count, n_new, cap) take new_pose's bytes, every target whose row lies in [0, count) gets the camera of its source pose —
new_pose[row] below n_new, the stored pose otherwise — by tests/traj_oracle.py's statements (dqo_traj_camera.h's: the camera bits of
dqo_traj_append), and the counts.  tests/test_repose_oracle.py holds it to values recorded from the reference's Camera.updatePose
(tests/golden/repose_golden.npz); tests/test_gpu_repose.py holds the kernel to it."""
import numpy as np

from traj_oracle import camera, invert_affine

f32, f64 = np.float32, np.float64
FIELDS = ("c2w", "w2c", "viewmatrix", "projmatrix", "campos")


def cameras(P, projection=None):
    """traj_oracle.camera plus w2c [4,4] f32, row-major: [W T; 0 0 0 1] of the double inverse, rounded once (viewmatrix transposed)."""
    cam = camera(P, projection)
    W, T = invert_affine(P)
    M = np.zeros((4, 4), f64)
    M[:3, :3], M[:3, 3], M[3, 3] = W, T, 1.0
    cam["w2c"] = M.astype(f32)
    return cam


def repose(pose, count, new_pose, targets, projection=None):
    """One launch.  pose: float64 [cap,4,4], rewritten in place; count: the header's row count; new_pose: float64 [n_new,4,4] or None;
    targets: a list of (row, wanted) with wanted a subset of FIELDS.  Returns (outs, stats): outs[t] = dict of the tensors target t
    gets (None: a target skipped for its row), stats = [pose rows rewritten, targets written, targets skipped, 0]."""
    cap = pose.shape[0]
    count = min(max(int(count), 0), cap)
    n_new = 0 if new_pose is None else new_pose.shape[0]
    rows = min(count, n_new)
    old = pose.copy()
    pose[:rows] = new_pose[:rows] if rows else pose[:0]
    outs, skipped = [], 0
    for row, wanted in targets:
        if row < 0 or row >= count:
            outs.append(None)
            skipped += 1
            continue
        src = new_pose[row] if row < n_new else old[row]
        cam = cameras(src, projection)
        outs.append({k: cam[k] for k in wanted if cam[k] is not None})
    return outs, [rows, len(targets) - skipped, skipped, 0]
