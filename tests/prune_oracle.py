"""CPU oracle of floater pruning (FusedMapper.prune_floaters / dqo_mapgrowth.prune_cameras, prune_step — csrc/map_prune.hip): a literal
restatement of Mapping.to_purne with create_virtual_cameras (SLAM/multiprocess/mapper.py:424-529).

    virtual_cameras   :471-481, 424-466 and frame.update (scene/cameras.py:169-183): float64 numpy scalars, one rounding per written
                      statement, in the order csrc/map_prune.hip lists them; cos / sin are the caller's (the host's) doubles
    centre_pixel      the pixel whose depth the focal point is taken at: the reference's transposed one, or the principal point
    prune_oracle      :509-527 on two clouds with the reference's delete semantics and a hidden row id

No GPU, no project code."""
import math

import numpy as np
import torch

FREED = dict(opacity_raw=-10.0, scaling_raw=-10.0, alive=0, row_flags=3, confidence=0.0, stable=0, add_tick=0, depth_error_counter=0,
             color_error_counter=0, frame_id=0)  # (+ xyz = park): what a deleted row holds
FATES = ("spare", "outside_window", "kept_touched", "deleted_unstable", "deleted_stable", "kept_skipped")


def host_cos_sin(theta_deg):
    t = math.radians(float(theta_deg))
    return math.cos(t), math.sin(t)


def centre_pixel(cx, cy, H, W, centre="reference"):
    """(row, column) the centre depth is read at.  reference: `cx, cy = int(frame.cy), int(frame.cx)` then `depth_map[cy, cx]`
    (mapper.py:471, 473) — row int(frame.cx), column int(frame.cy); IndexError outside the image, as numpy raises.  principal: row
    int(cy), column int(cx)."""
    row, col = (int(cx), int(cy)) if centre == "reference" else (int(cy), int(cx))
    if not (0 <= row < H and 0 <= col < W):
        raise IndexError((row, col))
    return row, col


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def rotation_matrix(axis, c, s):  # mapper.py:431-443
    one, zero = np.float64(1.0), np.float64(0.0)
    if axis == "x":
        return [[one, zero, zero], [zero, c, -s], [zero, s, c]]
    return [[c, zero, s], [zero, one, zero], [-s, zero, c]]


def virtual_cameras(viewmatrix, projection, depth_map, pixel, cos_t, sin_t):
    """viewmatrix, projection: [4,4] (the transposed w2c / the transposed projection), float32 as the kernel takes them — every entry is
    widened exactly; a float64 pose is taken as it is, which is how tests/test_prune_oracle.py checks the geometry beyond float32's
    orthonormality; depth_map: float32, any shape; pixel: flat index.  Returns dict(viewmatrix [4,4,4] f32, projmatrix [4,4,4] f32, focal [3] f32, and the float64 R [4,3,3], T [4,3], Rw, T0,
    focal64, offset, d)."""
    f64 = np.float64
    vm = np.asarray(viewmatrix).reshape(4, 4)
    Q = [[f64(v) for v in row] for row in np.asarray(projection).reshape(4, 4)]
    Rw = [[f64(vm[b, a]) for b in range(3)] for a in range(3)]  # W2V[a][b] = viewmatrix[b][a]
    T = [f64(vm[3, a]) for a in range(3)]
    d0 = f64(np.asarray(depth_map, np.float32).reshape(-1)[int(pixel)])
    d = f64(-1.0) if d0 == 0 else -d0
    z = [Rw[a][2] for a in range(3)]
    focal = [T[a] + d * z[a] for a in range(3)]
    offset = [T[a] - focal[a] for a in range(3)]
    c, s = f64(cos_t), f64(sin_t)
    views, projs, Rs, Ts = [], [], [], []
    for axis, sk in (("y", s), ("y", -s), ("x", s), ("x", -s)):
        A = rotation_matrix(axis, c, sk)
        Rk = [[_dot3(A[i], [Rw[0][j], Rw[1][j], Rw[2][j]]) for j in range(3)] for i in range(3)]
        Tk = [_dot3(A[i], offset) + focal[i] for i in range(3)]
        V = [[Rk[i][0], Rk[i][1], Rk[i][2], f64(0.0)] for i in range(3)] + [[Tk[0], Tk[1], Tk[2], f64(1.0)]]
        Pm = [[((V[r][0] * Q[0][q] + V[r][1] * Q[1][q]) + V[r][2] * Q[2][q]) + V[r][3] * Q[3][q] for q in range(4)] for r in range(4)]
        views.append(np.array(V, np.float64).astype(np.float32))
        projs.append(np.array(Pm, np.float64).astype(np.float32))
        Rs.append(np.array(Rk, np.float64)), Ts.append(np.array(Tk, np.float64))
    return dict(viewmatrix=np.stack(views), projmatrix=np.stack(projs), focal=np.array(focal, np.float64).astype(np.float32),
                R=np.stack(Rs), T=np.stack(Ts), Rw=np.array(Rw, np.float64), T0=np.array(T, np.float64), focal64=np.array(focal, np.float64),
                offset=np.array(offset, np.float64), d=float(d))


def prune_oracle(state, touched, window, park, invalid_renders=0, valid_renders=4):
    """state: CPU tensors in the single map's layout (dqo_mapgrowth.PRUNE_STATE); touched [P]: the sum of the four renders' n_touched
    (any non-zero value = touched); window = (lo, hi).  invalid_renders > 0: some render overflowed — nothing is deleted.  Returns
    dict(state, fate [P] (index into FATES), stats [8])."""
    P = int(state["xyz"].shape[0])
    lo, hi = int(window[0]), int(window[1])
    alive = state["alive"].bool()
    is_stable = alive & state["stable"].bool()
    rows = torch.arange(P)
    n_touched_map = torch.as_tensor(touched).reshape(-1).long()
    unstable_rows, stable_rows = rows[alive & ~is_stable], rows[is_stable]
    # global_params = cat(unstable, stable) (:490-495)
    cat_rows = torch.cat([unstable_rows, stable_rows])
    unstable_num = int(unstable_rows.numel())
    frame_ids = state["frame_id"].long()[cat_rows]
    n_touched = n_touched_map[cat_rows]
    id_mask = torch.logical_and(frame_ids > lo, frame_ids <= hi)  # (:510-515; one keyframe: lo = uid - 1, hi = uid)
    mask = torch.logical_and(n_touched == 0, id_mask)
    skipped = int(invalid_renders) > 0
    if skipped:
        mask = torch.zeros_like(mask)
    unstable_mask, stable_mask = mask[:unstable_num], mask[unstable_num:]
    gone_unstable, gone_stable = unstable_rows[unstable_mask], stable_rows[stable_mask]  # pointcloud.delete / stable_pointcloud.delete
    fate = torch.zeros(P, dtype=torch.long)
    fate[cat_rows] = FATES.index("outside_window")
    fate[cat_rows[id_mask]] = FATES.index("kept_skipped" if skipped else "kept_touched")
    fate[gone_unstable], fate[gone_stable] = FATES.index("deleted_unstable"), FATES.index("deleted_stable")
    out = {k: v.clone() for k, v in state.items()}
    gone = torch.cat([gone_unstable, gone_stable])
    out["xyz"][gone] = torch.as_tensor(park, dtype=out["xyz"].dtype).reshape(1, 3)
    for k, v in FREED.items():
        out[k][gone] = v
    stats = [int(id_mask.sum()), int(gone_unstable.numel()), int(gone_stable.numel()), int(valid_renders), int(skipped),
             int(alive.sum()) - int(gone.numel()), 0, 0]
    return dict(state=out, fate=fate, stats=stats)
