"""CPU oracle of the map-maintenance step (FusedMapper.maintain / dqo_mapgrowth.lifecycle_step): a literal two-cloud restatement of the
statements that close every frame of the reference mapper — SLAM/multiprocess/mapper.py:214 (optional), 217-219:

    gaussians_delete(unstable=False)   :692-730
    gaussians_fix()                    :657-676
    error_gaussians_remove()           :989-1102   (with gaussians_release, :679-689)
    gaussians_delete()                 :692-730

Two clouds (dicts of tensors with the reference's delete / remove / cat semantics, SLAM/gaussian_pointcloud.py:210-293, 415-432) and a
hidden `row_id` column that says which row of the single map a Gaussian came from.  The per-Gaussian maxima are scattered with
np.maximum.at, the thresholds compared with torch's own `>` on float32 tensors.  No GPU, no project code."""
import numpy as np
import torch

FREED = dict(opacity_raw=-10.0, scaling_raw=-10.0, alive=0, row_flags=3, confidence=0.0, stable=0, add_tick=0, depth_error_counter=0,
             color_error_counter=0)  # (+ xyz = park): what a deleted row holds
FATES = ("spare", "unstable", "stable", "deleted_depth", "deleted_oversized_unstable", "deleted_time", "deleted_oversized_stable")
COLUMNS = ("row_id", "scaling_raw", "confidence", "add_tick", "depth_error_counter", "color_error_counter")


class Cloud:
    """One of the reference's two GaussianPointCloud objects, reduced to the columns the maintenance statements touch."""

    def __init__(self, cols):
        self.c = {k: v.clone() for k, v in cols.items()}

    @property
    def num(self):
        return int(self.c["row_id"].shape[0])

    @property
    def radius(self):  # get_radius, gaussian_pointcloud.py:739-743
        sc = torch.exp(self.c["scaling_raw"])
        return (torch.sum(sc, dim=-1, keepdim=True) - torch.min(sc, dim=-1, keepdim=True)[0]) / 2

    def delete(self, mask):  # :210-232
        gone = self.c["row_id"][mask]
        self.c = {k: v[~mask] for k, v in self.c.items()}
        return gone

    def remove(self, mask):  # :235-293
        params = {k: v[mask] for k, v in self.c.items()}
        self.c = {k: v[~mask] for k, v in self.c.items()}
        return params

    def cat(self, params):  # :415-432
        self.c = {k: torch.cat([v, params[k]]) for k, v in self.c.items()}


class Margin:
    """The smallest relative distance of a float quantity from the threshold it was compared with."""

    def __init__(self):
        self.value = float("inf")

    def see(self, values, threshold):
        v = np.asarray(values, np.float64).reshape(-1)
        t = float(threshold)
        if v.size and t != 0.0:
            self.value = min(self.value, float(np.min(np.abs(v - t) / abs(t))))


def _gaussians_delete(cloud, time, window, unstable, margin, fate):
    if cloud.num == 0:  # :697
        return 0, 0
    radius = cloud.radius
    limit = radius.mean() * 10
    margin.see(radius.numpy(), float(limit))
    big = (radius > limit).squeeze(-1)
    old = ((time - cloud.c["add_tick"]) > window)
    delete_mask = (big | old) if unstable else big
    ids = cloud.c["row_id"]
    if unstable:
        fate[ids[big]] = FATES.index("deleted_oversized_unstable")
        fate[ids[old & ~big]] = FATES.index("deleted_time")
    else:
        fate[ids[big]] = FATES.index("deleted_oversized_stable")
    cloud.delete(delete_mask)
    return int(big.sum()), int((old & ~big).sum()) if unstable else 0


def lifecycle_oracle(state, tick, gt_color, gt_depth, render_color, render_depth, depth_index, color_index, *, stable_confidence_thres,
                     unstable_time_window, add_color_thres, add_depth_thres, delete_thresh=10, stable_oversized=False, park):
    """state: CPU tensors in the single map's layout (xyz [P,3], opacity_raw [P,1], scaling_raw [P,3], confidence, alive, row_flags,
    stable, add_tick, depth_error_counter, color_error_counter [P]); images [C,H,W] / index maps [1,H,W] in MAP rows, or all four None.
    Returns dict(state = the expected single-map state after the step, fate [P] (index into FATES), stats [8], margin)."""
    P = int(state["xyz"].shape[0])
    alive = state["alive"].bool()
    is_stable = alive & state["stable"].bool()
    rows = torch.arange(P)
    pick = lambda m: Cloud(dict(row_id=rows[m], scaling_raw=state["scaling_raw"][m].float(), confidence=state["confidence"][m].float().reshape(-1),
                                add_tick=state["add_tick"][m].long(), depth_error_counter=state["depth_error_counter"][m].long(),
                                color_error_counter=state["color_error_counter"][m].long()))
    pointcloud, stable_pointcloud = pick(alive & ~is_stable), pick(is_stable)
    margin = Margin()
    fate = torch.zeros(P, dtype=torch.long)
    stats = [0] * 8
    time = int(tick)

    # mapper.py:214 (optimise frames)
    if stable_oversized:
        stats[5], _ = _gaussians_delete(stable_pointcloud, time, unstable_time_window, False, margin, fate)

    # gaussians_fix, :657-676
    thres = float(stable_confidence_thres)
    stable_mask = pointcloud.c["confidence"] > thres
    stats[0] = int(stable_mask.sum())
    if stable_mask.sum() > 0:
        stable_params = pointcloud.remove(stable_mask)
        stable_params["confidence"] = torch.clip(stable_params["confidence"], max=thres)
        stable_pointcloud.cat(stable_params)

    # error_gaussians_remove, :989-1102
    if render_color is not None and stable_pointcloud.num > 0:
        unstable_points_num, stable_points_num = pointcloud.num, stable_pointcloud.num
        n = unstable_points_num + stable_points_num
        # global_params = cat(unstable, stable): the render's index maps name MAP rows, the reference's name positions of that cat
        where = torch.full((P,), n, dtype=torch.long)  # (a row that is no Gaussian of the map: outside [0, n), scattered nowhere)
        where[pointcloud.c["row_id"]] = torch.arange(unstable_points_num)
        where[stable_pointcloud.c["row_id"]] = unstable_points_num + torch.arange(stable_points_num)
        to_cat = lambda idx: torch.where((idx >= 0) & (idx < P), where[idx.long().clamp(0, P - 1)], torch.where(idx == -1, idx.long(), n))
        color, depth = render_color.permute(1, 2, 0).float(), render_depth.permute(1, 2, 0).float()
        color_map, depth_map = gt_color.permute(1, 2, 0).float(), gt_depth.permute(1, 2, 0).float()
        d_index, c_index = to_cat(depth_index.permute(1, 2, 0)), to_cat(color_index.permute(1, 2, 0))
        depth_error = torch.abs(depth_map - depth)
        depth_error[(depth_map - depth) < 0] = 0
        image_error = torch.abs(color_map - color)
        color_error = ((image_error[..., 0] + image_error[..., 1]) + image_error[..., 2])[..., None]  # torch.sum(image_error, dim=-1)
        invalid_mask = ((depth_map == 0) | (d_index == -1)).squeeze(-1)
        depth_error[invalid_mask] = 0
        color_error[depth_map == 0] = 0
        color_filter_thres, depth_filter_thres = 2 * float(add_color_thres), 2 * float(add_depth_thres)
        margin.see(color_error.numpy(), np.float32(color_filter_thres))
        margin.see(depth_error.numpy(), np.float32(depth_filter_thres))
        # accumulate_gaussian_error(..., check_max=True): per-Gaussian maxima from zero (cuda_utils map_process.cu:33-120)
        g_color, g_depth = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ci, di = c_index.reshape(-1).numpy(), d_index.reshape(-1).numpy()
        ce, de = color_error.reshape(-1).numpy(), depth_error.reshape(-1).numpy()
        ok = (ci >= 0) & (ci < n) & ~np.isnan(ce)
        np.maximum.at(g_color, ci[ok], ce[ok])
        ok = (di >= 0) & (di < n) & ~np.isnan(de)
        np.maximum.at(g_depth, di[ok], de[ok])
        depth_delete_mask = torch.from_numpy(g_depth) > depth_filter_thres
        color_release_mask = torch.from_numpy(g_color) > color_filter_thres
        depth_delete_mask_stable = depth_delete_mask[unstable_points_num:]
        color_release_mask_stable = color_release_mask[unstable_points_num:]
        stable_pointcloud.c["depth_error_counter"][depth_delete_mask_stable] += 1
        stable_pointcloud.c["color_error_counter"][color_release_mask_stable] += 1
        depth_delete_mask = stable_pointcloud.c["depth_error_counter"] >= delete_thresh
        color_release_mask = stable_pointcloud.c["color_error_counter"] >= delete_thresh
        fate[stable_pointcloud.delete(depth_delete_mask)] = FATES.index("deleted_depth")
        stats[2] = int(depth_delete_mask.sum())
        # gaussians_release(color_release_mask[~depth_delete_mask]), :679-689
        mask = color_release_mask[~depth_delete_mask]
        stats[1] = int(mask.sum())
        if mask.sum() > 0:
            unstable_params = stable_pointcloud.remove(mask)
            unstable_params["confidence"] = torch.zeros_like(unstable_params["confidence"])
            unstable_params["add_tick"] = time * torch.ones_like(unstable_params["add_tick"])
            pointcloud.cat(unstable_params)

    # gaussians_delete(), :692-730
    stats[3], stats[4] = _gaussians_delete(pointcloud, time, unstable_time_window, True, margin, fate)
    stats[6], stats[7] = pointcloud.num, stable_pointcloud.num

    out = {k: v.clone() for k, v in state.items()}
    gone = alive.clone()
    for cloud, flag in ((pointcloud, 0), (stable_pointcloud, 1)):
        ids = cloud.c["row_id"]
        gone[ids] = False
        fate[ids] = FATES.index("stable" if flag else "unstable")
        out["stable"][ids] = flag
        out["confidence"][ids] = cloud.c["confidence"].to(out["confidence"].dtype)
        for k in ("add_tick", "depth_error_counter", "color_error_counter"):
            out[k][ids] = cloud.c[k].to(out[k].dtype)
    out["xyz"][gone] = torch.as_tensor(park, dtype=out["xyz"].dtype).reshape(1, 3)
    for k, v in FREED.items():
        out[k][gone] = v
    return dict(state=out, fate=fate, stats=stats, margin=margin.value)
