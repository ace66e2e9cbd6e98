"""Host-side mirror of the dual-quadric fit of DQO-MAP (SLAM/multiprocess/quadrics.py) on top of libdqoraster.so.

`Ellipsoid_tensor` keeps the reference's class name and `forward(P)` meaning (quadrics.py:2144-2220: parameters axes_, R_,
center_; returns the projected axis-aligned bbox), `bboxes_iou` is quadrics.py:285-290, and `optimize_objects` is the
inner loop of `Object_Optimize_only` (quadrics.py:2251-2285) for ALL objects of a keyframe in one kernel launch instead
of ~60 eager launches x 20 iterations x objects.  GPU only.
"""
import torch

import _dqo_native as N


def _gpu_f32(x, dev):
    return torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()


def quadric_iou_fwd_bwd(axes, R, center, P34, obs_bbox):
    """Batched residual over B (object, view) pairs.  Returns dict(bbox[B,4], loss[B], valid[B], g_axes, g_R, g_center)."""
    if not (torch.is_tensor(axes) and axes.is_cuda):
        raise RuntimeError("quadric_iou_fwd_bwd needs GPU (ROCm) tensors; there is no CPU path.")
    dev = axes.device
    axes = _gpu_f32(axes, dev).reshape(-1, 3)
    B = axes.size(0)
    R, center = _gpu_f32(R, dev).reshape(B, 3, 3), _gpu_f32(center, dev).reshape(B, 3)
    P34, obs = _gpu_f32(P34, dev).reshape(B, 3, 4), _gpu_f32(obs_bbox, dev).reshape(B, 4)
    out = dict(bbox=torch.empty((B, 4), device=dev), loss=torch.empty((B,), device=dev),
               valid=torch.empty((B,), dtype=torch.int32, device=dev), g_axes=torch.empty((B, 3), device=dev),
               g_R=torch.empty((B, 3, 3), device=dev), g_center=torch.empty((B, 3), device=dev))
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_quadric_iou_fwd_bwd(B, N.ptr(axes), N.ptr(R), N.ptr(center), N.ptr(P34), N.ptr(obs), N.ptr(out["bbox"]),
                                                N.ptr(out["loss"]), N.ptr(out["valid"]), N.ptr(out["g_axes"]), N.ptr(out["g_R"]),
                                                N.ptr(out["g_center"]), N.current_stream()))
    return out


class _QuadricResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axes, R, center, P34, obs):
        o = quadric_iou_fwd_bwd(axes, R, center, P34, obs)
        ctx.save_for_backward(o["g_axes"], o["g_R"], o["g_center"])
        ctx.shapes = (axes.shape, R.shape, center.shape)
        return o["loss"], o["bbox"]

    @staticmethod
    def backward(ctx, g_loss, g_bbox):
        ga, gR, gc = ctx.saved_tensors
        sa, sR, sc = ctx.shapes
        return ((ga * g_loss[:, None]).reshape(sa), (gR * g_loss[:, None, None]).reshape(sR), (gc * g_loss[:, None]).reshape(sc),
                None, None)


def bboxes_iou(bb1, bb2):
    """quadrics.py:285-290 on tensors/floats (python min/max semantics)."""
    inter_w = max(min(bb1[2], bb2[2]) - max(bb1[0], bb2[0]), 0)
    inter_h = max(min(bb1[3], bb2[3]) - max(bb1[1], bb2[1]), 0)
    area_inter = inter_w * inter_h
    return area_inter / ((bb1[2] - bb1[0]) * (bb1[3] - bb1[1]) + (bb2[2] - bb2[0]) * (bb2[3] - bb2[1]) - area_inter)


class Ellipsoid_tensor(torch.nn.Module):
    """quadrics.py:2144-2220.  forward(P) returns the projected bbox; `residual(P, obs)` the fused 1 - IoU loss."""

    def __init__(self, axes, R, center, bbox=None, device="cuda"):
        super().__init__()
        self.axes_ = torch.nn.Parameter(torch.as_tensor(axes, dtype=torch.float32, device=device).clone())
        self.R_ = torch.nn.Parameter(torch.as_tensor(R, dtype=torch.float32, device=device).clone())
        self.center_ = torch.nn.Parameter(torch.as_tensor(center, dtype=torch.float32, device=device).clone())
        self.bbox = bbox

    def residual(self, P, obs_bbox):
        dev = self.axes_.device
        loss, bbox = _QuadricResidual.apply(self.axes_[None], self.R_[None], self.center_[None], _gpu_f32(P, dev)[None],
                                            _gpu_f32(obs_bbox, dev)[None])
        return loss[0], bbox[0]

    def forward(self, P):
        dev = self.axes_.device
        o = quadric_iou_fwd_bwd(self.axes_.detach()[None], self.R_.detach()[None], self.center_.detach()[None],
                                _gpu_f32(P, dev)[None], torch.zeros((1, 4), device=dev))
        return o["bbox"][0]


def optimize_objects(axes, R, center, P34_views, obs_views, view_offset, view_schedule):
    """Object_Optimize_only inner loops (quadrics.py:2251-2285) for n_obj objects in one launch.

    axes[n,3], R[n,3,3], center[n,3]: initial ellipsoids (updated copies are returned);
    P34_views[V,3,4], obs_views[V,4]: all stored (K @ Rt, detection bbox) pairs, object o owning rows
    view_offset[o]:view_offset[o+1]; view_schedule[n, n_iters] int32: view used at each iteration (negative = from the end;
    the reference draws random.randint for iter <= 5 and uses -1 afterwards).  Returns (axes, R, center, loss_hist[n, n_iters]).
    """
    if not (torch.is_tensor(axes) and axes.is_cuda):
        raise RuntimeError("optimize_objects needs GPU (ROCm) tensors; there is no CPU path.")
    dev = axes.device
    axes = _gpu_f32(axes, dev).reshape(-1, 3).clone()
    n = axes.size(0)
    R, center = _gpu_f32(R, dev).reshape(n, 3, 3).clone(), _gpu_f32(center, dev).reshape(n, 3).clone()
    P34_views, obs_views = _gpu_f32(P34_views, dev).reshape(-1, 3, 4), _gpu_f32(obs_views, dev).reshape(-1, 4)
    view_offset = torch.as_tensor(view_offset, dtype=torch.int32, device=dev).contiguous()
    view_schedule = torch.as_tensor(view_schedule, dtype=torch.int32, device=dev).reshape(n, -1).contiguous()
    n_iters = view_schedule.size(1)
    hist = torch.empty((n, n_iters), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_quadric_adam(n, n_iters, N.ptr(view_offset), N.ptr(P34_views), N.ptr(obs_views), N.ptr(view_schedule),
                                         N.ptr(axes), N.ptr(R), N.ptr(center), N.ptr(hist), N.current_stream()))
    return axes, R, center, hist


FATES = ("dropped", "invalidated", "matched", "new", "replaced", "unmatched")  # det_fate of dqo_objmap_frame, include/dqo_raster.h
FRAME_HEADER = ("accepted", "matched", "new", "replaced", "removed", "has_new_object", "overflow_obj", "overflow_views")
_TABLE = ("obj_axes", "obj_R", "obj_center", "obj_cat", "obj_uid", "obj_nviews", "view_P34", "view_bbox", "state")


class ObjectMap:
    """The device-resident object table and the reference's per-frame object stage (mapper.py:147-165, 204-205, 1503-1534) on it:
    `frame` is detections_filter + ObjectsInitialization / Occlusions_Check + MatchObject + remove_outlier in one launch
    (dqo_objmap_frame), `optimize` Object_Optimize_only over the rows that frame flagged (dqo_objmap_optimize), `mean_iou` record_iou
    (dqo_objmap_mean_iou).  `frame`, `optimize` and `mean_iou` read nothing back; `to_host` and `view_csr` (a gather for callers of
    `optimize_objects`, not needed between `frame` and `optimize`) do.  include/dqo_raster.h states the contract, INTEGRATION.md §4k the
    statement-by-statement map.  GPU only.

    Full tables never write past their capacity: the object or observation is dropped and counted in the frame header, and the count
    accumulates in a device word that `to_host` reads (and raises on)."""

    def __init__(self, cap_obj=256, cap_views=64, cap_det=64, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ObjectMap needs a GPU (ROCm) device; there is no CPU path.")
        if not (1 <= cap_obj <= 1024 and cap_views >= 2 and 1 <= cap_det <= 64 and cap_obj * cap_views * 12 <= 2 ** 31 - 1):
            raise ValueError(f"ObjectMap: cap_obj {cap_obj} (1 to 1024), cap_views {cap_views} (2 or more), cap_det {cap_det} (1 to 64)")
        self.cap_obj, self.cap_views, self.cap_det, self.device = int(cap_obj), int(cap_views), int(cap_det), dev
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        self.obj_axes, self.obj_R, self.obj_center = z((cap_obj, 3)), z((cap_obj, 9)), z((cap_obj, 3))
        self.obj_cat, self.obj_uid, self.obj_nviews = (z((cap_obj,), torch.int32) for _ in range(3))
        self.view_P34, self.view_bbox = z((cap_obj, cap_views, 12)), z((cap_obj, cap_views, 4))
        self.state = z((3,), torch.int32)  # object count, next uid, whether the first-frame branch has been taken
        self.opt_flag = z((cap_obj,), torch.uint8)
        self.overflow = z((2,), torch.int32)  # objects / observations dropped so far

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            N.check(fn(*args, N.current_stream()))

    def _table_ptrs(self, names):
        return [N.ptr(getattr(self, n)) for n in names]

    def frame(self, dets, depth, K, Rt, frame_id, seed):
        """One frame with detections.  dets: dict(bbox [M,4], ellipse [M,5] (centre, full axes, angle), cat [M], score [M]); depth [H,W];
        K [3,3]; Rt [3,4] (or [4,4]).  Returns dict(fate [M] int32 (index into FATES), row [M] int32, depth [M,2], opt_flag [cap_obj] uint8,
        header [8] int32 (FRAME_HEADER)) of device tensors, without synchronising.  No detections: nothing runs (mapper.py:148)."""
        dev = self.device
        bbox = _gpu_f32(dets["bbox"], dev).reshape(-1, 4)
        M = bbox.size(0)
        if M > self.cap_det:
            raise ValueError(f"ObjectMap.frame: {M} detections exceed cap_det = {self.cap_det}")
        out = dict(fate=torch.zeros((M,), dtype=torch.int32, device=dev), row=torch.full((M,), -1, dtype=torch.int32, device=dev),
                   depth=torch.zeros((M, 2), device=dev), opt_flag=self.opt_flag, header=torch.zeros((8,), dtype=torch.int32, device=dev))
        if M == 0:
            self.opt_flag.zero_()
            return out
        ell = _gpu_f32(dets["ellipse"], dev).reshape(M, 5)
        cat = torch.as_tensor(dets["cat"], device=dev).to(torch.int32).reshape(M).contiguous()
        score = _gpu_f32(dets["score"], dev).reshape(M)
        depth = _gpu_f32(depth, dev)
        if depth.dim() == 3 and depth.size(0) == 1:  # the frame map's [1, H, W]
            depth = depth[0]
        if depth.dim() != 2:
            raise ValueError("ObjectMap.frame: depth must be [H, W]")
        H, W = depth.shape
        K = _gpu_f32(K, dev).reshape(3, 3)
        Rt = _gpu_f32(Rt, dev).reshape(-1, 4)[:3].contiguous()
        self._call(N.lib().dqo_objmap_frame, self.cap_obj, self.cap_views, self.cap_det, *self._table_ptrs(_TABLE), M, N.ptr(bbox), N.ptr(ell),
                   N.ptr(cat), N.ptr(score), N.ptr(depth), N.ptr(K), N.ptr(Rt), int(W), int(H), int(frame_id) & 0x7FFFFFFF,
                   int(seed) & (2 ** 64 - 1), N.ptr(out["fate"]), N.ptr(out["row"]), N.ptr(out["depth"]), N.ptr(self.opt_flag),
                   N.ptr(out["header"]))
        self.overflow += out["header"][6:8]
        return out

    def optimize(self, frame_id, seed, loss_hist=False):
        """Object_Optimize_only (quadrics.py:2234-2298) for every row the last frame flagged: 20 Adam steps in place, the view of step
        `it` from the key rule over (seed, frame_id, uid, it) for it <= 5 and the last observation afterwards.  Returns the loss history
        [cap_obj, 20] when asked for (rows that were not flagged stay zero), else None."""
        hist = torch.zeros((self.cap_obj, 20), device=self.device) if loss_hist else None
        self._call(N.lib().dqo_objmap_optimize, self.cap_obj, self.cap_views, *self._table_ptrs(
            ("obj_axes", "obj_R", "obj_center", "obj_uid", "obj_nviews", "view_P34", "view_bbox", "state")), N.ptr(self.opt_flag),
            int(frame_id) & 0x7FFFFFFF, int(seed) & (2 ** 64 - 1), N.ptr(hist))
        return hist

    def mean_iou(self):
        """record_iou (mapper.py:1512-1531): each row's mean IoU over its stored observations with IoU > 0, 0 with none; [cap_obj]."""
        out = torch.empty((self.cap_obj,), device=self.device)
        self._call(N.lib().dqo_objmap_mean_iou, self.cap_obj, self.cap_views, *self._table_ptrs(
            ("obj_axes", "obj_R", "obj_center", "obj_nviews", "view_P34", "view_bbox", "state")), N.ptr(out))
        return out

    def view_csr(self, rows=None):
        """(P34_views [V,3,4], obs_views [V,4], view_offset [n+1]) of `rows` (default: every object), gathered in row and append order:
        what optimize_objects takes.  Reads the counts back."""
        n = int(self.state[0].item())
        rows = list(range(n)) if rows is None else [int(r) for r in rows]
        counts = self.obj_nviews.cpu().tolist()
        off = [0]
        for r in rows:
            off.append(off[-1] + counts[r])
        if rows:
            P = torch.cat([self.view_P34[r, :counts[r]] for r in rows]).reshape(-1, 3, 4)
            ob = torch.cat([self.view_bbox[r, :counts[r]] for r in rows]).reshape(-1, 4)
        else:
            P, ob = torch.zeros((0, 3, 4), device=self.device), torch.zeros((0, 4), device=self.device)
        return P, ob, torch.tensor(off, dtype=torch.int32, device=self.device)

    def to_host(self):
        """One dict per object in row order: category, uid, axes [3], R [3,3], center [3], bboxes [n,4], P34 [n,3,4].  The one place
        that reads back; raises when an object or an observation has been dropped for lack of room."""
        over = self.overflow.cpu().tolist()
        if over[0] or over[1]:
            raise RuntimeError(f"ObjectMap overflow: {over[0]} objects beyond cap_obj = {self.cap_obj} and {over[1]} observations beyond "
                               f"cap_views = {self.cap_views} were dropped")
        h = {k: getattr(self, k).cpu().numpy() for k in _TABLE}
        return [dict(category=int(h["obj_cat"][i]), uid=int(h["obj_uid"][i]), axes=h["obj_axes"][i].copy(), R=h["obj_R"][i].reshape(3, 3).copy(),
                     center=h["obj_center"][i].copy(), bboxes=h["view_bbox"][i, :h["obj_nviews"][i]].copy(),
                     P34=h["view_P34"][i, :h["obj_nviews"][i]].reshape(-1, 3, 4).copy()) for i in range(int(h["state"][0]))]

    def state_dict(self):
        d = {k: getattr(self, k).clone() for k in _TABLE + ("opt_flag", "overflow")}
        d["capacities"] = torch.tensor([self.cap_obj, self.cap_views, self.cap_det], dtype=torch.int32)
        return d

    def load_state_dict(self, d):
        caps = [int(x) for x in d["capacities"]]
        if caps[:2] != [self.cap_obj, self.cap_views]:
            raise ValueError(f"ObjectMap.load_state_dict: capacities {caps[:2]} do not match {[self.cap_obj, self.cap_views]}")
        for k in _TABLE + ("opt_flag", "overflow"):
            getattr(self, k).copy_(d[k].to(self.device))
