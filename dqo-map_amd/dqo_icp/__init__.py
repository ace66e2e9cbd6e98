"""Point-to-plane ICP of DQO-MAP's tracker on MI355X.

`ICP` mirrors the class of /root/reference/SLAM/icp.py:16-129 (same constructor arguments, same `icp(...)` signature and return
value).  Per Gauss-Newton iteration the reference builds residuals, Jacobians and the 6x6 normal equations with ~40 eager torch
kernels; here that is one call of libdqoraster.so's dqo_icp_normal_equations (csrc/icp.hip).  The damped 6x6 solve and the
se(3) exponential (icp.py:248-337) are restated in double precision on the host, where the reference also runs them
(its invH moves the matrix to the CPU).  GPU only: there is no CPU path.

The rest of the tracker's per-frame work runs on the device as well (csrc/track.hip, the Gauss-Newton kernel of csrc/icp.hip):
`preprocess_frame` is the geometry half of Tracker.map_preprocess (SLAM/multiprocess/tracker.py:118-165), and `IcpTracker` mirrors
SLAM/icp.py:361-458 (pyramids, model-depth fill, the coarse-to-fine loop, the failure test) as stream-ordered launches whose only
host synchronisation is predict_pose's read of the result.

`Trajectory` takes the pose from there (csrc/map_traj.hip): the world pose, the frame's camera tensors, the world-frame vertex / normal
maps, the keyframe test and the ATE curve (Tracker.tracking, SLAM/multiprocess/tracker.py:307-339; check_keyframe, mapper.py:734-773;
eval_total_ate, tracker.py:341-346) from predict_pose_async's device tensors, with no host read per frame.  Poses that come back
corrected (Mapping.update_poses, SLAM/multiprocess/mapper.py:256-263; pose_es.npy) go through `Trajectory.update_poses` and
`cameras_from_poses` (csrc/map_repose.hip): the store and every camera that follows it in one launch.
"""
import ctypes
import math

import numpy as np
import torch

import _dqo_native as N


def normal_equations(vertex0, vertex1, normal0, normal1, pose10, K, distance_threshold, normal_threshold):
    """(JtJ [6,6], JtR [6,1], valid_count 0-dim int32) of ICP.compute_residuals_jacobian + compute_jtj + compute_jtr."""
    N.require_gpu_op(vertex0, vertex1, normal0, normal1)
    dev = vertex0.device
    H, W = vertex0.shape[:2]
    v0, v1, n0, n1 = (t.float().contiguous() for t in (vertex0, vertex1, normal0, normal1))
    pose = pose10.to(device=dev, dtype=torch.float32).contiguous()
    Kc = K.detach().cpu() if torch.is_tensor(K) else torch.as_tensor(K)
    fx, fy, cx, cy = float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])
    lib = N.lib()
    JtJ = torch.empty((6, 6), dtype=torch.float32, device=dev)
    JtR = torch.empty((6, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.dqo_icp_workspace_bytes(),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.dqo_icp_normal_equations(H, W, N.ptr(v0), N.ptr(v1), N.ptr(n0), N.ptr(n1), N.ptr(pose), fx, fy, cx, cy,
                                             float(distance_threshold), float(normal_threshold), N.ptr(JtJ), N.ptr(JtR), N.ptr(cnt),
                                             N.ptr(ws), ws.numel(), N.current_stream()))
    return JtJ, JtR, cnt[0]


def lev_mar_H(JtWJ, damping):
    """icp.py:248-256: JtJ + damping * trace(JtJ) * I."""
    eye = torch.eye(6, dtype=JtWJ.dtype, device=JtWJ.device)
    return JtWJ + (torch.sum(eye * JtWJ) * damping) * eye


def exp_se3(xi):
    """icp.py:272-312 (rotation first, then translation through the left Jacobian), float64 on the host."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    wh = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    wh2 = wh @ wh
    th = float(np.linalg.norm(w))
    if th <= 1e-8:
        ew, j = np.eye(3), np.eye(3)
    else:
        ew = np.eye(3) + wh * math.sin(th) / th + wh2 * (1.0 - math.cos(th)) / th ** 2
        j = np.eye(3) + (1.0 - math.cos(th)) / th ** 2 * wh + (th - math.sin(th)) / th ** 3 * wh2
    T = np.eye(4)
    T[:3, :3] = ew
    T[:3, 3] = j @ v
    return T


def forward_update_pose(H, Rhs, pose):
    """icp.py:259-269, 331-337: xi = -H^-1 Rhs (pinv when singular), pose <- exp(xi) pose."""
    Hn = H.detach().double().cpu().numpy()
    inv = np.linalg.pinv(Hn) if np.linalg.det(Hn) == 0 else np.linalg.inv(Hn)
    xi = -inv @ Rhs.detach().double().cpu().numpy().reshape(6)
    return torch.as_tensor(exp_se3(xi), dtype=pose.dtype, device=pose.device) @ pose


class ICP:
    def __init__(self, max_iter=3, damping=1e-6, distance_threshold=0.2, normal_threshold=20, verbose=False):
        self.max_iterations = max_iter
        self.distance_threshold = distance_threshold
        self.normal_threshold = np.cos(np.deg2rad(normal_threshold))
        self.damping = damping
        self.verbose = verbose

    def icp(self, pose10, vertex_t0, vertex_t1, normal_t0, normal_t1, K):
        cnt = None
        for _ in range(self.max_iterations):
            JtWJ, JtR, cnt = normal_equations(vertex_t0, vertex_t1, normal_t0, normal_t1, pose10, K, self.distance_threshold,
                                              self.normal_threshold)
            pose10 = forward_update_pose(lev_mar_H(JtWJ, self.damping), JtR, pose10)
        H, W = vertex_t0.shape[:2]
        return pose10, cnt / H / W

    __call__ = icp


_K_UPLOADS = {}  # (device, the nine fp32 values) -> the device copy of a host intrinsic matrix


def _k_device(K, dev):
    """K as a row-major 3x3 fp32 tensor on `dev` for the kernels, which read the intrinsics from device memory: no host read.
    A GPU tensor is used where it is (converted on the device when it is not fp32 / contiguous), so a caller that builds a fresh GPU
    intrinsic every frame pays nothing.  A host matrix (CPU tensor, numpy array, nested list) is uploaded once per distinct value and
    device and the upload reused, which keeps repeated calls (a graph capture among them) free of copies; its values are read on
    every call, so changing them in place takes effect."""
    if torch.is_tensor(K) and K.is_cuda:
        if K.device != dev:
            raise ValueError(f"intrinsics on {K.device}, maps on {dev}")
        return K.detach().to(torch.float32).reshape(3, 3).contiguous()
    vals = np.asarray(K.detach() if torch.is_tensor(K) else K, dtype=np.float32).reshape(3, 3)
    key = (str(dev), vals.tobytes())
    if key not in _K_UPLOADS:
        if len(_K_UPLOADS) >= 64:
            _K_UPLOADS.clear()
        _K_UPLOADS[key] = torch.tensor(vals, device=dev)
    return _K_UPLOADS[key]


def _depth2d(depth):
    if not (torch.is_tensor(depth) and depth.is_cuda):
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
    if depth.dim() == 3 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth.dim() != 2:
        raise ValueError(f"depth must be [H, W] or [H, W, 1], got {tuple(depth.shape)}")
    return depth.detach().float().contiguous()


def preprocess_frame(depth, K, min_depth, max_depth, invalid_confidence_thresh, depth_filter=False):
    """The geometry half of Tracker.map_preprocess (SLAM/multiprocess/tracker.py:135-156) for a metric depth map [H, W] or [H, W, 1]:
    optional bilateral filter (radius 5, sigma 2 / 2), range mask, vertex / normal / confidence maps and the invalid-confidence mask,
    with depth, vertex, normal and confidence zeroed where that mask is set.  Two launches (csrc/track.hip).

    Returns {"depth_map": like `depth`, "vertex_map_c": [H, W, 3], "normal_map_c": [H, W, 3], "confidence_map": [H, W, 1],
    "invalid_confidence_mask": [H, W] bool}, all new tensors; `depth` is not modified.  The reference differs there: with the
    filter off its depth_map_filter IS depth_map, so the range mask and the zeroing also write into the frame's depth map (and
    frame.original_depth is reassigned from it); a caller that relies on that assigns "depth_map" back itself."""
    d = _depth2d(depth)
    H, W = d.shape
    lib = N.lib()
    dev = d.device
    Kd = _k_device(K, dev)
    out_depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    vertex = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    normal = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    conf = torch.empty((H, W, 1), dtype=torch.float32, device=dev)
    invalid = torch.empty((H, W), dtype=torch.uint8, device=dev)
    ws = torch.empty((max(1, lib.dqo_track_preprocess_workspace_bytes(H, W)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.dqo_track_preprocess(H, W, N.ptr(d), N.ptr(Kd), float(min_depth), float(max_depth), float(invalid_confidence_thresh),
                                         1 if depth_filter else 0, N.ptr(out_depth), N.ptr(vertex), N.ptr(normal), N.ptr(conf),
                                         N.ptr(invalid), N.ptr(ws), ws.numel(), N.current_stream()))
    return {"depth_map": out_depth.view(depth.shape), "vertex_map_c": vertex, "normal_map_c": normal, "confidence_map": conf,
            "invalid_confidence_mask": invalid.view(torch.bool)}


class _TrackBuffers:
    """Device state of an IcpTracker for one image size: three packed pyramid sets (two for the frames, one for the model depth),
    the pose and the scalars of predict_pose_async, and the workspaces.  Allocated once per size."""

    def __init__(self, H, W, levels, dev):
        lib = N.lib()
        self.H, self.W, self.L = H, W, levels
        n = lib.dqo_track_pyramid_pixels(H, W, levels)
        if n <= 0:
            raise ValueError(f"a {H}x{W} depth map has no {levels}-level pyramid")
        self.sizes = [(H >> (levels - 1 - i), W >> (levels - 1 - i)) for i in range(levels)]
        self.offsets = np.concatenate([[0], np.cumsum([h * w for h, w in self.sizes])]).tolist()
        f = dict(dtype=torch.float32, device=dev)
        self.sets = [(torch.empty((n, 3), **f), torch.empty((n, 3), **f)) for _ in range(3)]
        u8 = dict(dtype=torch.uint8, device=dev)
        self.pyr_ws = torch.empty((lib.dqo_track_pyramid_workspace_bytes(),), **u8)
        self.icp_ws = torch.empty((lib.dqo_icp_workspace_bytes(),), **u8)
        self.p2p_ws = torch.empty((lib.dqo_track_p2p_workspace_bytes(),), **u8)
        self.eye = torch.eye(4, **f)
        self.pose = torch.eye(4, **f)
        self.count = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.success = torch.ones((1,), dtype=torch.int32, device=dev)
        self.loss = torch.zeros((1,), **f)
        self.ratio = torch.zeros((1,), **f)
        self.K_pyr = [None] * 3  # the device intrinsics each pyramid set was built with, and the ICP's (kept alive for the kernels)
        self.K_icp = None

    def level(self, s, i, which):
        h, w = self.sizes[i]
        return self.sets[s][which][self.offsets[i]:self.offsets[i + 1]].view(h, w, 3)

    def pyramid(self, s, which):
        return [self.level(s, i, which) for i in range(self.L)]


class IcpTracker:
    """IcpTracker of SLAM/icp.py:361-458 on the device.  Same constructor argument (an object with the reference's attribute names)
    and methods; every method only issues stream-ordered launches, except predict_pose, whose read of the result is the tracker's only
    host synchronisation.  After the first call for an image size, predict_pose_async allocates nothing and does not synchronise, so it
    can be captured in a torch.cuda.graph (the graph holds the buffers of the tracker state it was captured in).  The intrinsics never
    go to the host: the kernels read K from device memory.  A GPU K (DQO-MAP's `frame.get_intrinsic`, a fresh tensor every frame) is
    used where it is; a host K is uploaded once per distinct value and reused (`_k_device`).  A captured graph reads the K tensor it
    was captured with.  A fp32 GPU K that is not contiguous, or not fp32, is converted on the device, which allocates.

    Differences from the reference: on the first frame (no last-frame pyramids) predict_pose returns (identity, True) — the reference
    returns its identity too but then raises a TypeError indexing the missing pyramids for its loss (icp.py:450); the 6x6 solve is in
    double with a Cholesky-or-Jacobi pseudo-inverse; the loss and the valid ratio are printed only when
    `verbose`."""

    def __init__(self, args):
        self.icp_downscales = list(args.icp_downscales)
        self.icp_warmup_frames = args.icp_warmup_frames
        self.icp_use_model_depth = args.icp_use_model_depth
        self.icp_trackers = [ICP(iters, distance_threshold=args.icp_distance_threshold, normal_threshold=args.icp_normal_threshold,
                                 damping=args.icp_damping, verbose=args.verbose) for iters in args.icp_downscale_iters]
        if not 1 <= len(self.icp_downscales) <= 4 or len(self.icp_trackers) != len(self.icp_downscales):
            raise ValueError("icp_downscales: 1 to 4 levels, one entry of icp_downscale_iters per level")
        self.icp_sample_distance_threshold = args.icp_sample_distance_threshold
        self.icp_sample_normal_threshold = args.icp_sample_normal_threshold
        self.icp_fail_threshold = args.icp_fail_threshold
        self.verbose = args.verbose
        self.K = None
        self._bufs = {}
        self._t0 = self._t1 = None  # (buffers, pyramid set) of the last / current frame
        self.depth_t1 = self.last_model_depth = None

    # -- pyramids in the reference's attribute names (views of the device buffers) -------------------------------------------------
    def _pyr(self, ref, which):
        return None if ref is None else ref[0].pyramid(ref[1], which)

    vertex_pyramid_t0 = property(lambda self: self._pyr(self._t0, 0))
    normal_pyramid_t0 = property(lambda self: self._pyr(self._t0, 1))
    vertex_pyramid_t1 = property(lambda self: self._pyr(self._t1, 0))
    normal_pyramid_t1 = property(lambda self: self._pyr(self._t1, 1))

    def _buffers(self, d):
        key = (d.shape[0], d.shape[1], d.device)
        if key not in self._bufs:
            self._bufs[key] = _TrackBuffers(d.shape[0], d.shape[1], len(self.icp_downscales), d.device)
        return self._bufs[key]

    def _build(self, b, s, depth):
        d = _depth2d(depth)
        if d.shape != (b.H, b.W):
            raise ValueError(f"depth map {tuple(d.shape)} does not match the tracker's {b.H}x{b.W} frames")
        v, n = b.sets[s]
        b.K_pyr[s] = _k_device(self.K, d.device)  # the tracker's K (the first one given), as build_vertex_pyramid uses it
        lib = N.lib()
        with torch.cuda.device(d.device):
            N.check(lib.dqo_track_pyramid(b.H, b.W, b.L, N.ptr(d), N.ptr(b.K_pyr[s]), N.ptr(v), N.ptr(n), N.ptr(b.pyr_ws),
                                          b.pyr_ws.numel(), N.current_stream()))

    def update_curr_status(self, depth_t1, K):
        """icp.py:391-396: vertex / normal pyramids of the current frame's depth with the tracker's K (the first one it was given)."""
        if self.K is None:
            self.K = K
        self.depth_t1 = depth_t1
        b = self._buffers(_depth2d(depth_t1))
        s = 0 if self._t0 != (b, 0) else 1  # never the set the last frame's pyramids live in
        self._t1 = (b, s)
        self._build(b, s, depth_t1)

    def move_last_status(self):
        """icp.py:398-401: the current frame becomes the last one (its pyramids are shared until the next update_curr_status)."""
        self._t0 = self._t1
        self.last_model_depth = self.depth_t1

    def update_last_status(self, frame, render_depth, frame_depth, render_normal, frame_normal):
        """icp.py:403-421: render_depth ([H, W] or [H, W, 1], contiguous fp32 on the GPU) takes frame_depth IN PLACE where the two
        disagree (depth difference, empty render, normal angle) and the frame has depth; it becomes the model depth."""
        for t in (render_depth, frame_depth, render_normal, frame_normal):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError("update_last_status: contiguous fp32 GPU tensors expected (render_depth is updated in place)")
        H, W = render_depth.shape[:2]
        if frame_depth.numel() != H * W or render_normal.numel() != 3 * H * W or frame_normal.numel() != 3 * H * W:
            raise ValueError("update_last_status: maps of different sizes")
        lib = N.lib()
        with torch.cuda.device(render_depth.device):
            N.check(lib.dqo_track_fill_model_depth(H, W, N.ptr(render_depth), N.ptr(frame_depth), N.ptr(render_normal), N.ptr(frame_normal),
                                                   float(self.icp_sample_distance_threshold), float(self.icp_sample_normal_threshold),
                                                   N.current_stream()))
        self.last_model_depth = render_depth

    def predict_pose_async(self, frame):
        """predict_pose on the device: (pose_t1_t0 [4, 4] fp32, success [1] int32, p2p loss [1] fp32, valid ratio [1] fp32), tensors
        owned by the tracker (overwritten by the next call for the same image size).  The first frame gives the identity, success 1,
        loss 0 and ratio 0."""
        K, frame_id = frame["K"], frame["frame_id"]
        if self._t1 is None:
            raise RuntimeError("predict_pose before update_curr_status")
        b = self._t1[0]
        if self._t0 is None:
            self.K = K
            b.pose.copy_(b.eye)
            b.success.fill_(1)
            b.loss.zero_()
            b.ratio.zero_()
            return b.pose, b.success, b.loss, b.ratio
        if self._t0[0] is not b:
            raise ValueError("the last and the current frame differ in size")
        if self.icp_use_model_depth and frame_id >= self.icp_warmup_frames:
            self._build(b, 2, self.last_model_depth)
            self._t0 = (b, 2)
        b.K_icp = _k_device(K, b.pose.device)  # held: the launches (or a captured graph) read it
        s0, s1 = self._t0[1], self._t1[1]
        lib = N.lib()
        with torch.cuda.device(b.pose.device):
            stream = N.current_stream()
            b.pose.copy_(b.eye)
            for level, ds in enumerate(self.icp_downscales):
                h, w = b.sizes[level]
                icp = self.icp_trackers[level]
                # icp.py:445-448: the current frame's maps are ICP's frame 0, the last frame's its frame 1
                v0, n0 = b.level(s1, level, 0), b.level(s1, level, 1)
                v1, n1 = b.level(s0, level, 0), b.level(s0, level, 1)
                for _ in range(icp.max_iterations):
                    N.check(lib.dqo_icp_gauss_newton(h, w, N.ptr(v0), N.ptr(v1), N.ptr(n0), N.ptr(n1), N.ptr(b.pose), N.ptr(b.K_icp),
                                                     float(ds), float(icp.distance_threshold), float(icp.normal_threshold), float(icp.damping),
                                                     N.ptr(b.count), N.ptr(b.icp_ws), b.icp_ws.numel(), stream))
            h, w = b.sizes[-1]
            N.check(lib.dqo_track_p2p_loss(h, w, N.ptr(b.level(s0, b.L - 1, 0)), N.ptr(b.level(s1, b.L - 1, 0)), N.ptr(b.level(s0, b.L - 1, 1)),
                                           N.ptr(b.pose), float(self.icp_fail_threshold), N.ptr(b.count), N.ptr(b.loss), N.ptr(b.success),
                                           N.ptr(b.ratio), N.ptr(b.p2p_ws), b.p2p_ws.numel(), stream))
        return b.pose, b.success, b.loss, b.ratio

    def predict_pose(self, frame):
        """icp.py:423-458: (pose_t1_t0 as a float32 numpy [4, 4], tracking_success).  The one host synchronisation of the tracker."""
        if self._t0 is None:
            self.K = frame["K"]
            return np.eye(4, dtype=np.float32), True
        pose, success, loss, ratio = self.predict_pose_async(frame)
        host = torch.cat([pose.reshape(-1), loss, ratio, success.float()]).cpu().numpy()
        if self.verbose:
            print(host[16], host[17])
        return host[:16].reshape(4, 4).copy(), bool(host[18] != 0)


def world_maps(vertex_c, normal_c, c2w, out=None):
    """transform_map of the frame's two maps (SLAM/multiprocess/tracker.py:332-337, SLAM/utils.py:56-63) in one launch
    (dqo_track_world_maps, csrc/map_traj.hip): (vertex_map_w, normal_map_w) = (R v + t, R n) with the float32 c2w [4,4] on the device.
    Maps: contiguous float32 [H,W,3] GPU tensors; normal_c may be None (then normal_map_w is None).  out: (vertex_w, normal_w) to write
    into — an output may be its input; default: new tensors.  A zero vertex maps to t, as the reference's does."""
    N.require_gpu_op((vertex_c, c2w), normal_c)
    maps = [vertex_c, normal_c] + list(out if out is not None else ())
    for t in maps:
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.shape == vertex_c.shape and t.shape[-1] == 3):
            raise RuntimeError("world_maps: contiguous float32 [H,W,3] maps of one size expected")
    if not (c2w.dtype == torch.float32 and c2w.is_contiguous() and c2w.numel() == 16):
        raise RuntimeError("world_maps: c2w must be a contiguous float32 [4,4] tensor")
    vw, nw = out if out is not None else (torch.empty_like(vertex_c), None if normal_c is None else torch.empty_like(normal_c))
    if (normal_c is None) != (nw is None):
        raise RuntimeError("world_maps: the normal map and its output come together")
    H, W = vertex_c.shape[:2]
    with torch.cuda.device(vertex_c.device):
        N.check(N.lib().dqo_track_world_maps(H, W, vertex_c.data_ptr(), None if normal_c is None else normal_c.data_ptr(), c2w.data_ptr(),
                                             vw.data_ptr(), None if nw is None else nw.data_ptr(), N.current_stream()))
    return vw, nw


REPOSE_OUTPUTS = (("c2w", (4, 4)), ("w2c", (4, 4)), ("viewmatrix", (4, 4)), ("projmatrix", (4, 4)), ("campos", (3,)))


def repose_targets(rows, device, c2w=None, w2c=None, viewmatrix=None, projmatrix=None, campos=None):
    """A target table of dqo_traj_repose (DqoReposeTarget, include/dqo_raster.h): int64 [T,6] on the device, entry t = (rows[t], the
    address of entry t of each destination; 0 for a destination that is None).  rows: T trajectory rows, a sequence or an integer GPU
    tensor (then nothing is copied from the host); a destination: a contiguous float32 GPU tensor [T,4,4] ([T,3] for campos; without the
    leading T when T == 1).  The destinations must outlive every launch that reads the table."""
    if torch.is_tensor(rows):
        r = rows.detach().to(device=device, dtype=torch.int64).reshape(-1)
    else:
        r = torch.tensor([int(x) for x in rows], dtype=torch.int64, device=device)
    T = r.numel()
    cols = [r]
    step = None
    for (name, shape), t in zip(REPOSE_OUTPUTS, (c2w, w2c, viewmatrix, projmatrix, campos)):
        if t is None:
            cols.append(torch.zeros_like(r))
            continue
        n = int(np.prod(shape))
        N.require_gpu_op(t)
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == T * n):
            raise RuntimeError(f"repose_targets: {name} must be a contiguous float32 tensor of {T} x {shape}")
        if step is None:
            step = torch.arange(T, dtype=torch.int64, device=device)
        cols.append(step * (4 * n) + t.data_ptr())
    return torch.stack(cols, 1).contiguous()


def _repose(pose, cap, header, new_pose, table, projection, has_projmatrix, bank_state, stats):
    """The dqo_traj_repose launch on the current stream (the caller holds the operands alive)."""
    args = N.DqoTrajRepose(cap=int(cap), n_new=0 if new_pose is None else int(new_pose.shape[0]), T=0 if table is None else int(table.shape[0]),
                           flags=N.REPOSE_HAS_PROJMATRIX if has_projmatrix else 0, pose=pose.data_ptr(), header=header.data_ptr(),
                           new_pose=N.ptr(new_pose), targets=N.ptr(table), projection=N.ptr(projection), bank_state=N.ptr(bank_state),
                           stats=N.ptr(stats))
    N.check(N.lib().dqo_traj_repose(ctypes.byref(args), N.current_stream()))


def cameras_from_poses(poses, projection=None, rows=None, out=None):
    """Camera.updatePose for a whole pose stack in ONE launch (dqo_traj_repose over the stack itself, no trajectory involved): what
    metric.py:181, make_mesh.py:199 and metric_obj.py:212 run per dataset frame (test_frame.updatePose(pose_es[cam_id])).
    poses: [N,4,4] GPU tensor of world poses (c2w; float64 contiguous is read in place, anything else is converted on the device);
    projection: the camera's projection_matrix (float32 [4,4], transposed as the reference keeps it) — without one no projmatrix is
    formed; rows: the T stack rows to form cameras for (a sequence or an integer GPU tensor; default all N, in order); out: a dict of
    contiguous float32 GPU tensors to write into (default: new ones).  Returns dict(c2w [T,4,4], w2c [T,4,4], viewmatrix [T,4,4],
    projmatrix [T,4,4] (only with a projection), campos [T,3], stats int32 [4]): Trajectory.append's camera bits for the same pose; `w2c`
    (row-major) is directly the view dqo_eval.mesh_cull and mesh_render_depth take, `viewmatrix` its transpose (world_view_transform).
    A row outside [0, N) leaves its entry as it was (new tensors: zero) and is counted in stats[2]."""
    N.require_gpu_op(poses, projection)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] < 1:
        raise RuntimeError("cameras_from_poses: an [N,4,4] stack of at least one pose expected")
    dev, n = poses.device, int(poses.shape[0])
    p = poses.detach().to(torch.float64).contiguous()
    proj = None if projection is None else projection.detach().to(device=dev, dtype=torch.float32).reshape(4, 4).contiguous()
    with torch.cuda.device(dev):
        r = torch.arange(n, dtype=torch.int64, device=dev) if rows is None else rows
        T = int(r.numel()) if torch.is_tensor(r) else len(r)
        res = {} if out is None else dict(out)
        for name, shape in REPOSE_OUTPUTS:
            if name == "projmatrix" and proj is None:
                res.pop(name, None)
            elif name not in res:
                res[name] = torch.zeros((T,) + shape, dtype=torch.float32, device=dev)
        res["stats"] = torch.zeros((4,), dtype=torch.int32, device=dev)
        table = repose_targets(r, dev, **{name: res.get(name) for name, _ in REPOSE_OUTPUTS})
        header = torch.full((4,), n, dtype=torch.int32, device=dev)  # (only the count word is read)
        _repose(p, n, header, None, table, proj, proj is not None, None, res["stats"])
    return res


class Trajectory:
    """The trajectory on the device: what Tracker.tracking does between the tracker's answer and the mapper's input
    (SLAM/multiprocess/tracker.py:307-339), the mapper's keyframe test (SLAM/multiprocess/mapper.py:734-773) and the ATE curve
    (tracker.py:341-346), without a host read on the per-frame path:

        pose, ok, _, _ = tracker.predict_pose_async(frame)
        traj.append(pose)                                   # pose_es[-1] @ pose_t1_t0, frame.updatePose, check_keyframe: one launch
        vw, nw = traj.world_maps(frame_map["vertex_map_c"], frame_map["normal_map_c"])
        mapper.set_frame(k, settings=traj.settings(template))

    It owns `capacity` rows of world poses (float64, c2w), ground-truth poses, keyframe flags and metrics, and the current frame's camera
    tensors; the row index lives on the device and the launch advances it, so a captured append fills consecutive rows when replayed.
    Arguments in the reference's spellings: projection — the camera's projection_matrix (float32 [4,4], transposed as the reference
    keeps it; without one `projmatrix` is not formed); gaussian_update_frame — check_keyframe runs on rows i == 0 and
    (i + 1) % gaussian_update_frame == 0 (0: never); keyframe_theta_thes (degrees) / keyframe_trans_thes (metres): base.yaml's values.
    init_pose: row 0 in relative mode (identity by default, tracker.py:318).

    Two departures from the reference: `campos` is the CURRENT pose's translation (Camera.update never refreshes camera_center, so the
    reference keeps the centre of the pose the camera was constructed with); and the first relative append ignores its argument and
    stores init_pose, as the reference's first frame stores np.eye(4) without asking the tracker.  `projmatrix` is the double product of
    the double w2c (transposed) and the projection, rounded once: within half a float32 ulp of the exact product, where the reference's
    float32 bmm of the rounded world_view_transform (cameras.py:179-183) is up to 1.25 ulp from it.

    Not here: the text trajectory files (poses.txt, TUM lines), the figures, the ORB back end, and the keyframes' images
    (keyframe_list / keymap_list stay with the caller)."""

    def __init__(self, capacity, device, projection=None, gaussian_update_frame=0, keyframe_theta_thes=30.0, keyframe_trans_thes=0.3,
                 init_pose=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
        if capacity < 1:
            raise ValueError("Trajectory: capacity must be at least 1")
        self.capacity, self.device = int(capacity), device
        self.gaussian_update_frame = int(gaussian_update_frame)
        self.keyframe_theta_thes, self.keyframe_trans_thes = float(keyframe_theta_thes), float(keyframe_trans_thes)
        f64, f32 = dict(dtype=torch.float64, device=device), dict(dtype=torch.float32, device=device)
        self._pose, self._pose_gt = torch.zeros((capacity, 4, 4), **f64), torch.zeros((capacity, 4, 4), **f64)
        self.flags = torch.zeros((capacity,), dtype=torch.int32, device=device)
        self.kf_metric = torch.zeros((capacity, 2), **f64)
        header = [0] * N.CONSTANTS["DQO_TRAJ_HEADER_WORDS"]  # count, last keyframe row, overflow, unused
        header[N.CONSTANTS["DQO_TRAJ_HEADER_LAST_KEYFRAME"]] = -1
        self.header = torch.tensor(header, dtype=torch.int32, device=device)
        self.projection = None if projection is None else projection.detach().to(**f32).reshape(4, 4).contiguous()
        self.init_pose = None if init_pose is None else torch.as_tensor(init_pose).detach().to(**f64).reshape(4, 4).contiguous()
        self.c2w, self.viewmatrix, self.projmatrix = torch.eye(4, **f32), torch.eye(4, **f32), torch.zeros((4, 4), **f32)
        self.campos = torch.zeros((3,), **f32)
        self._n = 0
        self._ate_ws = None
        self._held = ()  # the last append's converted operands, alive while its launch (or a graph that captured it) may read them
        # update_poses: the device counts of the last call, the table entry of the trajectory's own camera tensors (made here: its
        # destinations never move, and a captured call must not copy from the host), that entry joined with the caller's table (cached
        # per table object), and what the last launch reads
        self.repose_stats = torch.zeros((4,), dtype=torch.int32, device=device)
        self._own_targets = repose_targets([-1], device, c2w=self.c2w, viewmatrix=self.viewmatrix, campos=self.campos,
                                           projmatrix=None if self.projection is None else self.projmatrix)
        self._joined_targets, self._held_repose = (None, None), ()

    def __len__(self):
        """The host's mirror of the row count (the device's is header[0]): every append() counts one, up to the capacity.  Replays of a
        graph that captured an append advance the device count only: tell the mirror with advance() (the captured call itself, which
        launches nothing, has counted one: the first replay's)."""
        return self._n

    def advance(self, n=1):
        self._n = min(self.capacity, self._n + int(n))

    def append(self, pose, relative=True, pose_gt=None):
        """One frame: pose — the tracker's pose_t1_t0 (float32 [4,4] GPU tensor; relative=True: pose[i] = pose[i-1] @ pose) or a world
        pose (relative=False: use_gt_pose, an ORB-refined pose); pose_gt — the frame's ground-truth pose, stored beside it.  One launch
        (dqo_traj_append), nothing read back; a float32 contiguous relative pose and float64 contiguous world poses are used where they
        are, anything else is converted on the device first.  Appending to a full store sets the overflow word and writes nothing."""
        N.require_gpu_op(pose, pose_gt)
        if pose.numel() != 16 or (pose_gt is not None and pose_gt.numel() != 16):
            raise RuntimeError("Trajectory.append: [4,4] poses expected")
        p = pose.detach().to(torch.float32 if relative else torch.float64).contiguous()
        g = None if pose_gt is None else pose_gt.detach().to(torch.float64).contiguous()
        self._held = (p, g)
        has_proj = self.projection is not None
        with torch.cuda.device(self.device):
            N.check(N.lib().dqo_traj_append(self.capacity, self._pose.data_ptr(), self._pose_gt.data_ptr(), self.flags.data_ptr(),
                                            self.kf_metric.data_ptr(), self.header.data_ptr(), p.data_ptr() if relative else None,
                                            None if relative else p.data_ptr(), N.ptr(self.init_pose), N.ptr(g), N.ptr(self.projection),
                                            self.c2w.data_ptr(), self.viewmatrix.data_ptr(), self.projmatrix.data_ptr() if has_proj else None,
                                            self.campos.data_ptr(), self.gaussian_update_frame, self.keyframe_theta_thes,
                                            self.keyframe_trans_thes, N.current_stream()))
        self.advance()
        return self

    def update_poses(self, new_poses, targets=None, bank_state=None):
        """Mapping.update_poses / Tracker.save_traj's pose_es replacement (SLAM/multiprocess/mapper.py:256-263, tracker.py:399-401) in ONE
        launch (dqo_traj_repose, csrc/map_repose.hip), nothing read back: row r of the store takes new_poses[r] for every
        r < min(len, N) as exact bytes — rows at or beyond N keep their pose, where the reference would raise IndexError — and the
        trajectory's own current-frame tensors (c2w, viewmatrix, projmatrix, campos) are formed again from row len - 1, so settings() and
        world_maps() follow.  The next tested append compares against the MOVED pose of the last keyframe, as check_keyframe reads
        keyframe_list[-1] after update_poses; pose_gt, flags, kf_metric and the header stay (the reference never re-tests a keyframe).
        new_poses: [N,4,4] GPU tensor, used in place when float64 and contiguous, otherwise converted on the device first and kept alive
        like append's operands; None: poses unchanged, only the cameras are formed again.  targets: further cameras to form in the same
        launch, an int64 [T,6] GPU table of (row, c2w, w2c, viewmatrix, projmatrix, campos) — a trajectory row and five float32
        destination addresses, 0 = skip (repose_targets() builds one; the table is read at the call: pass a NEW tensor when its
        contents change; a trajectory made without a projection forms no projmatrix, its own or a target's); bank_state: a keyframe bank's state words, whose force word the launch sets (FusedMapper.update_poses passes
        both).  Returns the device counts, int32 [4], unread: pose rows rewritten, targets written, targets skipped for their row
        (outside [0, len)), 0.  Capturable: a replay reads new_poses and the tables where they were; the own camera's row is the host
        mirror's len - 1 at the call, as for append.  The world-frame maps of stored frames are not re-transformed (nor are the
        reference's)."""
        N.require_gpu_op(self._pose, new_poses, targets, bank_state)
        p = None
        if new_poses is not None:
            if new_poses.dim() != 3 or tuple(new_poses.shape[1:]) != (4, 4):
                raise RuntimeError("Trajectory.update_poses: new_poses must be an [N,4,4] stack")
            p = new_poses.detach().to(torch.float64).contiguous()
        if targets is not None and not (targets.dtype == torch.int64 and targets.dim() == 2 and targets.shape[1] == 6 and targets.is_contiguous()):
            raise RuntimeError("Trajectory.update_poses: targets must be a contiguous int64 [T,6] table")
        own = self._own_targets
        if targets is None or targets.shape[0] == 0:
            table = own
        else:
            if self._joined_targets[0] is not targets:
                self._joined_targets = (targets, torch.cat([own, targets]))
            table = self._joined_targets[1]
        table[0, 0:1].fill_(self._n - 1)  # (a fill launch: no host copy, capturable)
        self._held_repose = (p, table)
        with torch.cuda.device(self.device):
            _repose(self._pose, self.capacity, self.header, p, table, self.projection, self.projection is not None, bank_state,
                    self.repose_stats)
        return self.repose_stats

    def poses(self):
        """[len, 4, 4] float64 view of the world poses (pose_es)."""
        return self._pose[:self._n]

    def poses_gt(self):
        return self._pose_gt[:self._n]

    def settings(self, template):
        """`template` (a GaussianRasterizationSettings) with the current frame's camera tensors: FusedMapper.set_frame(k, settings=...)
        copies them device to device."""
        if self.projection is None:
            raise RuntimeError("Trajectory.settings: the trajectory was made without a projection, so there is no projmatrix")
        return template._replace(viewmatrix=self.viewmatrix, projmatrix=self.projmatrix, campos=self.campos)

    def world_maps(self, vertex_c, normal_c, out=None):
        """(vertex_map_w, normal_map_w) of the current frame (tracker.py:332-337): see world_maps()."""
        return world_maps(vertex_c, normal_c, self.c2w, out)

    def keyframe(self):
        """The device flag word [1] int32 of the last row: bit 0 tested, bit 1 is a keyframe (check_keyframe's return value), bit 2 in
        the keyframe list.  Nothing is read."""
        if self._n < 1:
            raise RuntimeError("Trajectory.keyframe: no frame yet")
        return self.flags[self._n - 1:self._n]

    def is_keyframe(self):
        """check_keyframe's return value for the last row: the one 4-byte read, where the caller has to branch."""
        return bool(int(self.keyframe().cpu()) & N.CONSTANTS["DQO_TRAJ_KEYFRAME"])

    def ate(self, out=None):
        """The ATE curve so far, float64 [len] on the device (dqo_eval.eval_ate of the stored poses against the stored ground truth)."""
        import dqo_eval
        if self._ate_ws is None:  # sized for the capacity once: the curve grows with every frame
            self._ate_ws = torch.empty((N.lib().dqo_eval_ate_workspace_bytes(self.capacity),), dtype=torch.uint8, device=self.device)
        return dqo_eval.eval_ate(self.poses(), self.poses_gt(), out=out, workspace_buffer=self._ate_ws)

    def overflowed(self):
        """True when an append found the store full (a host read)."""
        return bool(int(self.header[N.CONSTANTS["DQO_TRAJ_HEADER_OVERFLOW"]].cpu()))

    def save(self, save_path):
        """pose_es.npy / pose_gt.npy under save_path/save_traj as Tracker.save_traj writes them (tracker.py:397, 403-409): the only host
        copy of the trajectory."""
        import os
        d = os.path.join(save_path, "save_traj")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "pose_gt.npy"), self.poses_gt().cpu().numpy())
        np.save(os.path.join(d, "pose_es.npy"), self.poses().cpu().numpy())
