"""The whole-map operators of a FusedMapper (dqo_harness/fused_mapping.py), which derives from MapOperators: everything that looks at or
rewrites the map BETWEEN mapping iterations and has no part in capturing or replaying one — map maintenance (csrc/map_lifecycle.hip),
floater pruning (csrc/map_prune.hip), keyframe evaluation with MS-SSIM, TSDF meshing, geometry evaluation (plain, densified, from a
mesh, per object), checkpoints (csrc/map_checkpoint.hip), growth sampling and the window's masks.  Most of them are one sequence: refuse
a sharded mapper, settle the camera, activate(), render the whole map on the ONE persistent context (_maintain_render) and hand the
render with its header to a package function; the two that delete rows end with _rows_freed().  GPU only."""
import numpy as np
import torch

import _dqo_native as N
import diff_gaussian_rasterization_depth as dgr
import dqo_eval
import dqo_mapgrowth as mg
import dqo_ply
import dqo_tilemask
from _dqo_context import RastContext, capacity_for, overflowed

# What MapOperators requires of the class it is mixed into (FusedMapper):
#   the map         device, P, M, the row buffers by name (xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence, alive, stable,
#                   add_tick, frame_id, the two strike counters, gaussian_object, row_flags) and _rows(*groups), which iterates them;
#                   activate() and the activations it fills (opacity, scales, rotations), _act_valid; _empty
#   the camera      settings (normalised), tile_mask (the shared all-ones one), add_depth_thres
#   spare rows      _park_position(), _free_rows(rows), _ensure_alive(), _n_spare / _n_spare_stale, reserve()
#   the two clouds  trained_rows(), stable_rows(), _require_lifecycle(who), track_lifecycle(), attach_count_reducer (a shard's mark)
#   refresh_window  _frames / _mixed, the captured graphs whose masks it writes; refresh_bank: _bank / _require_bank(who), the keyframe bank
#   load_model      _graphs(), _last_probe, begin_mapping_call(), set_training_rows(); from_model_ply also the constructor
# and what it owns: the operators' scratch, declared in _init_operator_state() and dropped per P by _drop_row_sized_operator_state().

_WHOLE_RENDER = "would need the whole map's render, a shard's shows its objects only"


def _normalised_settings(st, device):
    """The op's forward makes its settings tensors fp32 + contiguous on every call (diff_gaussian_rasterization_depth/__init__.py);
    the captured path takes raw pointers once, so it does the same once.  The reference's cameras hand over
    `world_view_transform = torch.tensor(...).transpose(0, 1).cuda()` (scene/cameras.py:137-139): a non-contiguous view whose
    data_ptr() is the UN-transposed matrix."""
    def fix(t, name, n):
        if not torch.is_tensor(t):
            raise RuntimeError(f"raster settings: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"expected scalar type Float but found {t.dtype} ({name})")
        if not t.is_cuda:
            raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
        if t.numel() != n:
            raise RuntimeError(f"raster settings: {name} must have {n} elements")
        return t.to(device).contiguous()
    return st._replace(bg=fix(st.bg, "bg", 3), viewmatrix=fix(st.viewmatrix, "viewmatrix", 16), projmatrix=fix(st.projmatrix, "projmatrix", 16),
                       campos=fix(st.campos, "campos", 3))


def _checked_tile_mask(tm, device, H, W):
    if tm.dtype != torch.int32:
        raise RuntimeError(f"expected scalar type Int but found {tm.dtype} (tile_mask)")
    if not tm.is_cuda:
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
    if tm.numel() != ((H + 15) // 16) * ((W + 15) // 16):
        raise RuntimeError("tile_mask must have ceil(H/16) x ceil(W/16) elements")
    return tm.to(device).contiguous()


class _RenderContext(RastContext):
    """A rasteriser context plus the op's nine outputs (dgr._new_outputs) of the frames rendered on it."""
    __slots__ = ("out", "outputs")

    def __init__(self, P, W, H, device):
        self.out, self.outputs = dgr._new_outputs(P, H, W, device)
        super().__init__(P, W, H, device)


class MapOperators:
    # ------------------------------------------------------------------ the operators' scratch, and what they share --------
    def _init_operator_state(self):
        """Every buffer the operators keep from call to call, declared once (the constructor calls this).  What is sized by the image or
        by a K of the caller's survives a change of P; the rest is _drop_row_sized_operator_state's."""
        self._eval_tables, self._eval_ws = {}, None  # evaluate(): its [K,8] table per K, and dqo_eval's workspace
        self._eval_ms_ws = None  # evaluate_ms_ssim(): dqo_eval.ms_ssim's workspace
        self._eval_lpips_ws = None  # evaluate_lpips(): dqo_eval.lpips' workspace
        self._mesh_w2c = None  # make_mesh(): the frame's world-to-camera matrix, row major, float32 [4,4] on the device
        self._mesh_eval_views = {}  # evaluate_mesh(), evaluate_mesh_depth(): per (K, H, W), the views' w2c [K,16], once a render was asked for
        # depth [K,H,W], and evaluate_mesh_depth's two mesh renders
        self._window_ratios, self._window_ws = {}, None  # refresh_window(): its [K] ratio table per K, dqo_window_masks' workspace
        self._sample_ctx, self.sample_header = None, None  # sample_new(): the sampler's row buffers and workspace; its last header
        self._drop_row_sized_operator_state()

    def _drop_row_sized_operator_state(self):
        """What holds for one P only, made anew by the next call of its operator (_row_count_changed calls this)."""
        self._lifecycle = {}  # maintain(): lifecycle_step's vote words and workspace ("_lifecycle")
        self._maintain_ctx = None  # maintain(): the persistent buffers of its render (_maintain_render)
        self._prune_ctx = None  # prune_floaters(): its camera tables, workspace and stats
        self._eval_object_rows = None  # evaluate_geometry_objects(): its int32 [P] group column (gaussian_object, -1 = the row is left out)
        self._checkpoint = {}  # pack_rows() / save_model(): workspace, header, table and pinned staging buffers (_checkpoint_buffers)
        self._window_flags = None  # refresh_window(): the uint8 [P] row flags of its render

    def _refuse_sharded(self, who, why=_WHOLE_RENDER):
        if self.attach_count_reducer is not None:
            raise NotImplementedError(f"FusedMapper.{who}: a sharded mapper {why} (DESIGN.md §6)")

    def _settings_or_own(self, settings):
        """The camera an operator was given, normalised, or the mapper's."""
        return self.settings if settings is None else _normalised_settings(settings, self.device)

    def _rows_freed(self):
        """The end of an operator that freed rows on the device."""
        self._n_spare_stale = True  # (_refresh_spare_count)
        self._act_valid = False  # deleted rows' raw parameters changed
        self.activate()  # (a captured iteration starts from the activations of the current parameters)

    def _own_table(self, tables, K, *columns):
        """This mapper's float32 [K, *columns] result table of one operator (`tables`: its dict by K), made on first use."""
        table = tables.get(K)
        if table is None:
            table = tables[K] = torch.empty((K,) + columns, dtype=torch.float32, device=self.device)
        return table

    # ------------------------------------------------------------------ map maintenance (csrc/map_lifecycle.hip) ----------
    # configs/base.yaml:51-52, 59-60 and the `delete_thresh = 10` of mapper.py:1092
    MAINTAIN_DEFAULTS = dict(stable_confidence_thres=500.0, unstable_time_window=200, add_color_thres=0.1, add_depth_thres=None, delete_thresh=10)

    def _maintain_render(self, st, row_flags=None, tile_mask=None):
        """The whole map (both clouds: no row flags, no object gate; spare rows are parked and transparent) rendered at camera `st` through
        the C ABI into persistent buffers: the op's nine outputs c.out (0 colour, 1 depth, 2 colour hit index, 3 depth hit index).
        row_flags (refresh_window): DqoRastInputs.row_flags, uint8 [P] — its DQO_ROW_HIDDEN rows are not rendered; None: every row.
        tile_mask (prune_floaters): int32 [gy,gx], checked by the caller; None: every tile.
        The first call measures the frame (prepare, one header read, render) and sizes the instance capacity at
        capacity_for(its candidate pairs, 1.5); later calls are ONE dqo_rast_forward call on those buffers — no header copy, no event, no allocation."""
        dev, P, M = self.device, self.P, self.M
        H, W = int(st.image_height), int(st.image_width)
        if (H, W) != (int(self.settings.image_height), int(self.settings.image_width)):
            raise RuntimeError("FusedMapper.maintain: every frame of a mapper has the mapper's image size")
        stream = N.current_stream()
        c = self._maintain_ctx
        first = c is None or (c.P, c.H, c.W) != (P, H, W)
        if first:
            c = _RenderContext(P, W, H, dev)
        params = dgr._params(st, P, M)
        inputs = dgr._inputs(st, self.xyz, self.shs, self._empty, self.opacity, self.scales, self.rotations, self._empty,
                             self.tile_mask if tile_mask is None else tile_mask, row_flags=row_flags)
        if first:
            c.size(capacity_for(int(c.measure(params, inputs, c.outputs, stream).num_candidates), 1.5))
        c.render(params, inputs, c.outputs, stream, prepare=not first)
        self._maintain_ctx = c
        return c

    def maintain_overflowed(self):
        """Whether the most recent maintain()'s render outgrew its context (one small device-to-host read: call it where a
        synchronisation is affordable, like graph_overflowed()).  If so that frame cast no votes, and the next maintain() sizes a new
        context."""
        c = self._maintain_ctx
        if c is None:
            return False
        over = overflowed(c.geom)
        if over:
            self._maintain_ctx = None
        return over

    @torch.no_grad()
    def maintain(self, tick, gt_color, gt_depth, settings=None, stable_oversized=False, **thresholds):
        """The statements that close every frame of the reference mapper (SLAM/multiprocess/mapper.py:217-219) on this mapper's map:
            gaussians_fix()            :657-676    unstable rows with confidence > stable_confidence_thres become stable
            error_gaussians_remove()   :989-1102   the whole map is rendered at the frame's camera; a stable row some pixel charges with a
                                                   depth / colour error above 2 x add_depth_thres / add_color_thres gets a strike;
                                                   delete_thresh depth strikes delete it, else delete_thresh colour strikes release it
            gaussians_delete()         :692-730    oversized or too-long-unstable rows of the unstable cloud are deleted
        and, stable_oversized (optimise frames, :214), gaussians_delete(unstable=False) in front.  tick: the mapper's `time`; gt_color
        [3,H,W], gt_depth [1,H,W]: the frame (processed_map[-1]); settings: its camera (default: the mapper's).  thresholds:
        MAINTAIN_DEFAULTS (add_depth_thres None = the mapper's).  One render (_maintain_render), dqo_mapgrowth.lifecycle_step and one
        activation pass: everything is rewritten in place — deleted rows become spare rows, P stays, captured graphs stay valid.  The
        FIRST call (and the first after P changed or after maintain_overflowed() reported an overflow) sizes the render's context from
        one 32-byte header read, as capture() does; every later call reads nothing back and does not synchronise.  A later frame that
        outgrows that context renders nothing valid: it casts no vote (statements 0, 1 and 3 still run) and maintain_overflowed() tells.
        The spare-row count is read again by the next grow().  Row flags of surviving rows are the caller's:
        set_training_rows(trainable=~fm.stable_rows()) names the next call's clouds.  Returns the int32 [8] device tensor of counts
        (dqo_mapgrowth.LIFECYCLE_STATS)."""
        self._require_lifecycle("maintain")
        self._refuse_sharded("maintain", "would need the whole map's mean radii")
        unknown = set(thresholds) - set(self.MAINTAIN_DEFAULTS)
        if unknown:
            raise TypeError(f"FusedMapper.maintain: unknown thresholds {sorted(unknown)}")
        th = dict(self.MAINTAIN_DEFAULTS, **thresholds)
        if th["add_depth_thres"] is None:
            th["add_depth_thres"] = self.add_depth_thres
        st = self._settings_or_own(settings)
        self._ensure_alive()
        with torch.cuda.device(self.device):
            self.activate()
            c = self._maintain_render(st)
            # (the buffers as they are bound NOW; only the vote words and the workspace are kept from call to call)
            state = dict({b.name: a for b, a in self._rows("param", "meta")}, **self._lifecycle)
            stats = mg.lifecycle_step(state, tick, gt_color, gt_depth, c.out[0], c.out[1], c.out[3], c.out[2],
                                      stable_oversized=stable_oversized, park=self._park_position(), render_header=c.geom, **th)
            self._lifecycle = {"_lifecycle": state["_lifecycle"]}
        self._rows_freed()
        return stats

    # ------------------------------------------------------------------ floater pruning (csrc/map_prune.hip) -------------
    @torch.no_grad()
    def prune_floaters(self, depth_map, window, *, projection, settings=None, tile_mask=None, theta_deg=3.0, centre="reference"):
        """Mapping.to_purne with create_virtual_cameras (SLAM/multiprocess/mapper.py:424-529), the reference's floater elimination, on this
        mapper's map: the keyframe's camera is turned by +-theta_deg about two axes around the point it looks at (dqo_prune_cameras), the
        whole map (both clouds, no row flags; spare rows are parked) is rendered from the four virtual cameras, and every Gaussian with
        lo < frame_id <= hi that none of the four views touched (n_touched == 0) is deleted.  depth_map: the keyframe's depth, float32 GPU
        tensor of H*W elements (frame_map["depth_map"]); window = (lo, hi): (keyframe_list[-2].uid, keyframe_list[-1].uid], or
        (uid - 1, uid] with one keyframe (:510-515); projection: the camera's float32 [4,4] GPU tensor, transposed as the reference keeps it
        (Trajectory's argument); settings: the keyframe's camera (default: the mapper's); tile_mask: int32 [gy,gx] GPU tensor, what
        evaluate_render_range(frame) returned for the frame (:470), applied to all four views as the reference does (None: all tiles).
        centre="reference": the centre depth is read at row int(cx), column int(cy) — the reference's transposed `cx, cy = int(frame.cy),
        int(frame.cx)` then `depth_map[cy, cx]` (:471-473) — and a pixel outside the image is a ValueError before any launch (the reference
        raises IndexError there); centre="principal": row int(cy), column int(cx), the intent.  The virtual views take the frame's own
        campos, as the reference's do (Camera.update never refreshes camera_center).
        One camera launch, four x (_maintain_render, dqo_prune_touch), dqo_prune_rows and one activation pass, everything in place:
        deleted rows become spare rows, P stays, captured graphs stay valid.  The FIRST call for a (P, H, W) sizes the render's context
        from one header read exactly as maintain() does (they share it); every later call reads nothing back and does not synchronise.
        A view that outgrows that context touches nothing valid: then the call deletes nothing and reports skipped = 1
        (prune_overflowed() tells, where a synchronisation is affordable).  The spare-row count is read again by the next grow().  Returns
        the int32 [8] device tensor of counts (dqo_mapgrowth.PRUNE_STATS)."""
        self._require_lifecycle("prune_floaters")
        self._refuse_sharded("prune_floaters", "would need the touch counts of the whole map's render")
        if centre not in ("reference", "principal"):
            raise ValueError("FusedMapper.prune_floaters: centre is 'reference' or 'principal'")
        dev = self.device
        st = self._settings_or_own(settings)
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if (int(st.image_height), int(st.image_width)) != (H, W):
            raise RuntimeError("FusedMapper.prune_floaters: every frame of a mapper has the mapper's image size")
        N.require_gpu_op((depth_map, projection))
        if depth_map.dtype != torch.float32 or depth_map.numel() != H * W:
            raise RuntimeError(f"FusedMapper.prune_floaters: depth_map is a float32 tensor of {H} x {W} elements, the mapper's image size")
        lo, hi = int(window[0]), int(window[1])
        if lo > hi:
            raise ValueError(f"FusedMapper.prune_floaters: bad window ({lo}, {hi}]")
        row, col = (int(st.cx), int(st.cy)) if centre == "reference" else (int(st.cy), int(st.cx))
        if not (0 <= row < H and 0 <= col < W):
            raise ValueError(f"FusedMapper.prune_floaters: the centre pixel (row {row}, column {col}) lies outside the {H} x {W} image")
        tm = None if tile_mask is None else _checked_tile_mask(tile_mask, dev, H, W)
        self._ensure_alive()
        p = self._prune_ctx
        if p is None or p["key"] != self.P:
            f32 = dict(dtype=torch.float32, device=dev)
            p = self._prune_ctx = dict(key=self.P, cameras=(torch.empty((4, 4, 4), **f32), torch.empty((4, 4, 4), **f32), torch.empty((3,), **f32)),
                                       ws=mg.prune_workspace(self.P, dev), stats=torch.zeros((8,), dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            self.activate()
            view, proj, _ = mg.prune_cameras(st.viewmatrix, projection.to(dev).contiguous(), depth_map.contiguous().reshape(H, W), row * W + col,
                                             theta_deg, out=p["cameras"])
            try:
                for k in range(4):
                    c = self._maintain_render(st._replace(viewmatrix=view[k], projmatrix=proj[k]), tile_mask=tm)
                    mg.prune_touch(c.out[7], p["ws"], render_header=c.geom)
                # (the buffers as they are bound NOW)
                stats = mg.prune_step({b.name: a for b, a in self._rows("param", "meta")}, p["ws"], (lo, hi), self._park_position(), stats=p["stats"])
            except Exception:
                self._prune_ctx = None  # (a call that failed between its touches and its row pass leaves marks in the workspace)
                raise
        self._rows_freed()
        return stats

    def prune_overflowed(self):
        """Whether the most recent prune_floaters() skipped its deletion because one of its four renders outgrew the context (one small
        device-to-host read, like maintain_overflowed()).  If so the next call sizes a new context."""
        p = self._prune_ctx
        if p is None:
            return False
        over = int(p["stats"][4].item()) != 0
        if over:
            self._maintain_ctx = None
        return over

    # ------------------------------------------------------------------ keyframe evaluation, meshing (csrc/map_eval.hip, map_tsdf.hip) --
    @torch.no_grad()
    def evaluate(self, frames, min_depth=0.3, max_depth=5.0, out=None):
        """How good the map is, over a keyframe set: eval_frame / eval_picture of the reference (SLAM/eval.py:38-188, slam.py:155,184,
        metric.py) for every frame of `frames`, a list of (settings, gt_color [3,H,W], gt_depth [1,H,W] in metres); settings None = the
        mapper's camera.  min_depth / max_depth: the valid range of the target depth (configs/base.yaml:39-40).  Per frame: the whole map
        rendered on maintain()'s persistent context (_maintain_render: no row flags, no gate — what eval_frame renders with
        `global_params`), dqo_eval.eval_picture into row k, the SSIM value into its slot 4.  Returns the float32 [K,8] device table
        (dqo_eval.ROW: psnr, color_loss, depth_loss, valid_pixel_ratio, ssim, mse r/g/b; `out` or this mapper's own table for K,
        overwritten by the next call with the same K); dqo_eval.eval_picture_dict(table[k]) reads a row.
        The FIRST call for a (P, H, W) sizes the render's context from one 32-byte header read, exactly as maintain() does; after that a
        call reads nothing back, allocates nothing and does not synchronise.  A frame that outgrows that context leaves a row of NaN; the
        caller checks maintain_overflowed() where it can afford a read (it tells about the LAST frame rendered, and makes the next call
        size a new context).  Slot 4, "ssim", is the single-scale SSIM of utils/loss_utils.py:60-100; the reference's own "ssim", MS-SSIM,
        comes from evaluate_ms_ssim (the same renders, a second table), its LPIPS from evaluate_lpips (a third, on weights the caller brings)."""
        return self._evaluate(frames, min_depth, max_depth, out, None)

    @torch.no_grad()
    def evaluate_ms_ssim(self, frames, ms_ssim, min_depth=0.3, max_depth=5.0, out=None, _lpips=None):
        """evaluate(frames, min_depth, max_depth, out) that ALSO fills `ms_ssim`, a float32 [K,20] device table (dqo_eval.MS_ROW): row k
        receives the reference's OWN "ssim", MS-SSIM (dqo_eval.ms_ssim, SLAM/eval.py:19-25, :64), of frame k's render — the render
        eval_picture used, no second one, with the same render header; nine launches more per frame.  Returns the [K,8] table, byte for
        byte evaluate()'s; dqo_eval.eval_picture_dict(table[k], ms_row=ms_ssim[k]) reports "ssim" (MS-SSIM) and "ssim_single_scale".
        Both image sides must be above 160 (pytorch_msssim's assertion): RuntimeError before anything is rendered.  The workspace is
        kept on the mapper; after the first call nothing is allocated or read."""
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if min(H, W) < dqo_eval.MS_MIN_SIDE:
            raise RuntimeError(f"FusedMapper.evaluate_ms_ssim: both image sides must be above 160, the mapper's image is {W} x {H}")
        K = len(frames)
        if (not torch.is_tensor(ms_ssim) or tuple(ms_ssim.shape) != (K, 20) or ms_ssim.dtype != torch.float32 or not ms_ssim.is_contiguous()
                or not ms_ssim.is_cuda):
            raise RuntimeError(f"FusedMapper.evaluate_ms_ssim: ms_ssim must be a contiguous float32 [{K},20] device table")
        return self._evaluate(frames, min_depth, max_depth, out, ms_ssim, _lpips)

    @torch.no_grad()
    def evaluate_lpips(self, frames, lpips, weights, ms_ssim=None, min_depth=0.3, max_depth=5.0, out=None):
        """evaluate(frames, min_depth, max_depth, out) that ALSO fills `lpips`, a float32 [K,8] device table (dqo_eval.LPIPS_ROW): row k
        receives the reference's "lpips" (dqo_eval.lpips, SLAM/eval.py:28-30, :65-68) of frame k's render — the render eval_picture used,
        no second one, with the same render header; twelve launches more per frame — on `weights`, a dqo_eval.LpipsWeights the caller made
        from ITS AlexNet and linear heads (none are shipped: the number is the reference's only on the reference's weights).  ms_ssim: a
        [K,20] table as evaluate_ms_ssim's, filled as well, or None.  Returns the [K,8] picture table, byte for byte evaluate()'s;
        dqo_eval.eval_picture_dict(table[k], ms_row=ms_ssim[k], lpips_row=lpips[k]) reports "lpips".  Both image sides must be at least
        31: RuntimeError before anything is rendered, as for a table of another shape.  The workspace is kept on the mapper; after the
        first call nothing is allocated or read."""
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if min(H, W) < dqo_eval.LPIPS_MIN_SIDE:
            raise RuntimeError(f"FusedMapper.evaluate_lpips: both image sides must be at least 31, the mapper's image is {W} x {H}")
        K = len(frames)
        if (not torch.is_tensor(lpips) or tuple(lpips.shape) != (K, 8) or lpips.dtype != torch.float32 or not lpips.is_contiguous()
                or not lpips.is_cuda):
            raise RuntimeError(f"FusedMapper.evaluate_lpips: lpips must be a contiguous float32 [{K},8] device table")
        if not isinstance(weights, dqo_eval.LpipsWeights):
            raise RuntimeError("FusedMapper.evaluate_lpips: weights must be a dqo_eval.LpipsWeights")
        if ms_ssim is not None:
            return self.evaluate_ms_ssim(frames, ms_ssim, min_depth, max_depth, out, _lpips=(lpips, weights))
        return self._evaluate(frames, min_depth, max_depth, out, None, (lpips, weights))

    def _evaluate(self, frames, min_depth, max_depth, out, ms_ssim, lpips=None):
        self._refuse_sharded("evaluate")
        dev = self.device
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if lpips is not None and self._eval_lpips_ws is None:
            self._eval_lpips_ws = dqo_eval.lpips_workspace(W, H, dev)
        if ms_ssim is not None and self._eval_ms_ws is None:
            self._eval_ms_ws = dqo_eval.ms_ssim_workspace(W, H, dev)
        if self._eval_ws is None:
            self._eval_ws = dqo_eval.workspace(W, H, dev)
        table = self._own_table(self._eval_tables, len(frames), 8) if out is None else out
        with torch.cuda.device(dev):
            self.activate()
            for k, (settings, gt_color, gt_depth) in enumerate(frames):
                c = self._maintain_render(self._settings_or_own(settings))
                o = c.out
                dqo_eval.eval_picture(dict(render=o[0], depth=o[1], depth_index_map=o[3]), gt_color, gt_depth, min_depth, max_depth, out=table,
                                      row=k, workspace_buffer=self._eval_ws, render_header=c.geom)
                if ms_ssim is not None:
                    dqo_eval.ms_ssim(o[0], gt_color, out=ms_ssim, row=k, workspace_buffer=self._eval_ms_ws, render_header=c.geom)
                if lpips is not None:
                    dqo_eval.lpips(o[0], gt_color, lpips[1], out=lpips[0], row=k, workspace_buffer=self._eval_lpips_ws, render_header=c.geom)
        return table

    @torch.no_grad()
    def make_mesh(self, frames, volume, depth_trunc=30.0):
        """The map as a triangle mesh: what make_mesh.py and eval_frame(..., volume=..., scale=...) (SLAM/eval.py:299, 316-343) do with
        an open3d TSDF volume — every frame's render of the whole map becomes an RGB-D image and is integrated — into `volume`, a
        dqo_eval.TsdfVolume the caller made over the box it wants (and clears when it wants a fresh one).  frames: a list of raster
        settings, None = the mapper's camera.  Per frame: the whole map rendered on maintain()'s persistent context (_maintain_render, as
        evaluate() does: no row flags, no gate — what eval_frame renders), then volume.integrate(depth, colour) with
        fx = W / (2 tanfovx), fy = H / (2 tanfovy), the settings' cx, cy, w2c = the transpose of the settings' viewmatrix (formed on the
        device) and render_header = the context's header: a frame that outgrew the context integrates nothing and counts in
        volume.header[5] (maintain_overflowed() tells, where a read is affordable).  depth_trunc: deeper pixels are ignored.
        The reference swaps its eval opaque threshold into the renderer for this walk (make_mesh.py:156); here the caller chooses it:
        pass settings whose opaque_threshold is the one it wants.  The FIRST call for a (P, H, W) sizes the render's context from one
        32-byte header read, exactly as maintain() does; after that a call reads nothing back, allocates nothing and does not
        synchronise.  Returns `volume`; volume.extract(cap_vertices, cap_faces) is the mesh, dqo_ply.write_mesh_ply its file;
        make_clean_mesh goes on to the cleaned, smoothed mesh with normals, make_simplified_mesh to the same with fewer triangles.
        NotImplementedError on a sharded mapper (a shard's render shows its objects only, volumes are
        not merged)."""
        self._refuse_sharded("make_mesh")
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if self._mesh_w2c is None:
            self._mesh_w2c = torch.empty((4, 4), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.activate()
            for settings in frames:
                st = self._settings_or_own(settings)
                c = self._maintain_render(st)
                self._mesh_w2c.copy_(st.viewmatrix.reshape(4, 4).t())  # (the settings keep the transposed w2c)
                K = (W / (2.0 * float(st.tanfovx)), H / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
                volume.integrate(c.out[1], c.out[0], K, self._mesh_w2c, depth_trunc=depth_trunc, render_header=c.geom)
        return volume

    @torch.no_grad()
    def make_clean_mesh(self, frames, volume, cap_vertices, cap_faces, depth_trunc=30.0, min_component_faces=0, largest_only=False,
                        smooth_iter=0, smooth_lambda=0.5, smooth_mu=None, normals=True):
        """The map as the mesh a SLAM pipeline reports: make_mesh(frames, volume, depth_trunc), volume.extract(cap_vertices, cap_faces),
        then on the device dqo_eval.mesh_components(min_faces=min_component_faces, largest_only) — the floaters that the renders of a
        Gaussian map leave in the volume go —, dqo_eval.mesh_smooth(smooth_iter, smooth_lambda, smooth_mu) on positions and colours —
        smooth_iter and smooth_lambda are the reference configs' mesh_smooth_iter and mesh_smooth_lambda
        (configs/Cube_Diorama_base.yaml:45-46: 10 and 0.5), smooth_mu makes it Taubin's — and, with `normals`, dqo_eval.mesh_normals.
        Returns the cleaned mesh dict (vertices, colors, faces, header = dqo_eval.MESHOPS_HEADER, normals), in dqo_eval's own buffers
        for the capacities, overwritten by the next call; dqo_eval.mesh_counts(mesh) reads its counts,
        dqo_ply.write_mesh_ply_normals writes it (cut at the counts).  No host read after the first call of a shape (make_mesh's one
        header read); NotImplementedError on a sharded mapper, exactly as make_mesh.  make_simplified_mesh is the same with fewer
        triangles."""
        return self._clean_mesh("make_clean_mesh", frames, volume, cap_vertices, cap_faces, depth_trunc, min_component_faces, largest_only,
                                None, None, smooth_iter, smooth_lambda, smooth_mu, normals)

    @torch.no_grad()
    def make_simplified_mesh(self, frames, volume, cap_vertices, cap_faces, simplify_voxel, simplify_origin=None, depth_trunc=30.0,
                             min_component_faces=0, largest_only=False, smooth_iter=0, smooth_lambda=0.5, smooth_mu=None, normals=True):
        """make_clean_mesh with fewer triangles: extract -> mesh_components -> dqo_eval.mesh_simplify(voxel_size=simplify_voxel,
        origin=simplify_origin, or the volume's origin) -> mesh_smooth -> mesh_normals, the other arguments make_clean_mesh's.
        Components come first, because clustering would weld a floater to a surface that passes through its cell; smoothing comes
        after, because clustering leaves the jaggedness that smoothing removes.  simplify_voxel is typically two to four times
        volume.voxel_length.  Returns the mesh dict of dqo_eval.mesh_simplify (header = dqo_eval.MESH_SIMPLIFY_HEADER) with normals, in
        dqo_eval's own buffers for the capacities — not make_clean_mesh's.  Nothing is read back; NotImplementedError on a sharded
        mapper.  A method of its own, not two more keywords of make_clean_mesh, whose parameter list is held as it is."""
        if simplify_voxel is None:
            raise ValueError("make_simplified_mesh: simplify_voxel is a cell size in metres (make_clean_mesh is the call without simplification)")
        return self._clean_mesh("make_simplified_mesh", frames, volume, cap_vertices, cap_faces, depth_trunc, min_component_faces, largest_only,
                                simplify_voxel, simplify_origin, smooth_iter, smooth_lambda, smooth_mu, normals)

    def _clean_mesh(self, who, frames, volume, cap_vertices, cap_faces, depth_trunc, min_component_faces, largest_only, simplify_voxel,
                    simplify_origin, smooth_iter, smooth_lambda, smooth_mu, normals):
        self._refuse_sharded(who)
        self.make_mesh(frames, volume, depth_trunc=depth_trunc)
        with torch.cuda.device(self.device):
            mesh = dqo_eval.mesh_components(volume.extract(cap_vertices, cap_faces), min_faces=min_component_faces, largest_only=largest_only)
            if simplify_voxel is not None:
                mesh = dqo_eval.mesh_simplify(mesh, simplify_voxel, origin=volume.origin if simplify_origin is None else simplify_origin)
            dqo_eval.mesh_smooth(mesh, smooth_iter, lam=smooth_lambda, mu=smooth_mu, scope="all")
            if normals:
                dqo_eval.mesh_normals(mesh)
            else:
                mesh.pop("normals", None)
        return mesh

    # ------------------------------------------------------------------ geometry evaluation (csrc/knn.hip, map_densify.hip) --
    @torch.no_grad()
    def densify(self, rows="stable", **kw):
        """The densified cloud the reference evaluates where a config sets pcd_densify: stable_pointcloud.densify(1, 30, 5)
        (slam.py:202-206, SLAM/gaussian_pointcloud.py:67-130) and eval_pcd's subsample of it (SLAM/eval.py:244), from this mapper's raw
        parameters through dqo_eval.densify, whose keywords (sigma, circle_num, levels, theta, sample_nums, seed, frame, want_normals,
        want_index, workspace_buffer) pass through and whose dict comes back.  rows "stable": the rows of the reference's
        stable_pointcloud, alive & stable (needs track_lifecycle()); "all": every Gaussian of the map (`alive`, or every row of a mapper
        without spare rows).  Nothing is read back."""
        if "keep" in kw:
            raise RuntimeError("FusedMapper.densify: the row mask is chosen with rows=, not keep=")
        if rows == "stable":
            keep = self.stable_rows().to(torch.uint8)
        elif rows == "all":
            keep = self.alive
        else:
            raise RuntimeError(f"FusedMapper.densify: rows must be 'stable' or 'all', got {rows!r}")
        return dqo_eval.densify(self.xyz.detach(), self.scaling_raw.detach(), self.rotation_raw.detach(), keep=keep, **kw)

    def _densified_cloud(self, who, kw):
        """(points, keep) of densify(**kw) as the geometry evaluators take it: `sample_nums` defaults to eval_frame's 1 000 000 and is
        checked against dqo_nn1's limit, no normals unless asked for."""
        kw = dict(kw or {})
        kw.setdefault("sample_nums", 1000000)
        if kw["sample_nums"] is None or not 1 <= int(kw["sample_nums"]) < (1 << 25):
            raise RuntimeError(f"FusedMapper.{who}: densify's sample_nums must be in [1, 2^25 - 1], got {kw['sample_nums']}")
        kw.setdefault("want_normals", False)
        d = self.densify(**kw)
        return d["points"], d["keep"]

    @torch.no_grad()
    def evaluate_geometry(self, gt_points, dist_thres=(0.03,), transform=None, out=None, row=0):
        """How good the map's GEOMETRY is against a ground-truth point set: eval_pcd of the reference (SLAM/eval.py:190-282) — accuracy,
        completion, chamfer distance, precision / recall / F1 per threshold — through dqo_eval.eval_pcd.  The reconstruction is this
        mapper's own `xyz` buffer with `alive` as the row mask: the points the reference reads back from the PLY it saved, without the
        file, a copy or a host read.  gt_points [G,3]: the ground-truth points (from a mesh: evaluate_geometry_mesh);
        transform: [3,4] / [4,4] applied to the map's points (:241).  Returns the float32 [32] device row (dqo_eval.PCD_ROW; out[row] of
        a caller-owned [K,32] table if given); dqo_eval.eval_pcd_dict reads it.  The workspace is dqo_eval's, per device and sizes.
        The configs with pcd_densify evaluate another point set: evaluate_geometry_densified."""
        return dqo_eval.eval_pcd(gt_points, self.xyz.detach(), dist_thres, transform, rec_keep=self.alive, out=out, row=row)

    @torch.no_grad()
    def evaluate_geometry_densified(self, gt_points, dist_thres=(0.03,), transform=None, out=None, row=0, densify=None):
        """evaluate_geometry on the point set the reference evaluates for the configs with pcd_densify (replica, aithor, real,
        Cube_Diorama; metric.py:156-157): the densified cloud of densify()'s rows, subsampled as eval_pcd does (SLAM/eval.py:244).
        densify: a dict of densify()'s keywords, `rows` included (None or {}: the reference's call, densify(1, 30, 5) of the stable
        cloud); its `sample_nums` defaults to 1 000 000 as eval_frame's and may be at most 2^25 - 1, dqo_nn1's limit.  densify()'s
        `keep` goes in as eval_pcd's row mask, so no count is read back.  Everything else as evaluate_geometry."""
        rec, rec_keep = self._densified_cloud("evaluate_geometry_densified", densify)
        return dqo_eval.eval_pcd(gt_points, rec, dist_thres, transform, rec_keep=rec_keep, out=out, row=row)

    @torch.no_grad()
    def evaluate_geometry_mesh(self, vertices, faces, sample_nums=1000000, seed=0, dist_thres=(0.03,), transform=None, out=None, row=0,
                               densify=None):
        """eval_pcd of the reference from the ground-truth MESH (SLAM/eval.py:228-282; metric.py, metric_obj.py): sample_nums points are
        drawn on its surface (dqo_eval.sample_surface: trimesh.sample.sample_surface, :247) and the map is evaluated against them.
        vertices [V,3] float32, faces [F,3] int32: device tensors (dqo_ply.read_mesh_ply reads gt_mesh.ply on the host); sample_nums in
        [1, 2^25 - 1]; seed: the draw's.  densify None: the reconstruction is the live rows, as evaluate_geometry's; True, or a dict of
        densify()'s keywords: the densified cloud, as evaluate_geometry_densified's (True: the reference's densify(1, 30, 5) of the
        stable cloud).  The sampled points and their `keep` go in as gt_points / gt_keep: one chain on the current stream from the mesh
        tensors to the [32] row, no host read.  A mesh without area gives a row of NaN.  Everything else as evaluate_geometry."""
        return self._evaluate_geometry_mesh("evaluate_geometry_mesh", False, vertices, faces, sample_nums, seed, dist_thres, transform, out, row,
                                            densify)

    @torch.no_grad()
    def evaluate_geometry_mesh_surface(self, vertices, faces, sample_nums=1000000, seed=0, dist_thres=(0.03,), transform=None, out=None, row=0,
                                       densify=None):
        """evaluate_geometry_mesh with the map's points measured to the ground-truth SURFACE (dqo_eval.eval_pcd_surface with gt_mesh):
        accuracy and precision are the exact point-to-triangle distances from every point of the reconstruction to the mesh
        (dqo_eval.nearest_on_mesh), free of the sampling's noise floor and of `seed`.  The map is a point cloud and has no surface, so
        completion and recall stay evaluate_geometry_mesh's: the sampled ground-truth points to their nearest map point.  Every
        argument and the returned float32 [32] device row are evaluate_geometry_mesh's, whose signature is pinned, so the rule is this
        method.  The face count lies in [1, 2^25 - 1]."""
        return self._evaluate_geometry_mesh("evaluate_geometry_mesh_surface", True, vertices, faces, sample_nums, seed, dist_thres, transform, out,
                                            row, densify)

    def _evaluate_geometry_mesh(self, who, surface, vertices, faces, sample_nums, seed, dist_thres, transform, out, row, densify):
        """evaluate_geometry_mesh's and evaluate_geometry_mesh_surface's body."""
        gt = dqo_eval.sample_surface(vertices, faces, sample_nums, seed=seed)
        if densify is None or densify is False:
            rec, rec_keep = self.xyz.detach(), self.alive
        else:
            rec, rec_keep = self._densified_cloud(who, None if densify is True else densify)
        if surface:
            return dqo_eval.eval_pcd_surface(gt["points"], rec, dict(vertices=vertices, faces=faces), None, dist_thres, transform,
                                             gt_keep=gt["keep"], rec_keep=rec_keep, out=out, row=row)
        return dqo_eval.eval_pcd(gt["points"], rec, dist_thres, transform, gt_keep=gt["keep"], rec_keep=rec_keep, out=out, row=row)

    @torch.no_grad()
    def evaluate_mesh(self, mesh, gt_vertices, gt_faces, frames=None, depths=None, sample_nums=1000000, seed=0, dist_thres=(0.03,),
                      transform=None, eps=0.03, min_corners=3, depth_trunc=float("inf"), out=None, row=0):
        """How good the MESH this mapper produced is against the ground-truth mesh, in one call: dqo_eval.eval_mesh — both meshes
        culled to what the frames' cameras saw (dqo_eval.mesh_cull), both sampled by their device counts
        (dqo_eval.sample_surface_counted: gt with `seed`, the reconstruction with seed + 1), the point sets compared (eval_pcd).
        mesh: a mesh dict — make_mesh's volume.extract(...), make_clean_mesh's or make_simplified_mesh's; gt_vertices [V,3] float32,
        gt_faces [F,3] int32: device tensors (dqo_ply.read_mesh_ply reads gt_mesh.ply on the host).
        frames: make_mesh's list of raster settings (None in the list = the mapper's camera), or None = no culling.  From the frames
        the method forms, on the device, w2c [K,16] — each settings' viewmatrix transposed, as make_mesh does — and takes
        fx = W / (2 tanfovx), fy = H / (2 tanfovy), cx, cy; the frames must share one image size and one set of intrinsics: ValueError
        otherwise, before anything is launched.
        depths: None — frustum test only; "render" — the whole map rendered per frame on maintain()'s context (_maintain_render, as
        make_mesh does) and its depth copied into a [K,H,W] buffer this mapper keeps: the cull's occlusion test runs against the very
        pixels that made the mesh (NotImplementedError on a sharded mapper, whose render shows its objects only); a float32 [K,H,W]
        device tensor — the caller's own depth, for example the sensor's, or the ground-truth mesh's own render
        (dqo_eval.mesh_render_depth(gt, ...)["depth"]) where no sensor depth exists.  eps, min_corners, depth_trunc: mesh_cull's.
        sample_nums, seed, dist_thres, transform, out, row: eval_mesh's.  Returns the float32 [32] device row (dqo_eval.PCD_ROW;
        dqo_eval.eval_pcd_dict reads it).  Nothing is read back after the first render of a shape (make_mesh's one header read)."""
        return self._evaluate_mesh("evaluate_mesh", mesh, gt_vertices, gt_faces, frames, depths, sample_nums, seed, dist_thres, transform,
                                   dict(eps=eps, depth_trunc=depth_trunc, min_corners=min_corners), out, row)

    @torch.no_grad()
    def evaluate_mesh_visible(self, mesh, gt_vertices, gt_faces, frames, depths=None, sample_nums=1000000, seed=0, dist_thres=(0.03,),
                              transform=None, eps=0.03, min_pixels=1, depth_trunc=float("inf"), out=None, row=0):
        """evaluate_mesh with visibility decided per FACE (dqo_eval.eval_mesh's views["visibility"] = "faces", dqo_eval.mesh_cull_visible):
        each mesh is rendered from the frames' cameras with the near plane clipped and keeps the faces that win at least min_pixels
        pixels, so a wall of two triangles that fills every frame stays in the ground truth although no corner of it lies inside an
        image — evaluate_mesh's per-vertex rule drops it, and reports completion and recall against a ground truth without walls.
        frames, depths (None, "render" or a [K,H,W] tensor: the occlusion test per pixel), eps, depth_trunc and every other argument:
        evaluate_mesh's, whose signature is pinned, so the rule is this method.  Returns the float32 [32] device row."""
        if frames is None:
            raise ValueError("FusedMapper.evaluate_mesh_visible: frames is a list of raster settings: visibility needs cameras")
        return self._evaluate_mesh("evaluate_mesh_visible", mesh, gt_vertices, gt_faces, frames, depths, sample_nums, seed, dist_thres, transform,
                                   dict(eps=eps, depth_trunc=depth_trunc, min_pixels=min_pixels, visibility="faces"), out, row)

    @torch.no_grad()
    def evaluate_mesh_surface(self, mesh, gt_vertices, gt_faces, frames=None, depths=None, sample_nums=1000000, seed=0, dist_thres=(0.03,),
                              transform=None, eps=0.03, min_corners=3, depth_trunc=float("inf"), out=None, row=0, visibility="vertices",
                              min_pixels=1):
        """evaluate_mesh / evaluate_mesh_visible with the distances taken to the SURFACE (dqo_eval.eval_mesh_surface): the same culling,
        the same samples, but a sample is measured to the nearest FACE of the other culled mesh — the exact point-to-triangle distance of
        dqo_eval.nearest_on_mesh — instead of the nearest sample of it, which adds about 0.5 / sqrt(samples per square metre) to accuracy
        and completion.  visibility: "vertices" — evaluate_mesh's rule with min_corners (frames may be None: no culling) — or "faces" —
        evaluate_mesh_visible's with min_pixels (frames required).  Every other argument and the returned float32 [32] device row are
        evaluate_mesh's; that method's and evaluate_mesh_visible's signatures are pinned, so the rule is this method."""
        if visibility not in ("vertices", "faces"):
            raise ValueError(f"FusedMapper.evaluate_mesh_surface: visibility is 'vertices' or 'faces', got {visibility!r}")
        if visibility == "faces" and frames is None:
            raise ValueError("FusedMapper.evaluate_mesh_surface: frames is a list of raster settings: visibility='faces' needs cameras")
        rule = dict(eps=eps, depth_trunc=depth_trunc, min_corners=min_corners) if visibility == "vertices" else \
            dict(eps=eps, depth_trunc=depth_trunc, min_pixels=min_pixels, visibility="faces")
        return self._evaluate_mesh("evaluate_mesh_surface", mesh, gt_vertices, gt_faces, frames, depths, sample_nums, seed, dist_thres, transform,
                                   rule, out, row, chain=dqo_eval.eval_mesh_surface)

    def _evaluate_mesh(self, who, mesh, gt_vertices, gt_faces, frames, depths, sample_nums, seed, dist_thres, transform, rule, out, row,
                       chain=dqo_eval.eval_mesh):
        """evaluate_mesh's, evaluate_mesh_visible's and evaluate_mesh_surface's body; rule: the cull's keywords of dqo_eval.eval_mesh's
        views; chain: dqo_eval.eval_mesh or eval_mesh_surface."""
        gt = dict(vertices=gt_vertices, faces=gt_faces)
        if frames is None:
            if depths is not None:
                raise ValueError(f"FusedMapper.{who}: depths belong to frames; frames=None is the evaluation without culling")
            return chain(mesh, gt, sample_nums, seed, dist_thres=dist_thres, transform=transform, out=out, row=row)
        render = isinstance(depths, str)
        if render and depths != "render":
            raise ValueError(f"FusedMapper.{who}: depths is None, 'render' or a [K,H,W] device tensor, got {depths!r}")
        if render:
            self._refuse_sharded(who)
        with torch.cuda.device(self.device):
            bufs, K, W, H = self._frame_views(who, frames, render)
            views = dict(w2c=bufs["w2c"], K=K, W=W, H=H, depth=bufs["depth"] if render else depths, **rule)
            return chain(mesh, gt, sample_nums, seed, dist_thres=dist_thres, transform=transform, views=views, out=out, row=row)

    def _frame_views(self, who, frames, render):
        """What evaluate_mesh and evaluate_mesh_depth form from a list of raster settings (None in the list = the mapper's camera), on
        the device: (bufs, K, W, H) — bufs: this mapper's buffers for (len(frames), H, W), with "w2c" float32 [K,16], each settings'
        viewmatrix transposed as make_mesh does, and, with `render`, "depth" float32 [K,H,W]: the whole map rendered per frame on
        maintain()'s context (_maintain_render); K = (fx, fy, cx, cy) with fx = W / (2 tanfovx), fy = H / (2 tanfovy).  The frames must
        share one image size and one set of intrinsics: ValueError otherwise, before anything is made or launched."""
        raw = [self.settings if st is None else st for st in frames]
        if not raw:
            raise ValueError(f"FusedMapper.{who}: frames is empty" + (" (None is the evaluation without culling)" if who == "evaluate_mesh" else ""))
        camera = lambda st: (int(st.image_width), int(st.image_height), float(st.tanfovx), float(st.tanfovy), float(st.cx), float(st.cy))
        W, H, tfx, tfy, cx, cy = camera(raw[0])
        for k, st in enumerate(raw):
            if camera(st) != (W, H, tfx, tfy, cx, cy):
                raise ValueError(f"FusedMapper.{who}: frame {k} has another image size or other intrinsics than frame 0 "
                                 f"({camera(st)} against {(W, H, tfx, tfy, cx, cy)}): the views share one camera")
        K = len(raw)
        bufs = self._mesh_eval_views.setdefault((K, H, W), {})
        if "w2c" not in bufs:
            bufs["w2c"] = torch.empty((K, 16), dtype=torch.float32, device=self.device)
        if render and "depth" not in bufs:
            bufs["depth"] = torch.empty((K, H, W), dtype=torch.float32, device=self.device)
        if render:
            self.activate()
        for k, st in enumerate(raw):
            st = _normalised_settings(st, self.device)
            bufs["w2c"][k].view(4, 4).copy_(st.viewmatrix.reshape(4, 4).t())  # (the settings keep the transposed w2c)
            if render:
                bufs["depth"][k].copy_(self._maintain_render(st).out[1].reshape(H, W))
        return bufs, (W / (2.0 * tfx), H / (2.0 * tfy), cx, cy), W, H

    @torch.no_grad()
    def evaluate_mesh_depth(self, mesh, gt_vertices, gt_faces, frames, depth_trunc=float("inf"), out=None):
        """Depth L1 of this mapper's reconstruction against the ground-truth mesh at the frames' cameras — the number the dense-SLAM
        evaluation protocols report beside evaluate_mesh's: the ground-truth mesh rendered to depth per frame
        (dqo_eval.mesh_render_depth) and compared pixel by pixel (dqo_eval.depth_l1, the ground truth as the truth) with
        mesh given — that mesh (make_mesh's, make_clean_mesh's, ...) rendered the same way;
        mesh=None  — the map's own render per frame (_maintain_render, as evaluate_mesh's depths="render"): NotImplementedError on a
                     sharded mapper, whose render shows its objects only.
        gt_vertices, gt_faces: as evaluate_mesh's.  frames: evaluate_mesh's list of raster settings; w2c and the intrinsics are formed
        from them exactly as there (one image size, one set of intrinsics: ValueError otherwise).  depth_trunc: deeper ground truth is
        not rendered and not compared.  The depth stacks live in buffers this mapper keeps per (K, H, W).  Returns depth_l1's float32
        [K + 1, 8] device table (dqo_eval.DEPTH_L1_ROW; `out` if given); dqo_eval.depth_l1_dict reads it.  Nothing is read back after
        the first render of a shape (make_mesh's one header read)."""
        return self._evaluate_mesh_depth("evaluate_mesh_depth", dqo_eval.mesh_render_depth, mesh, gt_vertices, gt_faces, frames, depth_trunc, out)

    @torch.no_grad()
    def evaluate_mesh_depth_clipped(self, mesh, gt_vertices, gt_faces, frames, depth_trunc=float("inf"), out=None):
        """evaluate_mesh_depth with the near plane clipped (dqo_eval.mesh_render_depth_clip; dqo_eval.eval_mesh_depth's views["clip_near"]):
        a face that crosses a frame's near plane — the floor or a wall of the room the camera stands in — is rendered, where
        evaluate_mesh_depth drops it and the table shows its hole as only_b, neither and l1_image.  Arguments and the returned table:
        evaluate_mesh_depth's, whose signature is pinned, so the rule is this method."""
        return self._evaluate_mesh_depth("evaluate_mesh_depth_clipped", dqo_eval.mesh_render_depth_clip, mesh, gt_vertices, gt_faces, frames,
                                         depth_trunc, out)

    def _evaluate_mesh_depth(self, who, render_mesh, mesh, gt_vertices, gt_faces, frames, depth_trunc, out):
        """evaluate_mesh_depth's and evaluate_mesh_depth_clipped's body; render_mesh: dqo_eval's mesh render of the two."""
        render = mesh is None
        if render:
            self._refuse_sharded(who)
        if frames is None:
            raise ValueError(f"FusedMapper.{who}: frames is a list of raster settings: a depth needs cameras")
        gt = dict(vertices=gt_vertices, faces=gt_faces)
        with torch.cuda.device(self.device):
            bufs, K, W, H = self._frame_views(who, frames, render)
            kw = dict(depth_trunc=depth_trunc)
            truth = render_mesh(gt, bufs["w2c"], K, W, H, out=bufs.setdefault("render_gt", {}), **kw)["depth"]
            rec = bufs["depth"] if render else render_mesh(mesh, bufs["w2c"], K, W, H, out=bufs.setdefault("render_rec", {}), **kw)["depth"]
            return dqo_eval.depth_l1(truth, rec, depth_trunc=depth_trunc, out=out)

    def _object_rows(self, rows, who):
        """int32 [P], a buffer of this mapper's own: gaussian_object where the row is alive and in `rows`, -1 elsewhere — the group
        column of the per-object evaluation.  Nothing is gathered: the map's buffers go in as stored."""
        self._refuse_sharded(who, "holds its own objects only; merging shards is not built")
        if self.gaussian_object is None:
            raise RuntimeError(f"FusedMapper.{who}: this mapper has no object ids; call set_object_gate() first")
        if isinstance(rows, str):
            if rows == "stable":
                self._require_lifecycle(who)
                take = self.stable_rows()
            elif rows == "all":
                take = None if self.alive is None else self.alive != 0
            else:
                raise RuntimeError(f"FusedMapper.{who}: rows must be 'stable', 'all' or a mask of {self.P} rows, got {rows!r}")
        else:
            if not torch.is_tensor(rows) or rows.numel() != self.P or rows.dtype not in (torch.bool, torch.uint8) or rows.device != self.xyz.device:
                raise RuntimeError(f"FusedMapper.{who}: rows must be 'stable', 'all' or a uint8 / bool device mask of {self.P} rows")
            take = rows.reshape(-1) != 0
            if self.alive is not None:
                take = take & (self.alive != 0)
        col = self._eval_object_rows
        if col is None:
            col = self._eval_object_rows = torch.empty((self.P,), dtype=torch.int32, device=self.device)
        col.copy_(self.gaussian_object)
        if take is not None:
            col.masked_fill_(~take, -1)
        return col

    @torch.no_grad()
    def evaluate_geometry_objects(self, gt_points, gt_object, dist_thres=(0.01,), transform=None, rows="stable", out=None, row=0):
        """The map's geometry PER OBJECT: what metric_obj.py:169-236 reports from the `*_stable_obj{id}.ply` files, without the files —
        dqo_eval.eval_pcd_objects of this mapper's own `xyz` with its `gaussian_object` column against gt_points [G,3] / gt_object [G]
        (from meshes: evaluate_geometry_objects_mesh).  rows "stable": the alive rows of the stable cloud (what metric_obj.py loads;
        needs track_lifecycle()); "all": every alive row; or a uint8 / bool [P] mask (alive rows of it).  The restriction is written as -1
        into a group column this mapper keeps: no row is gathered, nothing is read back.  Returns the float32 [64,32] device table (rows
        [row, row + 64) of `out` if given); dqo_eval.eval_pcd_objects_dict reads it.  RuntimeError without an object gate
        (set_object_gate), and without track_lifecycle() for rows="stable"; NotImplementedError on a sharded mapper."""
        col = self._object_rows(rows, "evaluate_geometry_objects")
        return dqo_eval.eval_pcd_objects(gt_points, gt_object, self.xyz.detach(), col, dist_thres, transform, out=out, row=row)

    @torch.no_grad()
    def evaluate_geometry_objects_mesh(self, meshes, sample_nums=1000000, seed=0, dist_thres=(0.01,), transform=None, rows="stable", out=None,
                                       row=0):
        """evaluate_geometry_objects from the objects' ground-truth MESHES, meshes = {object id: (vertices [V,3] float32, faces [F,3]
        int32)} as device tensors: sample_nums points are drawn on every mesh (dqo_eval.sample_surface_objects, metric_obj.py's
        sample_nums=1000000 per object) and the map is evaluated against them — one chain on the current stream from the mesh tensors
        to the [64,32] table, no host read."""
        col = self._object_rows(rows, "evaluate_geometry_objects_mesh")  # (the checks first: no sample is drawn for a refused call)
        gt, gt_object = dqo_eval.sample_surface_objects(meshes, sample_nums, seed=seed)
        return dqo_eval.eval_pcd_objects(gt, gt_object, self.xyz.detach(), col, dist_thres, transform, out=out, row=row)

    # ------------------------------------------------------------------ checkpoints (csrc/map_checkpoint.hip) -----------
    def _checkpoint_buffers(self, table=True, host=False, objects=False):
        """self._checkpoint for this P, with what the caller needs made on first use, in this order: the pack's workspace "ws" and its
        int32 [2] "header" (always); `table`: the device table "buf"; `host`: the pinned staging buffer "host" and "host_header";
        `objects`: save_model_objects' "obj_header" and its pinned copy.  One table size serves both column sets: the wider one's."""
        P, dev, n = self.P, self.device, self.P * (6 + 3 * self.M + 9)
        k = self._checkpoint
        if k.get("P") != P:
            k = self._checkpoint = dict(P=P, ws=dqo_ply.pack_workspace(P, dev), header=torch.empty((2,), dtype=torch.int32, device=dev))
        if table and "buf" not in k:
            k["buf"] = torch.empty((n,), dtype=torch.float32, device=dev)
        if host and "host" not in k:
            k["host"] = torch.empty((n,), dtype=torch.float32, pin_memory=True)
            k["host_header"] = torch.empty((2,), dtype=torch.int32, pin_memory=True)
        if objects and "obj_header" not in k:
            k["obj_header"] = torch.empty((2, 64), dtype=torch.int32, device=dev)
            k["host_obj_header"] = torch.empty((2, 64), dtype=torch.int32, pin_memory=True)
        return k

    @torch.no_grad()
    def pack_rows(self, include_confidence=True, out=None):
        """(table, header), both on the device: the map's live rows as the vertex table of the reference's PLY files
        (dqo_ply.pack_rows, dqo_map_pack_rows) — the unstable cloud's rows in row order, then the stable cloud's; header int32 [2] =
        {U, S}.  The first U rows are path.ply's vertex data, the last S path_stable.ply's, all of them path_merge.ply's.  A mapper
        without track_lifecycle() is all unstable, one without spare rows all alive.  table: `out` (float32 [>= P, C]) or this mapper's
        own buffer, overwritten by the next call; rows at and behind U + S keep their bytes.  Two launches on the current stream, no
        allocation after the first call, no synchronisation."""
        P, C = self.P, 6 + 3 * self.M + 8 + (1 if include_confidence else 0)
        k = self._checkpoint_buffers(table=out is None)
        if out is None:
            out = k["buf"][:P * C].view(P, C)
        return dqo_ply.pack_rows(self.xyz, self.shs, self.opacity_raw, self.scaling_raw, self.rotation_raw, self.confidence, self.alive,
                                 self.stable, include_confidence, out=out, header=k["header"], workspace_buffer=k["ws"])

    @torch.no_grad()
    def save_model(self, path, save_data=True, save_sibr=True, save_merge=True):
        """gaussian_map.save_model (SLAM/multiprocess/mapper.py:1580-1608; slam.py:164, 194) of this mapper's map; `path` is the prefix.
            save_data   path.ply, path_stable.ply            with the confidence column
            save_sibr   path_sibr.ply, path_stable_sibr.ply  without it
            save_merge  path_merge.ply / path_merge_sibr.ply, the unstable rows then the stable rows — only when both clouds have rows
        A file of an empty cloud is not written (gaussian_pointcloud.py:642-643).  Per column set: ONE pack_rows, ONE device-to-host copy
        into a pinned staging buffer this mapper keeps, and every file is written from a slice of that buffer (the merged file is the
        table itself: nothing is re-read).  It runs on the current stream, behind whatever replays are enqueued, and synchronises once
        per column set; the first set's copy takes all P rows (the counts are not known yet), the second the U + S live rows.
        Returns {file: rows} of the files written.  The per-object files of save_model_ply_obj (SAVE_obj_ply, mapper.py:1586-1588) are
        save_model_objects(); a sharded mapper saves its shard."""
        P, M = self.P, self.M
        written, counts = {}, None
        for with_conf, tag in ((True, ""), (False, "_sibr")):
            if not (save_data if with_conf else save_sibr):
                continue
            C = 6 + 3 * M + 8 + (1 if with_conf else 0)
            table, header = self.pack_rows(include_confidence=with_conf)
            k = self._checkpoint_buffers(host=True)
            n = P if counts is None else counts[0] + counts[1]
            k["host"][:n * C].copy_(table.view(-1)[:n * C], non_blocking=True)
            k["host_header"].copy_(header, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            counts = (int(k["host_header"][0]), int(k["host_header"][1]))
            U, S = counts
            rows = k["host"][:(U + S) * C].view(U + S, C)
            files = [(path + tag + ".ply", rows[:U]), (path + "_stable" + tag + ".ply", rows[U:])]
            if save_merge and U > 0 and S > 0:
                files.append((path + "_merge" + tag + ".ply", rows))
            for name, part in files:
                if dqo_ply.write_vertex_table(name, part, 3 * (M - 1), with_conf) > 0:
                    written[name] = int(part.shape[0])
        return written

    @torch.no_grad()
    def save_model_objects(self, path):
        """The per-object files gaussian_map.save_model writes with SAVE_obj_ply (mapper.py:1586-1588: save_model_ply_obj,
        SLAM/gaussian_pointcloud.py:589-637, of both clouds) — path_obj{id}.ply for the unstable cloud, path_stable_obj{id}.ply for the
        stable one (what metric_obj.py loads), WITHOUT the confidence column, one file per object a cloud has rows of (ids in [0, 64),
        set_object_gate's; a row with another id is in no file).  ONE pack (dqo_ply.pack_rows_by_object), one device-to-host copy into
        save_model's pinned staging buffer, every file a slice of it; one synchronisation.  Returns {file: rows} of the files written.
        A method of its own so that save_model's files, signature and return value stay what they are; a sharded mapper saves its shard."""
        if self.gaussian_object is None:
            raise RuntimeError("FusedMapper.save_model_objects: the files need the Gaussians' object ids; call set_object_gate() first")
        P, M = self.P, self.M
        C = 6 + 3 * M + 8
        k = self._checkpoint_buffers(host=True, objects=True)
        table, header = dqo_ply.pack_rows_by_object(self.xyz, self.shs, self.opacity_raw, self.scaling_raw, self.rotation_raw,
                                                    self.gaussian_object, None, self.alive, self.stable, False,
                                                    out=k["buf"][:P * C].view(P, C), header=k["obj_header"], workspace_buffer=k["ws"])
        k["host"][:P * C].copy_(table.view(-1), non_blocking=True)  # (all P rows: the counts are not known yet)
        k["host_obj_header"].copy_(header, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        written = {}
        for name, first, rows in dqo_ply.object_file_slices(path, k["host_obj_header"].numpy()):
            part = k["host"][first * C:(first + rows) * C].view(rows, C)
            if dqo_ply.write_vertex_table(name, part, 3 * (M - 1), False) > 0:
                written[name] = rows
        return written

    @staticmethod
    def _read_checkpoint(path, stable_path):
        """[(table of `path` or None, has_confidence), (table of `stable_path` or None, ...)], and the SH size the files agree on."""
        tables, M = [], None
        for p in (path, stable_path):
            if p is None:
                tables.append(None)
                continue
            props, table = dqo_ply.read_vertex_table(p)
            n_rest = sum(1 for q in props if q.startswith("f_rest_"))
            conf = "confidence" in props
            if n_rest % 3 != 0 or list(props) != dqo_ply.attribute_names(n_rest, conf):
                raise RuntimeError(f"{p}: not a map file: its properties are not those of save_model_ply")
            if M is not None and M != n_rest // 3 + 1:
                raise RuntimeError(f"{p}: {n_rest} f_rest columns, {path} has {3 * (M - 1)}")
            M = n_rest // 3 + 1
            tables.append(np.ascontiguousarray(table, np.float32))
        if M is None:
            raise RuntimeError("FusedMapper.load_model: neither file was given")
        return tables, M

    @torch.no_grad()
    def load_model(self, path, stable_path=None, tick=0):
        """gaussian_map.pointcloud.load / stable_pointcloud.load (SLAM/gaussian_pointcloud.py:132-207; metric.py, metric_obj.py,
        make_mesh.py) into THIS mapper, in place: the rows of `path` become the unstable cloud in rows [0, U), the rows of `stable_path`
        the stable cloud in rows [U, U + S) (either may be None: an empty cloud has no file).  Values are the files' raw parameters, bit
        for bit (the constructor's clamp and log are not applied); confidence is the file's column, or zeros without one.  add_tick =
        frame_id = tick (the files do not hold the column), both strike counters and every Adam moment zero; every other row becomes a spare row exactly as _free_rows leaves one.
        P never changes: more rows than P is a RuntimeError that names the reserve() needed.  A stable file on a mapper that does not
        track lifecycles starts tracking.  One host-to-device copy and one launch (dqo_map_unpack_rows) per file.  Row flags: every live
        row is trained and rendered (set_training_rows() names the next call's clouds).  Ends with
        begin_mapping_call(reset_optimizer=True); the captured graphs are marked stale — their capacities were sized on another map."""
        tables, M = self._read_checkpoint(path, stable_path)
        self._load_tables(tables, M, tick)
        return self

    def _load_tables(self, tables, M, tick):
        dev, P = self.device, self.P
        if M != self.M:
            raise RuntimeError(f"FusedMapper.load_model: the files hold {M} SH coefficients per Gaussian, this mapper {self.M}")
        if self.gaussian_object is not None:
            raise RuntimeError("FusedMapper.load_model: the files carry no object ids; switch the gate off (set_object_gate(None, None)) first")
        U, S = (0 if t is None else int(t.shape[0]) for t in tables)
        n = U + S
        if n > P:
            raise RuntimeError(f"FusedMapper.load_model: the files hold {n} rows, this mapper has {P}: reserve({n - P}) more rows first")
        if self.stable is None and S > 0:
            self.track_lifecycle()
        if n < P:
            self._ensure_alive()
        first = 0
        for t in tables:
            if t is not None and t.shape[0] > 0:
                dqo_ply.unpack_rows(torch.from_numpy(t).to(dev), first, self.xyz, self.shs, self.opacity_raw, self.scaling_raw,
                                    self.rotation_raw, self.confidence)
                first += int(t.shape[0])
        if self.alive is not None:
            self.alive[:n] = 1
        if self.stable is not None:
            self.stable[:U] = 0
            self.stable[U:n] = 1
            self.add_tick[:n] = int(tick)
            self.frame_id[:n] = int(tick)
            self.depth_error_counter.zero_(), self.color_error_counter.zero_()
        if n < P:
            self._free_rows(torch.arange(n, P, device=dev))
        self._n_spare, self._n_spare_stale = P - n, False
        self._maintain_ctx = self._last_probe = None  # (sized on the map that was here before)
        self.set_training_rows()
        self._act_valid = False
        self.begin_mapping_call(reset_optimizer=True)
        for g in self._graphs():
            g.stale = True
        self.activate()  # (a captured iteration starts from the activations of the current parameters)

    @classmethod
    def from_model_ply(cls, path, stable_path, settings, device, spare_rows=0, **kw):
        """A mapper of the files' row count and SH size, started from disk: the constructor on placeholder values, reserve(spare_rows),
        track_lifecycle() and load_model(path, stable_path) — what metric.py / make_mesh.py do with a saved map.  kw: the constructor's
        (and `tick` for load_model)."""
        tick = kw.pop("tick", 0)
        tables, M = cls._read_checkpoint(path, stable_path)
        n = sum(int(t.shape[0]) for t in tables if t is not None)
        if n < 1:
            raise RuntimeError("FusedMapper.from_model_ply: the files hold no rows")
        scene = dict(xyz=np.zeros((n, 3), np.float32), shs=np.zeros((n, M, 3), np.float32), opacity=np.full((n, 1), 0.5, np.float32),
                     scales=np.ones((n, 3), np.float32), rotations=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
        fm = cls(scene, settings, device, **kw)
        fm.reserve(spare_rows)
        fm.track_lifecycle()
        fm._load_tables(tables, M, tick)
        return fm

    # ------------------------------------------------------------------ growth sampling (csrc/map_sample.hip) ------------
    # configs/base.yaml:32-33, 47-52
    SAMPLE_DEFAULTS = dict(uniform_sample_num=50000, add_transmission_thres=0.5, add_depth_thres=None, add_color_thres=0.1,
                           transmission_sample_ratio=1.0, error_sample_ratio=0.05, init_opacity=0.99, xyz_factor=(1.0, 1.0, 0.1),
                           capacity=None, key_bits=32)

    @torch.no_grad()
    def sample_new(self, frame_map, settings=None, *, seed, tick, first_frame=False, model_map=None, **thresholds):
        """The first statement of a mapping frame — Mapping.temp_points_init (SLAM/multiprocess/mapper.py:1231-1347): get_render_output
        (:1673-1688; the whole map rendered at the frame's camera on the persistent context maintain() keeps: colour, depth, T_map, depth
        hit index) followed by dqo_mapgrowth.temp_points_init on the frame.  frame_map: the reference's dict (depth_map [H,W,1],
        vertex_map_w, normal_map_w, color_map [H,W,3], optional instance_img [H,W,3]); settings: the frame's camera (default: the
        mapper's); first_frame: the form without a render (:1234-1247).  thresholds: SAMPLE_DEFAULTS (add_depth_thres None = the
        mapper's).  Returns what grow() takes, so a frame runs as grow(sample_new(...), ...) -> window -> maintain(...); the counts of the
        call are left in self.sample_header.  With an object gate the mapper keeps the rows of the objects it holds: a shard's rows are
        the unsharded mapper's rows with its objects' ids, in the same order — given the same render: both k are whole-frame counts, so a
        shard passes the WHOLE map's render as model_map (dqo_mapgrowth.temp_points_init's dict; its own render shows its objects only).
        The sampler's buffers are made once per capacity."""
        unknown = set(thresholds) - set(self.SAMPLE_DEFAULTS)
        if unknown:
            raise TypeError(f"FusedMapper.sample_new: unknown thresholds {sorted(unknown)}")
        th = dict(self.SAMPLE_DEFAULTS, **thresholds)
        if th["add_depth_thres"] is None:
            th["add_depth_thres"] = self.add_depth_thres
        dev = self.device
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if th["capacity"] is None:
            th["capacity"] = mg.sample_capacity(H, W, first_frame, th["uniform_sample_num"], th["transmission_sample_ratio"], th["error_sample_ratio"])
        with torch.cuda.device(dev):
            if first_frame:
                model_map = None
            elif model_map is None:
                st = self._settings_or_own(settings)
                self.activate()
                c = self._maintain_render(st)
                if self.maintain_overflowed():  # (the frame outgrew the context an earlier frame sized: size a new one)
                    c = self._maintain_render(st)
                out = c.out
                model_map = dict(render_color=out[0].permute(1, 2, 0), render_depth=out[1].permute(1, 2, 0),
                                 render_depth_index=out[3].permute(1, 2, 0), render_transmission=out[6].permute(1, 2, 0))
            s = self._sample_ctx
            if s is None or s["key"] != (th["capacity"], self.M):
                s = self._sample_ctx = dict(key=(th["capacity"], self.M), buffers=mg.sample_buffers(th["capacity"], self.M, dev),
                                            workspace=torch.empty((N.lib().dqo_growth_sample_workspace_bytes(W, H),), dtype=torch.uint8, device=dev))
            new, self.sample_header = mg.temp_points_init(frame_map, model_map, seed=seed, tick=tick, sh_coeffs=self.M, buffers=s["buffers"],
                                                          workspace=s["workspace"], **th)
            if self.gaussian_object is not None:
                if "obj_id" not in new:
                    raise RuntimeError("FusedMapper.sample_new: with an object gate the frame needs 'instance_img'")
                held = torch.zeros((64,), dtype=torch.bool, device=dev)
                held[(self.gaussian_object if self.alive is None else self.gaussian_object[self.alive.bool()]).long()] = True
                keep = held[new["obj_id"].clamp(0, 63).long()] & (new["obj_id"] >= 0) & (new["obj_id"] < 64)
                new = {k: v[keep] for k, v in new.items()}
        return new

    # ------------------------------------------------------------------ the window's masks (csrc/map_tilemask.hip) --------
    @torch.no_grad()
    def refresh_window(self, frames=None, *, global_opt=False, sample_ratio=-1, rows=None, out=None):
        """The loop that opens every mapping call of the reference — `for frame in self.processed_frames: render_mask, tile_mask, _ =
        self.evaluate_render_range(frame)` (SLAM/multiprocess/mapper.py:549-555, 1173-1189; the function: :930-988) — for the captured
        frames of the window (`frames`: the slots, default all of them), on the GPU and in place.  Per frame: the cloud `rows` (bool [P];
        default trained_rows(), the reference's choice in both callers — `unstable_params` in local_optimize, `stable_params` in
        global_optimization; every other row and every spare row is hidden through DqoRastInputs.row_flags) rendered at the frame
        graph's own camera on the persistent context maintain() keeps, then dqo_tilemask.window_masks on its T_map (error mode: also its
        colour and the graph's target) straight into the graph's render mask and tile mask: the next replay trains under them.  Mixed
        graphs (k, m) that use frame m's masks get them by device copies, each buffer once, as set_frame does.
        global_opt / sample_ratio: evaluate_render_range's (the local, error and final branch).  Returns the float32 [K] device tensor of
        the frames' render ratios (`out`, or this mapper's own table for K, overwritten by the next call with the same K).
        The FIRST call for a (P, H, W) sizes the render's context from one 32-byte header read, exactly as maintain() does; after that a
        call reads nothing back, keeps no new allocation and does not synchronise.  A frame that outgrows that context keeps its old
        masks and gets a NaN ratio; maintain_overflowed() tells (about the LAST frame rendered) where a read is affordable.
        Refused before anything is launched: a frame captured without a render mask; a frame whose tile mask is this mapper's shared
        all-ones tile mask (writing it would change every default-mask render of the mapper); a sharded mapper; an image size other than
        the mapper's."""
        self._refuse_sharded("refresh_window")
        dev = self.device
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        gy, gx = (H + 15) // 16, (W + 15) // 16
        slots = [k for k, g in enumerate(self._frames) if g is not None] if frames is None else [int(k) for k in frames]
        for k in slots:
            if not 0 <= k < len(self._frames) or self._frames[k] is None:
                raise RuntimeError(f"FusedMapper.refresh_window: frame {k} of the window is not captured")
            g = self._frames[k]
            if (int(g.settings.image_height), int(g.settings.image_width)) != (H, W):
                raise RuntimeError("FusedMapper.refresh_window: every frame of a mapper has the mapper's image size")
            if g.mask is None:
                raise RuntimeError(f"FusedMapper.refresh_window: frame {k} was captured without a render mask")
            if g.tile_mask is self.tile_mask or g.tile_mask.data_ptr() == self.tile_mask.data_ptr():
                raise RuntimeError(f"FusedMapper.refresh_window: frame {k} was captured without a tile mask of its own (it reads the "
                                   "mapper's shared all-ones tile mask, which every default-mask render reads too)")
            if g.mask.numel() != H * W or g.tile_mask.numel() != gy * gx:
                raise RuntimeError("FusedMapper.refresh_window: every frame of a mapper has the mapper's image size")
        targets = [(lambda g=self._frames[k]: g.settings, self._frames[k].gt_color, self._frames[k].mask.view(H, W),
                    self._frames[k].tile_mask.view(gy, gx)) for k in slots]
        table = self._window_mask_pass("refresh_window", targets, global_opt, sample_ratio, rows, out)
        done = set()
        for k in slots:
            done.update((self._frames[k].mask.data_ptr(), self._frames[k].tile_mask.data_ptr()))
        with torch.cuda.device(dev):
            for k in slots:
                g = self._frames[k]
                for (_, m), g2 in self._mixed.items():
                    if m != k:
                        continue
                    for src, dst in ((g.mask, g2.mask), (g.tile_mask, g2.tile_mask)):
                        if dst is not None and dst.data_ptr() not in done and dst.data_ptr() != self.tile_mask.data_ptr():
                            done.add(dst.data_ptr())
                            dst.copy_(src.view(dst.shape))
        return table

    def _window_mask_pass(self, who, targets, global_opt, sample_ratio, rows, out):
        """The loop refresh_window and refresh_bank share.  targets: per frame (camera: a call that returns the settings to render at,
        made when the frame's turn comes; gt_color; render mask uint8 [H,W]; tile mask int32 [gy,gx]) — the masks are written in place.
        Returns the ratio table (refresh_window says what `rows` and `out` are and what the first call reads back)."""
        dev = self.device
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if rows is None:
            rows = self.trained_rows()
        elif not torch.is_tensor(rows) or rows.dtype != torch.bool or rows.numel() != self.P or rows.device != self.row_flags.device:
            raise RuntimeError(f"FusedMapper.{who}: rows must be a bool GPU tensor with one entry per row")
        K = len(targets)
        if out is None:
            table = self._own_table(self._window_ratios, K)
        elif out.dtype != torch.float32 or tuple(out.shape) != (K,) or not out.is_contiguous() or out.device != self.row_flags.device:
            raise RuntimeError(f"FusedMapper.{who}: out must be a contiguous float32 [{K}] tensor on the mapper's device")
        else:
            table = out
        with torch.cuda.device(dev):
            if self._window_ws is None:
                self._window_ws = dqo_tilemask.window_masks_workspace(H, W, dev)
            if self._window_flags is None:
                self._window_flags = torch.empty((self.P,), dtype=torch.uint8, device=dev)
            hidden = ~rows.reshape(-1)
            if self.alive is not None:  # a spare row is no Gaussian of the map, whichever cloud is asked for
                hidden |= self.alive == 0
            self._window_flags.copy_(hidden).mul_(N.ROW_HIDDEN)
            self.activate()
            for i, (camera, gt_color, render_mask, tile_mask) in enumerate(targets):
                c = self._maintain_render(camera(), row_flags=self._window_flags)
                o = c.out
                dqo_tilemask.window_masks(o[6], o[0], gt_color, global_opt=global_opt, sample_ratio=sample_ratio, render_mask=render_mask,
                                          tile_mask=tile_mask, ratio_out=table[i:i + 1], render_header=c.geom, workspace=self._window_ws)
        return table

    @torch.no_grad()
    def refresh_bank(self, slots=None, *, global_opt=False, sample_ratio=-1, rows=None, out=None):
        """refresh_window's loop for the keyframes of the bank (capture_bank; `slots`: default every filled one): the cloud `rows` rendered
        at the slot's camera, dqo_tilemask.window_masks straight into the slot's render mask and tile mask in the bank — the next select
        launch that names the slot copies them (force is set: also when the slot is the one the graph holds).  Returns the ratio table
        as refresh_window does; like it, a call after the first for a (P, H, W) reads nothing back and does not synchronise."""
        self._refuse_sharded("refresh_bank")
        bank = self._require_bank("refresh_bank")
        slots = bank.slots() if slots is None else [int(k) for k in slots]
        for k in slots:
            if not 0 <= k < bank.K_cap or not bank.filled[k]:
                raise RuntimeError(f"FusedMapper.refresh_bank: slot {k} of the bank holds no keyframe")
        targets = [(lambda k=k: bank.camera_of(k), bank.gt_color[k], bank.render_mask[k], bank.tile_mask[k]) for k in slots]
        table = self._window_mask_pass("refresh_bank", targets, global_opt, sample_ratio, rows, out)
        bank.word("force").fill_(1)
        return table
