"""Fused mapping iteration: the same arithmetic as

    out = render(settings, params.activated()); loss = mapping_loss(out, gt, mask); loss.backward(); adam.step()

(dqo_harness/mapping.py, i.e. SLAM/multiprocess/mapper.py:531-605 + 836-875 + gaussian_pointcloud.py:331-378), but without
the autograd graph and the ~110 eager launches per iteration: activation kernel -> rasteriser forward -> fused masked-loss
forward+backward -> rasteriser backward -> fused (activation-Jacobian + Adam) kernel.  The rasteriser is called through the
same operator code (`_RasterizeGaussians.forward / .backward`), so it is the same C-ABI path the drop-in op uses.

`capture()` records one whole iteration (eight kernel launches since round 3: zero fill, preprocess, binning, two sort kernels, forward
blend with the loss tap, backward blend, and ONE per-Gaussian tail — record sums, the per-Gaussian chain and Adam; no memset node, no
host synchronisation, the Adam step count, the attach set and its size kept on the device) into a hipGraph over persistent buffers;
`replay()` re-issues it with a single launch call — at ~0.53 ms of GPU work per iteration on config 3 the per-launch host work of the
eager path is otherwise longer than the GPU work.  `reserve()` + `grow()` + `begin_mapping_call()` keep the captured graph valid across
map-growth steps and mapping calls (everything they change is rewritten in place).

Round 6 — the reference's optimise LOOP, not one frame of it (mapper.py:531-605, 1105-1228): a frame set (`capture_window`: one graph
per frame of the window / keyframe selection, each with its own context buffers and capacities, all sharing parameters, moments and the
device-side step count; `replay(frame)` = the per-iteration frame choice, `run_window` = the reference's schedule), the two clouds in
one map (`set_training_rows`: the rows the call trains and the rows it renders; frozen rows are rendered and back-propagated through
but are no parameters of the call), per-call learning rates in device memory (`set_lrs`), the per-iteration confidence counter
(`confidence`, mapper.py:908-910) inside the tail kernel, and `history_merge()` (mapper.py:607-650) as one kernel.

With a render mask (every live call site of the reference) the loss is the masked L1 pair and the reference skips SSIM (B14); without
one the SSIM term of mapper.py:839-845 is added by dqo_map_ssim_fwd_bwd (three launches; the loss tap is off then — the SSIM gradient
is an image).  GPU only.

What looks at or rewrites the whole map between iterations (maintain, prune_floaters, evaluate*, make_mesh, the checkpoints, sample_new,
refresh_window) and the scratch it keeps is dqo_harness/map_operators.py: FusedMapper derives from its MapOperators.  This file keeps the
row table (_ROW_BUFFERS), reserve() / grow(), track_lifecycle() and the captured graphs.
"""
import collections
import ctypes
import os
import threading

import numpy as np
import torch

import _dqo_native as N
import diff_gaussian_rasterization_depth as dgr
import dqo_mapgrowth as mg
from _dqo_context import bucket_for, capacity_for, header_words, overflowed, read_header
from dqo_harness import mapping
from dqo_harness.map_operators import MapOperators, _RenderContext, _checked_tile_mask, _normalised_settings


def tile_object_sets(pixel_object):
    """DqoObjectGate.tile_objects of a pixel_object map (int32 [H, W], ids in [0, 64), < 0 = no owner): per 16x16 tile the 64-bit set of
    the owners among its pixels, as an int64 tensor [ceil(H/16) * ceil(W/16)] (bit patterns; row-major tiles)."""
    H, W = pixel_object.shape
    gy, gx = (H + 15) // 16, (W + 15) // 16
    pad = torch.full((gy * 16, gx * 16), -1, dtype=torch.int64, device=pixel_object.device)
    pad[:H, :W] = pixel_object
    t = pad.reshape(gy, 16, gx, 16).permute(0, 2, 1, 3).reshape(gy * gx, 256)
    bits = torch.where(t >= 0, torch.ones_like(t) << t.clamp(min=0), torch.zeros_like(t))
    out = bits[:, 0].clone()
    for j in range(1, 256):  # (bitwise OR over the tile's pixels; once per mapping call)
        out |= bits[:, j]
    return out.contiguous()


class _Ctx:
    """Stand-in for the autograd ctx when the op's static forward/backward are driven directly."""

    def save_for_backward(self, *a):
        self.saved_tensors = a

    def mark_non_differentiable(self, *a):
        pass


class _SideJob:
    """`work` on the stream `side`, beside the caller's own kernels: start() runs it on a host thread of its own (threaded=False: in
    line, the A/B of the overlap); result() joins both and returns what it returned or raises what it raised."""

    def __init__(self, work, side, threaded):
        self.work, self.side, self.value, self.error = work, side, None, None
        self.thread = threading.Thread(target=self._run) if threaded else None

    def _run(self):
        try:
            self.value = self.work()
        except BaseException as e:  # (re-raised by result(), in the caller's thread)
            self.error = e

    def start(self):
        self.thread.start() if self.thread is not None else self._run()
        return self

    def result(self):
        if self.thread is not None:
            self.thread.join()
        torch.cuda.current_stream().wait_stream(self.side)
        if self.error is not None:
            raise self.error
        return self.value


# Every tensor of a FusedMapper with one row per Gaussian, declared once.  reserve(), grow(), begin_mapping_call() and the state snapshots
# iterate this table (FusedMapper._rows) instead of naming the buffers: a new per-Gaussian buffer is one line here plus the code that
# uses it.  A buffer is the mapper's attribute `name` (`of` = (k, i): the Adam moment state[k][i]), None while it does not exist.
#   group  "param" the raw parameters Adam trains | "moment" Adam's moments and the sparse Adam's flag | "snapshot" init_stat of the
#          mapping call (src: the parameter begin_mapping_call copies; attach_mask is computed) | "meta" what a row is | "sized" sized
#          by P (shape: P -> shape), made anew when P changes (spare None: uninitialised, else the fill) | "dropped" dropped when P changes
#   spare  the value of a spare row (reserve): "park" = _park_position(), "unit_q" = the unit quaternion
#   freed  an in-place growth step writes `spare` into the rows it frees: what makes the row a spare row for the kernels
#   live   the value of a row a Gaussian moves into, where the growth step computes none
_RowBuffer = collections.namedtuple("_RowBuffer", "name group spare freed live src of shape", defaults=(None, False, 0, None, None, None))
_LIFECYCLE_ROWS = ("stable", "add_tick", "depth_error_counter", "color_error_counter", "frame_id")
_ROW_BUFFERS = (
    _RowBuffer("xyz", "param", "park", freed=True), _RowBuffer("shs", "param", 0.0), _RowBuffer("opacity_raw", "param", -10.0, freed=True),
    _RowBuffer("scaling_raw", "param", -10.0, freed=True), _RowBuffer("rotation_raw", "param", "unit_q"),
    *(_RowBuffer(f"state[{k}][{i}]", "moment", 0.0, of=(k, i)) for k in ("xyz", "shs", "opacity", "scaling", "rotation") for i in (0, 1)),
    _RowBuffer("moment_live", "moment", 0),
    _RowBuffer("init_xyz", "snapshot", "park", src="xyz"), _RowBuffer("init_scaling", "snapshot", -10.0, src="scaling_raw"),
    _RowBuffer("init_rotation", "snapshot", "unit_q", src="rotation_raw"), _RowBuffer("attach_mask", "snapshot", 0),
    _RowBuffer("alive", "meta", 0, freed=True, live=1),
    _RowBuffer("row_flags", "meta", N.ROW_HIDDEN | N.ROW_FROZEN, freed=True),  # (a spare row: not rendered, not trained)
    _RowBuffer("confidence", "meta", 0.0, freed=True), _RowBuffer("gaussian_object", "meta", 0),
    # track_lifecycle(): which of the reference's two clouds a row belongs to (1 = stable_pointcloud) and what maintain() keeps per row
    # (SLAM/gaussian_pointcloud.py:43-46)
    _RowBuffer("stable", "meta", 0, freed=True), _RowBuffer("add_tick", "meta", 0, freed=True),
    _RowBuffer("depth_error_counter", "meta", 0, freed=True), _RowBuffer("color_error_counter", "meta", 0, freed=True),
    # track_lifecycle(): the frame a row was added at (GaussianPointCloud._frame_ids, SLAM/gaussian_pointcloud.py:52): prune_floaters()' window
    _RowBuffer("frame_id", "meta", 0, freed=True),
    _RowBuffer("opacity", "sized", shape=lambda P: (P, 1)), _RowBuffer("scales", "sized", shape=lambda P: (P, 3)),
    _RowBuffer("rotations", "sized", shape=lambda P: (P, 4)),
    # (one partial sum per block of 256 Gaussians from dqo_map_adam_step, per wave of 64 from dqo_rast_backward_adam)
    _RowBuffer("attach_partial", "sized", 0.0, shape=lambda P: (4 * ((P + 255) // 256),)),
    _RowBuffer("init_shs", "dropped"), _RowBuffer("init_confidence", "dropped"),
)


class _FrameGraph:
    """One captured mapping iteration of a FusedMapper (capture()): the frame's inputs, the options it was captured with, and the
    capacities, buffers and C structs the capture fixed (the graph holds their addresses)."""

    def __init__(self, frame, settings, pixel_object, tile_objects, gt_color, gt_depth, mask, tile_mask, options):
        self.frame = frame  # slot of the window (None: the single-frame mapper's graph; (k, m): a mixed graph of _graph_of; "bank": capture_bank's)
        # the frame's inputs, read in place at every replay and rewritten in place by set_frame: the graph's own copies of the camera
        # tensors, the gate's owner map and its tile sets (None: no gate), the target images, the uint8 render mask (None: unmasked)
        self.settings, self.pixel_object, self.tile_objects = settings, pixel_object, tile_objects
        self.gt_color, self.gt_depth, self.mask, self.tile_mask = gt_color, gt_depth, mask, tile_mask
        # capture()'s options as passed (tile_buckets, keep_tile_order, loss_tap, fused_tail, list_split, unroll, run_unroll,
        # short_bucket_margin): _recapture passes them again
        self.options = options
        # capture_bank's graph: the keyframe bank, whose select launch every iteration of this graph issues first (None: the frame's inputs
        # change by set_frame alone), and that launch's DqoWindowBank over this graph's buffers
        self.head, self.head_args = options.get("head"), None
        self.stale = False  # the attach set / object gate changed since the capture: its kernel arguments point at freed buffers
        self.cap = 0  # instance capacity
        self.bucket = 0  # DqoRastCtx.tile_bucket_capacity (0: packed lists)
        self.out = None  # the op's 9 outputs (dgr._new_outputs) of the last iteration
        self.ctx = self.geom = self.img = self.binning = self.ws = None  # the context (its buffers by name) and the backward's workspace
        self.grads = None  # gradient rows of the unfused tail (dict: means3D, sh, opacity, scales, rot)
        self.grad_scale = None  # DqoLossTap.grad_scale
        # the step state is the mapper's, shared by all its graphs (DqoAdamStep.step_dev: the Adam launch advances it itself through
        # block_ticket; bias_table: the bias corrections, computed once per step)
        self.step_dev = self.ticket = self.bias = None
        self.params = self.inputs = self.outputs = self.cctx = self.cgrads = self.adam = None
        self.tap = self.gate = None  # DqoLossTap (None: loss kernels), DqoObjectGate (None: no gate)
        self.ls_fwd = self.ls_bwd = 0  # DqoRastCtx.list_split of the forward and of the backward call
        self.fused_tail = False  # the per-Gaussian backward and Adam as one kernel (dqo_rast_backward_adam)
        self.unroll, self.graph = 1, None  # iterations per replay(), the graph
        self.run_unroll, self.run_graph = 1, None  # iterations per launch of replay_run's graph (None: run_unroll is 1)


_CAMERA_ROW = (("bg", 0, 3), ("viewmatrix", 3, 19), ("projmatrix", 19, 35), ("campos", 35, 38))  # floats of a bank's camera row (DqoWindowBank)
_CAPTURED_SCALARS = ("image_height", "image_width", "tanfovx", "tanfovy", "cx", "cy", "sh_degree", "scale_modifier", "opaque_threshold",
                     "depth_threshold", "normal_threshold", "color_sigma", "T_threshold")  # kernel arguments of a captured iteration


class _KeyframeBank:
    """The keyframe bank of a FusedMapper (capture_bank): K_cap slots of everything a captured iteration reads per frame, in device
    memory (DqoWindowBank's layout), the staging buffers ONE captured graph reads, the schedule, the select launch's state words and its
    lost-frame log.  dqo_window_bank_select, issued at the head of every iteration of that graph, moves the scheduled slot into the
    staging buffers (csrc/map_window_bank.hip)."""

    def __init__(self, K_cap, st, gate, schedule_capacity, device):
        H, W = int(st.image_height), int(st.image_width)
        gy, gx = (H + 15) // 16, (W + 15) // 16
        f, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
        self.K_cap, self.H, self.W, self.gate, self.device = int(K_cap), H, W, bool(gate), device
        self.scalars = st  # the intrinsics every slot shares: captured kernel arguments
        self.filled = [False] * self.K_cap
        self.rows = [None] * self.K_cap  # the trajectory row a slot's camera follows (bank_set(row=...)); None: not bound
        self.camera = torch.zeros((K_cap, 40), **f)
        self.gt_color, self.gt_depth = torch.empty((K_cap, 3, H, W), **f), torch.empty((K_cap, 1, H, W), **f)
        self.render_mask = torch.zeros((K_cap, H, W), dtype=torch.uint8, device=device)
        self.tile_mask = torch.ones((K_cap, gy, gx), **i32)
        self.pixel_object = torch.full((K_cap, H, W), -1, **i32) if gate else None
        self.tile_objects = torch.zeros((K_cap, gy * gx), dtype=torch.int64, device=device) if gate else None
        # what the graph reads (capture() makes its own copies of the camera tensors and of the gate's tile sets: DqoWindowBank's
        # destination is taken from the graph, select())
        self.stage = dict(gt_color=torch.empty((3, H, W), **f), gt_depth=torch.empty((1, H, W), **f),
                          render_mask=torch.zeros((H, W), dtype=torch.uint8, device=device), tile_mask=torch.ones((gy, gx), **i32),
                          pixel_object=torch.full((H, W), -1, **i32) if gate else None)
        # a camera in tensors of its own for the renders that read a slot in place (probe(), refresh_bank): a camera row's parts start
        # on 4-byte boundaries, the allocator's tensors on 256-byte ones
        self.camera_scratch = st._replace(bg=torch.zeros((3,), **f), viewmatrix=torch.zeros((16,), **f), projmatrix=torch.zeros((16,), **f),
                                          campos=torch.zeros((3,), **f))
        self.schedule = torch.zeros((max(1, int(schedule_capacity)), 2), **i32)
        self.lost = torch.zeros((self.schedule.shape[0],), **i32)
        self.state = torch.zeros((N.WINDOW_BANK_STATE_WORDS,), **i32)
        self.graph = None  # the _FrameGraph (frame "bank"); None: run_bank captures it
        self.capture_kw, self.capacity_margin, self.unroll = {}, 1.15, 1

    def slots(self):
        return [k for k, on in enumerate(self.filled) if on]

    def word(self, name):
        """The state word `name` (N.WINDOW_BANK_WORDS) as a one-element view."""
        at = N.TICKET_WORDS + N.WINDOW_BANK_WORDS.index(name)
        return self.state[at:at + 1]

    def camera_of(self, slot):
        """Slot's camera as settings over camera_scratch (four small device copies; the next call overwrites them)."""
        for name, a, b in _CAMERA_ROW:
            getattr(self.camera_scratch, name).copy_(self.camera[slot, a:b])
        return self.camera_scratch

    def stage_slot(self, slot, g=None):
        """Slot's parts into the staging buffers by host-issued copies (graph g given: into the buffers it reads)."""
        dst = self.stage if g is None else dict(gt_color=g.gt_color, gt_depth=g.gt_depth, render_mask=g.mask, tile_mask=g.tile_mask,
                                                pixel_object=g.pixel_object)
        for name in ("gt_color", "gt_depth", "render_mask", "tile_mask") + (("pixel_object",) if self.gate else ()):
            dst[name].copy_(getattr(self, name)[slot].view(dst[name].shape))
        if g is not None:
            for name, a, b in _CAMERA_ROW:
                getattr(g.settings, name).copy_(self.camera[slot, a:b].view(getattr(g.settings, name).shape))
            if self.gate:
                g.tile_objects.copy_(self.tile_objects[slot].view(g.tile_objects.shape))

    def probe(self, mapper):
        """(candidates, longest tile list) a graph that serves every filled slot must hold: the maximum of FusedMapper._probe under
        each slot's own camera, tile mask and owner map."""
        cand = longest = 0
        for k in self.slots():
            c, l = mapper._probe(self.tile_mask[k], self.camera_of(k), self.pixel_object[k] if self.gate else None,
                                 self.tile_objects[k] if self.gate else None)
            cand, longest = max(cand, c), max(longest, l)
        return cand, longest

    def select(self, g, stream):
        """dqo_window_bank_select into graph g's input buffers (the launch a captured iteration starts with)."""
        if g.head_args is None:
            st, gate = g.settings, self.gate
            g.head_args = N.DqoWindowBank(
                W=self.W, H=self.H, K_cap=self.K_cap, n=self.schedule.shape[0], camera=N.ptr(self.camera), gt_color=N.ptr(self.gt_color),
                gt_depth=N.ptr(self.gt_depth), render_mask=N.ptr(self.render_mask), tile_mask=N.ptr(self.tile_mask),
                pixel_object=N.ptr(self.pixel_object) if gate else None, tile_objects=N.ptr(self.tile_objects) if gate else None,
                dst_bg=N.ptr(st.bg), dst_viewmatrix=N.ptr(st.viewmatrix), dst_projmatrix=N.ptr(st.projmatrix), dst_campos=N.ptr(st.campos),
                dst_gt_color=N.ptr(g.gt_color), dst_gt_depth=N.ptr(g.gt_depth), dst_render_mask=N.ptr(g.mask), dst_tile_mask=N.ptr(g.tile_mask),
                dst_pixel_object=N.ptr(g.pixel_object) if gate else None, dst_tile_objects=N.ptr(g.tile_objects) if gate else None,
                schedule=N.ptr(self.schedule), state=N.ptr(self.state), lost=N.ptr(self.lost), render_header=g.geom.data_ptr())
        N.check(N.lib().dqo_window_bank_select(ctypes.byref(g.head_args), stream))

    def arm(self, n, stream):
        N.check(N.lib().dqo_window_bank_arm(N.ptr(self.state), int(n), stream))


class FusedMapper(MapOperators):
    def __init__(self, scene, settings, device, lrs=None, betas=(0.9, 0.999), eps=1e-15, color_weight=mapping.COLOR_WEIGHT,
                 depth_weight=mapping.DEPTH_WEIGHT, add_depth_thres=0.1, sparse_moments=True, attach=True, attach_count_reducer=None):
        t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=device)
        self.device = device
        self.settings = _normalised_settings(settings, device)
        self.xyz = t(scene["xyz"])
        self.shs = t(scene["shs"])  # [P, M, 3]; coefficient 0 is f_dc, the rest f_rest (no torch.cat per iteration)
        op = t(scene["opacity"]).clamp(1e-4, 1 - 1e-4)
        self.opacity_raw = torch.log(op / (1 - op))
        self.scaling_raw = torch.log(t(scene["scales"]))
        self.rotation_raw = t(scene["rotations"]).clone()
        self.P, self.M = self.xyz.shape[0], self.shs.shape[1]
        self.lrs = dict(mapping.LRS if lrs is None else lrs)
        self.betas, self.eps = betas, eps
        self.color_weight, self.depth_weight, self.add_depth_thres = color_weight, depth_weight, add_depth_thres
        self.state = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in self._params().items()}
        # exact sparse Adam (DqoAdamStep.moment_live): 0 = the Gaussian's moments are still identically zero
        self.moment_live = torch.zeros((self.xyz.shape[0],), dtype=torch.uint8, device=device) if sparse_moments else None
        self.step_count = 0
        # Device-side step state SHARED by every captured graph of this mapper (one graph per frame of a window: capture_window):
        # DqoAdamStep.step_dev / block_ticket / bias_table.  _expected_step = what step_dev holds while host and device counts agree.
        i32 = dict(dtype=torch.int32, device=device)
        self._step_dev = torch.full((1,), 1, **i32)
        self._ticket = torch.zeros((N.TICKET_WORDS,), **i32)
        self._bias = torch.zeros((8,), dtype=torch.float32, device=device)
        self._expected_step, self._unsettled = 1, False
        # DqoAdamStep.block_ticket: the Adam launch advances the device step count itself (False: a one-thread launch behind it does)
        self.use_block_ticket = True
        # _g: the graph replayed last / by default (a _FrameGraph); _frames: the captured graphs of a window (capture_window);
        # _mixed: (k, m) -> graph of frame k's camera and target under frame m's masks (global_optimization's quirk)
        self._drop_graphs()
        self._window_kw, self._window_frames = {}, []  # capture_window's arguments: _graph_of captures mixed graphs from them
        self._bank = None  # capture_bank's keyframe bank (_KeyframeBank); its graph is one of _graphs()
        self._last_probe = None  # (candidates, longest list, P) the last capture was sized on: capture(reuse_probe=True)
        self._side_stream = None  # grow()'s stream for the attach step (made once: creating a stream costs a growth step ~1 ms)
        # The reference keeps TWO clouds and trains one of them per mapping call while it renders one or both (mapper.py:533, 578,
        # 1119, 1199-1204).  One map here: DqoAdamStep.row_flags / DqoRastInputs.row_flags (bit 0 = not trained, bit 1 = not rendered),
        # rewritten in place by set_training_rows — a captured graph follows.
        self.row_flags = torch.zeros((self.P,), dtype=torch.uint8, device=device)
        self._first_trained_row = 0
        # `_confidence` (SLAM/gaussian_pointcloud.py:42, 836): += 1 per iteration for every trained row with a non-zero f_dc gradient
        # (mapper.py:908-910), counted by the Adam launch itself (DqoAdamStep.confidence)
        self.confidence = torch.zeros((self.P,), dtype=torch.float32, device=device)
        self.count_confidence = True
        # the six groups' learning rates in device memory (DqoAdamStep.lr_table): set_lrs rewrites them between two mapping calls
        self.lr_table = torch.zeros((6,), dtype=torch.float32, device=device)
        self._write_lr_table()
        self.history_merge_weight = 0.5  # history_merge_max_weight, configs/base.yaml:54
        self.init_shs = self.init_confidence = None  # history_stat's other members (begin_mapping_call(history=True))
        self._act_valid = False  # opacity / scales / rotations hold the activations of the current raw parameters
        self.use_attach = bool(attach)
        # The attach loss is a mean over the attach set of the WHOLE map (mapper.py:812-829).  A mapper that holds a shard of the map
        # must divide by the whole map's count for the shards to add up to the unsharded job: attach_count_reducer(local count) -> global
        # count (e.g. one all-reduce of one integer per mapping call — not per iteration); None = this mapper holds the whole map.
        self.attach_count_reducer = attach_count_reducer
        self.gaussian_object = self.pixel_object = self.tile_objects = None  # set_object_gate()
        self.object_cell = None  # per-object growth decisions: cell size of dqo_mapgrowth.object_offsets (None = its 16 m default)
        self.per_object_loss = False
        self.alive = None  # reserve(): uint8 [P], 0 = a spare row (parked behind the camera, no Gaussian of the map)
        self.stable = self.add_tick = self.depth_error_counter = self.color_error_counter = self.frame_id = None  # track_lifecycle()
        self._n_spare_stale = False  # maintain() freed rows on the device since _n_spare was read
        self._init_operator_state()  # (the whole-map operators' scratch: map_operators.py)
        self._n_spare = self._spare_rows = 0  # spare rows now (host copy of the count: grow() keeps it up to date) / as reserve()d
        # DqoAdamStep.attach_gains: the attach term's two factors in device memory, rewritten in place by begin_mapping_call — a captured
        # graph survives a new mapping call
        self.attach_gains = torch.zeros((2,), dtype=torch.float32, device=device)
        self.init_xyz = self.init_scaling = self.init_rotation = self.attach_mask = None  # init_stat: begin_mapping_call takes it
        self._row_count_changed()  # (makes the activations and attach_partial)
        self.begin_mapping_call(reset_optimizer=False)
        f = dict(dtype=torch.float32, device=device)
        H, W = settings.image_height, settings.image_width
        self.dL_dcolor = torch.empty((3, H, W), **f)
        self.dL_ddepth = torch.empty((1, H, W), **f)
        self.loss = torch.zeros(8, **f)  # dqo_map_loss_fwd_bwd: total, colour, depth, 0, then the four unnormalised sums
        lib = N.lib()
        self.loss_ws = torch.empty((lib.dqo_map_loss_workspace_bytes(),), dtype=torch.uint8, device=device)
        # the unmasked branch of Mapping.loss_update adds 0.2 * (1 - ssim) (mapper.py:839-845): dqo_map_ssim_fwd_bwd, buffers made on first use
        self.ssim_weight = mapping.SSIM_WEIGHT
        self.ssim_out = self.ssim_ws = None
        self._empty = torch.Tensor([])
        self.tile_mask = torch.ones(((H + 15) // 16, (W + 15) // 16), dtype=torch.int32, device=device)

    def set_object_gate(self, gaussian_object, pixel_object, per_object_loss=True):
        """The per-object job of SURVEY.md §8(e) (not a reference feature): gaussian_object int32 [P] (every Gaussian's object id, >= 0),
        pixel_object int32 [H, W] (every pixel's owner, < 0 = none).  A list entry then acts on a pixel only if the ids agree
        (DqoObjectGate), and — per_object_loss — the loss is the sum of the objects' own masked losses (DqoLossTap.per_object;
        ids in [0, 64)), so that what an object learns does not depend on which other objects this mapper holds: shards of one map add up
        to the unsharded job.  None, None switches the gate off (the reference's semantics).  A captured graph must be captured again."""
        if gaussian_object is None:
            self.gaussian_object = self.pixel_object = self.tile_objects = None
            self.per_object_loss = False
        else:
            H, W = int(self.settings.image_height), int(self.settings.image_width)
            go = torch.as_tensor(gaussian_object).to(self.device, torch.int32).contiguous().reshape(-1)
            po = torch.as_tensor(pixel_object).to(self.device, torch.int32).contiguous().reshape(H, W)
            if go.numel() != self.P:
                raise RuntimeError("set_object_gate: gaussian_object must have one id per Gaussian")
            if int(go.min().item()) < 0 or int(go.max().item()) > 63 or int(po.max().item()) > 63:
                raise RuntimeError("set_object_gate: object ids must lie in [0, 64)")
            self.gaussian_object, self.pixel_object, self.per_object_loss = go, po, bool(per_object_loss)
            self.tile_objects = tile_object_sets(po)  # DqoObjectGate.tile_objects: which objects own a pixel of each 16x16 tile
        for g in self._graphs():
            g.stale = True
        return self

    # ------------------------------------------------------------------ the two clouds, per-call learning rates ---------
    def _graphs(self):
        gs = [g for g in self._frames if g is not None] + list(self._mixed.values())
        if self._bank is not None and self._bank.graph is not None:
            gs.append(self._bank.graph)
        if self._g is not None and all(self._g is not f for f in gs):
            gs.append(self._g)
        return gs

    _LR_ORDER = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")

    def _write_lr_table(self):
        # (fill_ carries the python float as a kernel argument: no pageable host copy, no synchronisation)
        for i, k in enumerate(self._LR_ORDER):
            self.lr_table[i:i + 1].fill_(float(self.lrs[k]))

    def set_lrs(self, lrs=None, **scale):
        """The learning rates of the NEXT mapping call, rewritten in device memory (DqoAdamStep.lr_table): captured graphs stay valid.
        `lrs`: dict over xyz / f_dc / f_rest / opacity / scaling / rotation (missing keys keep their value); `scale`: factors on the
        current values, e.g. Mapping.global_optimization's  l[0]["lr"] = 0; l[i]["lr"] *= 0.1  (mapper.py:1120-1123) is
        set_lrs(dict(xyz=0.0), f_dc=0.1, f_rest=0.1, opacity=0.1, scaling=0.1, rotation=0.1).  The bias-correction table of the device
        step is dropped (it holds products with the old rates)."""
        if lrs:
            self.lrs.update({k: float(v) for k, v in lrs.items()})
        for k, f in scale.items():
            self.lrs[k] = self.lrs[k] * float(f)
        self._write_lr_table()
        self._bias.zero_()
        return self

    @torch.no_grad()
    def set_training_rows(self, trainable=None, rendered=None):
        """Which rows the next mapping call TRAINS and which it RENDERS (bool [P] GPU tensors or None = all).  The reference's two clouds:
          local_optimize        trains `pointcloud` (unstable), renders cat(unstable, stable)      (mapper.py:533, 578, 1810-1840)
                                -> set_training_rows(trainable=~stable_mask)
          global_optimization   trains and renders `stable_pointcloud` alone                        (mapper.py:1119, 1199-1204)
                                -> set_training_rows(trainable=stable_mask, rendered=stable_mask)
        A row that is not trained is rendered and back-propagated THROUGH (its list entries shape every pixel it touches) but is no
        parameter of the call: no gradient row is formed, parameters, moments and confidence stay bit for bit, it is in no attach set.
        A row that is not rendered is culled by the per-Gaussian forward (and not trained).  Written in place (DqoAdamStep.row_flags /
        DqoRastInputs.row_flags live in device memory): captured graphs stay valid.  Call before begin_mapping_call (the attach set and
        history_merge's "first row" follow the trained rows)."""
        dev = self.device
        fl = torch.zeros((self.P,), dtype=torch.uint8, device=dev)
        if trainable is not None:
            fl |= (~trainable.to(dev).bool().reshape(-1)).to(torch.uint8) * N.ROW_FROZEN
        if rendered is not None:
            fl |= (~rendered.to(dev).bool().reshape(-1)).to(torch.uint8) * (N.ROW_HIDDEN | N.ROW_FROZEN)
        if self.alive is not None:  # a spare row is no Gaussian of the map, whichever camera looks its way
            fl |= (self.alive == 0).to(torch.uint8) * (N.ROW_HIDDEN | N.ROW_FROZEN)
        self.row_flags.copy_(fl)
        # row 0 of the reference's trained cloud: its history weight serves every row's feature / scaling merge (mapper.py:620-637)
        self._first_trained_row = int(torch.argmax(((fl & N.ROW_FROZEN) == 0).to(torch.uint8)).item())
        return self

    def trained_rows(self):
        """bool [P]: the rows the current mapping call trains."""
        return (self.row_flags & N.ROW_FROZEN) == 0

    @torch.no_grad()
    def history_merge(self, max_weight=None):
        """Mapping.history_merge (mapper.py:607-650), the statement that closes every local_optimize call: the trained rows are pulled back
        towards their state at the start of the call (begin_mapping_call(history=True) took `history_stat`), weighted by the share of
        their confidence that is older than the call.  One launch (dqo_map_history_merge); the activations are recomputed."""
        w = self.history_merge_weight if max_weight is None else float(max_weight)
        if w <= 0:
            return self
        if self.init_shs is None or self.init_confidence is None or self.init_shs.shape[0] != self.P:
            raise RuntimeError("FusedMapper.history_merge: begin_mapping_call(history=True) must have taken history_stat for this map")
        rot0 = torch.nn.functional.normalize(self.init_rotation)  # history_stat["rotation"] = get_rotation (mapper.py:541)
        with torch.cuda.device(self.device):
            N.check(N.lib().dqo_map_history_merge(self.P, self.M, w, self._first_trained_row, N.ptr(self.row_flags), N.ptr(self.init_confidence),
                                                  N.ptr(self.confidence), N.ptr(self.init_xyz), N.ptr(self.init_shs), N.ptr(self.init_scaling),
                                                  N.ptr(rot0), N.ptr(self.xyz), N.ptr(self.shs), N.ptr(self.scaling_raw),
                                                  N.ptr(self.rotation_raw), N.current_stream()))
        self._act_valid = False
        self.activate()  # (a captured iteration starts from the activations of the current parameters)
        return self

    def begin_mapping_call(self, reset_optimizer=True, history=False):
        """Start of one `local_optimize` call (SLAM/multiprocess/mapper.py:531-548): snapshot `init_stat` (the raw parameters the
        attach loss pulls towards, :533-545, and the attach set `sigmoid(opacity) < 0.9`, :812-813) and — reset_optimizer — drop the
        Adam moments, because the reference builds a fresh torch.optim.Adam per call (:548, B13).  Everything is rewritten in place
        when the map has kept its size (buffers, attach set and its size live in device memory: a captured graph stays valid)."""
        P = self.xyz.shape[0]
        mask = (torch.sigmoid(self.opacity_raw) < 0.9).reshape(-1)
        if self.alive is not None:
            mask &= self.alive.bool()  # (a spare row is no Gaussian of the map)
        if self.row_flags.shape[0] == P:
            mask &= (self.row_flags & N.ROW_FROZEN) == 0  # init_stat is the TRAINED cloud's (mapper.py:533-545, 1132-1137)
        if history:  # history_stat's members that only history_merge reads (mapper.py:535-540)
            if self.init_shs is not None and self.init_shs.shape[0] == P:
                self.init_shs.copy_(self.shs), self.init_confidence.copy_(self.confidence)
            else:
                self.init_shs, self.init_confidence = self.shs.clone(), self.confidence.clone()
        snapshot = [b for b in _ROW_BUFFERS if b.group == "snapshot"]
        same = all(getattr(self, b.name) is not None and getattr(self, b.name).shape[0] == P for b in snapshot)
        for b in snapshot:
            src = mask if b.src is None else getattr(self, b.src)  # (attach_mask: the set found above)
            if same:
                getattr(self, b.name).copy_(src)
            else:
                setattr(self, b.name, src.to(torch.uint8) if b.src is None else src.clone())
        self.attach_partial.zero_()
        self._count_attach_set()
        self._attach_n = 0
        if reset_optimizer:
            for _, a in self._rows("moment"):
                a.zero_()
            self.step_count = 0
            self._step_dev.fill_(1)
            self._expected_step, self._unsettled = 1, False
        if not same:  # the captured kernel arguments (attach set buffers) were fixed at capture time
            for g in self._graphs():
                g.stale = True

    def _count_attach_set(self):
        self.attach_count = int(self.attach_mask.sum().item()) if self.use_attach else 0
        if self.use_attach and self.attach_count_reducer is not None:
            self.attach_count = int(self.attach_count_reducer(self.attach_count))
        n = self.attach_count
        # the two factors exactly as the library derives them from attach_count: double arithmetic, rounded to float once
        # (fill_ carries the python double as a kernel argument and rounds it to float once; a host tensor copied to the device would be
        # a synchronous pageable copy: ~1 ms per mapping call)
        self.attach_gains[0:1].fill_(2000.0 / (3.0 * n) if n > 0 else 0.0)
        self.attach_gains[1:2].fill_(2000.0 / (4.0 * n) if n > 0 else 0.0)

    def activate(self):
        """(opacity [P,1], scales [P,3], rotations [P,4]): the activations of the current raw parameters (SLAM/gaussian_pointcloud.py:
        732-733, 746-747), i.e. what the rasteriser sees in the next iteration — computed if they are not up to date.  The tensors are
        this mapper's own buffers: the next Adam step overwrites them."""
        if not self._act_valid:
            with torch.cuda.device(self.device):
                N.check(N.lib().dqo_map_activate(self.P, N.ptr(self.opacity_raw), N.ptr(self.scaling_raw), N.ptr(self.rotation_raw),
                                                 N.ptr(self.opacity), N.ptr(self.scales), N.ptr(self.rotations), N.current_stream()))
            self._act_valid = True
        return self.opacity, self.scales, self.rotations

    # ------------------------------------------------------------------ map growth ---------------------------------------
    def radius(self):
        """GaussianPointCloud.get_radius (SLAM/gaussian_pointcloud.py:739-743): mean of the two larger scales."""
        sc = torch.exp(self.scaling_raw)
        return (sc.sum(dim=1) - sc.min(dim=1).values) / 2

    def normals(self, rows=None):
        """GaussianPointCloud.get_normal (SLAM/gaussian_pointcloud.py:780-791): the column of R(q / |q|) along the smallest scale,
        normalised with the reference's + 1e-8 (utils/general_utils.py:108-137 build_rotation)."""
        q = self.rotation_raw if rows is None else self.rotation_raw[rows]
        sc = self.scaling_raw if rows is None else self.scaling_raw[rows]
        q = q / torch.sqrt((q * q).sum(1, keepdim=True))
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        cols = (torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
                torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
                torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1))
        k = torch.argmin(sc, dim=1)  # (exp is monotone: the smallest raw scale is the smallest scale)
        nrm = torch.where((k == 0)[:, None], cols[0], torch.where((k == 1)[:, None], cols[1], cols[2]))
        return nrm / (torch.sqrt((nrm * nrm).sum(1, keepdim=True)) + 1e-8)

    def _park_position(self):
        """Where spare rows sit: 10^4 units behind the camera of this mapper's settings — culled by the frustum test (p_view.z <= 0.2,
        forward.cu:258-262) like any Gaussian behind the camera, and far from every search box of the growth step."""
        V = self.settings.viewmatrix  # world_view_transform as the reference passes it: p_view = p @ V[:3, :3] + V[3, :3]
        return (self.settings.campos.reshape(3) - 1.0e4 * V[:3, 2]).to(torch.float32)

    # ------------------------------------------------------------------ the per-Gaussian buffers (_ROW_BUFFERS) ----------
    def _rows(self, *groups):
        """(declaration, tensor) of every per-Gaussian buffer of the given groups (none given: all of them) that exists now."""
        for b in _ROW_BUFFERS:
            if not groups or b.group in groups:
                a = self.state[b.of[0]][b.of[1]] if b.of else getattr(self, b.name)
                if a is not None:
                    yield b, a

    def _set_rows(self, b, a):
        if b.of:
            pair = list(self.state[b.of[0]])
            pair[b.of[1]] = a
            self.state[b.of[0]] = tuple(pair)
        else:
            setattr(self, b.name, a)

    def _spare_value(self, b):
        if b.spare == "park":
            return self._park_position()
        if b.spare == "unit_q":
            return mg.const_tensor([1.0, 0.0, 0.0, 0.0], self.device)
        return b.spare

    @staticmethod
    def _write_rows(a, rows, value):
        """a[rows] = value.  (index_fill_ carries a scalar as a kernel argument; `a[rows] = scalar` stages it through a host tensor: a
        blocking copy.)"""
        if torch.is_tensor(value):
            a[rows] = value
        else:
            a.index_fill_(0, rows, value)

    def _free_rows(self, rows):
        """In place: the Gaussians of `rows` leave the map.  Only what makes a row a spare row for the kernels is written (`freed` in
        _ROW_BUFFERS); the other buffers keep their bits until a Gaussian moves in or the next mapping call rewrites them."""
        for b, a in self._rows("param", "meta"):
            if b.freed:
                self._write_rows(a, rows, self._spare_value(b))

    def _fill_rows(self, rows, new):
        """In place: the Gaussians of `new` (buffer name -> their rows' values) move into `rows`.  What growth adds is rendered and trained by
        the next call (the unstable cloud, mapper.py:1438-1466) with confidence 0; moments and init_stat are the next mapping call's."""
        for b, a in self._rows("param", "meta"):
            self._write_rows(a, rows, new.get(b.name, b.live))

    def _compact_and_append(self, keep_old, new, carry_call):
        """Into new buffers: the old rows `keep_old` (indices; None = all) in order, then the Gaussians of `new`.  A new row holds what
        `new` gives for the buffer, or for the parameter the buffer is a snapshot of, and zeros elsewhere.  carry_call: the mapping call
        goes on, so moments and init_stat come along; else the moments are made empty and init_stat is left to begin_mapping_call, which
        would overwrite both (a third of the step's copies)."""
        n = new["xyz"].shape[0]
        for b, a in self._rows("param", "meta", *(("moment", "snapshot") if carry_call else ())):
            add = new.get(b.name, new.get(b.src))
            if add is None:
                add = torch.zeros((n,) + tuple(a.shape[1:]), dtype=a.dtype, device=self.device)
            self._set_rows(b, torch.cat([a if keep_old is None else a[keep_old], add]).contiguous())
        self.P = self.xyz.shape[0]
        if not carry_call:
            for b, a in self._rows("moment", "snapshot"):
                self._set_rows(b, None if b.group == "snapshot" else torch.zeros((self.P,) + tuple(a.shape[1:]), dtype=a.dtype, device=self.device))

    def _drop_graphs(self):
        self._g, self._frames, self._mixed = None, [], {}
        # update_poses: window frame -> the trajectory row its camera follows (set_frame(row=...)), and the target table built from the
        # bound rows (None: build it; every capture and every binding drops it, since the addresses can change)
        self._frame_rows, self._repose_table = {}, None

    def _row_count_changed(self):
        """After P changed: what is sized by P is made anew (the one place the activations and attach_partial are allocated), what holds
        for one P only and every captured graph (whose kernel arguments are the old buffers and their length) is dropped."""
        for b in _ROW_BUFFERS:
            if b.group == "dropped":
                setattr(self, b.name, None)
            elif b.group == "sized":
                make = torch.empty if b.spare is None else torch.zeros
                setattr(self, b.name, make(b.shape(self.P), dtype=torch.float32, device=self.device))
        self._attach_n, self._act_valid = 0, False
        self._drop_row_sized_operator_state()
        self._drop_graphs()
        if self._bank is not None:  # (the bank's keyframes do not depend on P: run_bank captures its graph again)
            self._bank.graph = None

    @torch.no_grad()
    def reserve(self, spare_rows):
        """Room for `spare_rows` more Gaussians in every per-Gaussian buffer, so that a growth step writes the new Gaussians into spare
        rows and turns deleted ones into spare rows IN PLACE: no re-allocation, and a captured graph (whose kernel arguments are these
        buffers and their length) stays valid across growth steps and mapping calls.  A spare row is parked behind the camera
        (_park_position) with the raw parameters of a tiny transparent Gaussian: the preprocess stage culls it, it gets no gradient, the
        sparse Adam never touches it, it is in no attach set — the map behaves as if the row did not exist, at the cost of the
        per-Gaussian kernels looking at it.  `alive` [P] uint8 tells the rows apart.  Call before capture()."""
        n = int(spare_rows)
        if n <= 0:
            return self
        self._ensure_alive()
        for b, a in self._rows("param", "moment", "snapshot", "meta"):
            fill = self._spare_value(b)
            tail = torch.empty((n,) + tuple(a.shape[1:]), dtype=a.dtype, device=self.device)
            tail[:] = fill.to(a.dtype) if torch.is_tensor(fill) else fill
            self._set_rows(b, torch.cat([a, tail]).contiguous())
        self._spare_rows = n
        self._n_spare = int(self.alive.numel() - int(self.alive.sum().item()))  # (host copy of the spare-row count: grow() keeps it up to date)
        self.P += n
        self._row_count_changed()
        return self

    def _ensure_alive(self):
        """From here on the mapper tells its rows apart: `alive` of a mapper that never reserve()d is all ones."""
        if self.alive is None:
            self.alive = torch.ones((self.P,), dtype=torch.uint8, device=self.device)

    @property
    def n_alive(self):
        return self.P if self.alive is None else int(self.alive.sum().item())

    def _refresh_spare_count(self):
        """maintain() frees rows on the device and reads nothing back: the host's spare-row count is re-read from `alive` by the next
        grow(), which synchronises anyway."""
        if self._n_spare_stale:
            self._n_spare, self._n_spare_stale = int(self.alive.numel() - int(self.alive.sum().item())), False

    # ------------------------------------------------------------------ the two clouds' rows (maintain(): map_operators.py) ----------
    @torch.no_grad()
    def track_lifecycle(self, stable_mask=None, tick=0, frame_id=None):
        """Start keeping what the reference keeps per Gaussian for its map maintenance: which cloud the row belongs to (`stable` uint8,
        1 = stable_pointcloud; stable_mask bool [P] or None = the whole map is unstable), `add_tick` (int32, `tick` for every Gaussian
        of the map now) and the two strike counters of error_gaussians_remove (int32, zero), and `frame_id` (int32, the frame a row was added at:
        GaussianPointCloud._frame_ids, SLAM/gaussian_pointcloud.py:52; `frame_id` for every Gaussian of the map now, None = `tick`).  Spare
        rows hold 0 in all five.  From here on reserve() and grow() carry them, maintain() rewrites the first four and leaves frame_id to
        its row (a row it frees keeps a stale one: nothing reads it while alive == 0, and grow() overwrites it), prune_floaters() reads
        frame_id.  A mapper that never calls this behaves as before."""
        dev, P = self.device, self.P
        live = torch.ones((P,), dtype=torch.bool, device=dev) if self.alive is None else self.alive.bool()
        stable = torch.zeros((P,), dtype=torch.bool, device=dev) if stable_mask is None else stable_mask.to(dev).bool().reshape(-1)
        if stable.numel() != P:
            raise RuntimeError("FusedMapper.track_lifecycle: stable_mask must have one entry per row")
        self.stable = (stable & live).to(torch.uint8)
        self.add_tick = live.to(torch.int32) * int(tick)
        self.frame_id = live.to(torch.int32) * int(tick if frame_id is None else frame_id)
        self.depth_error_counter = torch.zeros((P,), dtype=torch.int32, device=dev)
        self.color_error_counter = torch.zeros((P,), dtype=torch.int32, device=dev)
        self._lifecycle = {}
        return self

    def _require_lifecycle(self, who):
        if self.stable is None:
            raise RuntimeError(f"FusedMapper.{who}: this mapper does not track its Gaussians' lifecycle; call track_lifecycle() first")

    def stable_rows(self):
        """bool [P]: the rows of the reference's stable_pointcloud (alive & stable) — what set_training_rows and grow(stable_mask=...) take."""
        self._require_lifecycle("stable_rows")
        return (self.stable != 0) if self.alive is None else (self.stable != 0) & (self.alive != 0)

    @torch.no_grad()
    def grow(self, new, delete_mask=None, min_radius=0.001, max_radius=0.05, xyz_factor=(1.0, 1.0, 0.1), scale_factor=1.0,
             new_mapping_call=False, stable_mask=None, unstable_opacity_low=0.1, attach_async=True, tick=None, frame_id=None):
        """The map-growth step between two mapping calls — Mapping.gaussians_add (SLAM/multiprocess/mapper.py:249-254) and the
        deletion half of error_gaussians_remove (:1086-1096) — on this mapper's map.  `new`: dict(xyz [Q,3], scales [Q,3],
        rotations [Q,4], opacity [Q,1], shs [Q,M,3]; with an object gate also obj_id [Q]) of numpy arrays or GPU tensors.
          1. temp_points_filter (:1351-1380): new points that fall inside an existing Gaussian (one of their 3 nearest existing
             centres closer than 0.6 x its radius; dqo_knn3_query) are dropped;
          2. temp_to_optimize -> GaussianPointCloud.update_geometry (:1438-1442, gaussian_pointcloud.py:519-570): the survivors'
             scales come from the gaps to their 3 nearest neighbours among (survivors + existing points in their bounding box)
             (distCUDA2 = dqo_knn3), points whose neighbours' 3-sigma spheres already reach them are dropped;
          3. delete_mask [P] bool (optional): existing Gaussians to delete (the reference derives it from
             accumulate_gaussian_error's per-Gaussian depth error, cuda_utils._C);
          4. cat (:1466): the rest joins the map with zero Adam moments.
        stable_mask [P] bool GPU tensor (optional) is the reference's split into its two clouds — 1 = a Gaussian of `stable_pointcloud`,
        0 = of the unstable `pointcloud` — and switches on the two steps that need it:
          1'. the filter of step 1 looks at the UNSTABLE Gaussians only (:1356-1357, unstable_params);
          1b. temp_points_attach (:1384-1436): the survivors of step 1 that project onto a pixel whose strongest contributor in a render
             of the STABLE Gaussians alone exists and whose plane they lie within 0.5 x add_depth_thres of get opacity
             `unstable_opacity_low` — which makes them members of the next mapping call's attach set (opacity < 0.9).  The stable-only
             render is this mapper's map with the other Gaussians parked behind the camera (the index map is the stable cloud's, in
             map rows).
        With an object gate every decision judges a candidate against the Gaussians of its OWN object only (dqo_mapgrowth.*_per_object),
        so a shard — which holds whole objects — takes exactly the decisions the unsharded map takes for its objects.
        The result is stored in one of two ways (_store_in_place / _store_reallocating say what each means for captured graphs): in
        place when the map has reserve()d spare rows, new_mapping_call is set and the spare and deleted rows hold the new Gaussians;
        into re-allocated buffers otherwise.  new_mapping_call=True also starts the next mapping call (begin_mapping_call: fresh Adam,
        fresh init_stat, as the reference does after every growth step, mapper.py:533-548).  tick (a mapper that track_lifecycle()s): the
        new rows' add_tick — they join the unstable cloud with zero strike counters (temp_to_optimize, mapper.py:1438-1466); frame_id:
        their frame_id (temp_to_optimize(frame_id), :1451-1460; None = tick if given, else 0).  Returns the counts of each stage."""
        self._refresh_spare_count()
        c = self._grow_candidates(new)
        Q = c["xyz"].shape[0]
        stats = dict(candidates=int(Q), inside_existing=0, invalid_scale=0, added=0, deleted=0)
        exist = (self.xyz, self.radius())  # (spare rows sit 10^4 units away: outside every search box)
        keep = torch.ones((Q,), dtype=torch.bool, device=self.device)
        live_rows = None if self.alive is None else self.alive.bool()
        attach = self._start_attach(c, stable_mask, unstable_opacity_low, attach_async) if stable_mask is not None and Q > 0 else None
        if Q > 0:
            inside = self._inside_existing(c, exist, stable_mask, live_rows)
            if inside is not None:
                keep &= ~inside
                stats["inside_existing"] = int(inside.sum().item())
        idx = keep.nonzero().reshape(-1)
        c = {k: None if v is None else v[idx] for k, v in c.items()}
        scales = invalid = None
        if idx.numel() > 0:
            scales, invalid = self._init_scales(c, exist, live_rows, min_radius, max_radius)
        if attach is not None:  # (the join sits between the scale search and the reading of its result: the attach overlaps both searches)
            stats["attached"] = self._lower_attached(c, idx, attach.result(), Q, unstable_opacity_low)
        rows = self._new_rows(c, scales, invalid, scale_factor, xyz_factor, stats)
        stats["added"] = n_add = int(rows["xyz"].shape[0])
        if tick is not None and self.add_tick is not None:
            rows["add_tick"] = torch.full((n_add,), int(tick), dtype=torch.int32, device=self.device)
        if self.frame_id is not None:
            fid = frame_id if frame_id is not None else (tick if tick is not None else 0)
            rows["frame_id"] = torch.full((n_add,), int(fid), dtype=torch.int32, device=self.device)
        if self.alive is not None:
            # (the deleted rows as indices, found once: four boolean-mask writes were four passes over the map + four host round trips)
            if delete_mask is None:
                del_rows = torch.empty((0,), dtype=torch.long, device=self.device)
            else:
                del_rows = (delete_mask.to(self.device).bool().reshape(-1) & live_rows).nonzero().reshape(-1)
            stats["deleted"] = int(del_rows.numel())
            if new_mapping_call and n_add <= self._n_spare + stats["deleted"]:
                return self._store_in_place(rows, del_rows, stable_mask, stats)
            # spare rows exhausted (or the mapping call goes on): compact — spare rows go with the deleted ones — and reserve again
            delete_mask = ~live_rows
            delete_mask.index_fill_(0, del_rows, True)
            self.alive, self._n_spare = None, 0
            stats["in_place"] = False
        return self._store_reallocating(rows, delete_mask, new_mapping_call, stats)

    def _grow_candidates(self, new):
        """grow()'s `new` as GPU tensors; obj: the object ids the gate needs (`_obj_id`, gaussian_pointcloud.py:497; None without a gate)."""
        dev = self.device
        t = lambda a: a.to(dev).float().contiguous() if torch.is_tensor(a) else torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
        c = dict(xyz=t(new["xyz"]), scales=t(new["scales"]), rotations=t(new["rotations"]), opacity=t(new["opacity"]).reshape(-1, 1),
                 shs=t(new["shs"]), obj=None)
        if self.gaussian_object is not None:
            if new.get("obj_id") is None:
                raise RuntimeError("FusedMapper.grow: with an object gate the new points need 'obj_id'")
            c["obj"] = torch.as_tensor(new["obj_id"]).to(dev, torch.int32).reshape(-1)
        return c

    def _start_attach(self, c, stable_mask, unstable_opacity_low, attach_async):
        """temp_points_attach only changes opacities and judges every candidate by itself; the filter and update_geometry only read
        positions and radii: the attach runs beside BOTH, on ALL candidates (the ones the filter drops are dropped from its answer
        afterwards) — on a stream and a host thread of its own (both sides wait on the host for small results in between their
        kernels).  Started behind the filter, the step's critical path was filter + attach."""
        dev = self.device
        self.activate()
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=dev)
        side = self._side_stream
        side.wait_stream(torch.cuda.current_stream())

        def work(tx=c["xyz"], to=c["opacity"], tobj=c["obj"]):
            with torch.cuda.device(dev), torch.cuda.stream(side), torch.no_grad():
                return self._temp_points_attach(tx, to, stable_mask, unstable_opacity_low, temp_obj=tobj)

        return _SideJob(work, side, threaded=attach_async).start()

    def _inside_existing(self, c, exist, stable_mask, live_rows):
        """Step 1 / 1': bool [Q], the candidates inside an existing Gaussian — of the unstable cloud when the clouds are told apart, of
        their own object with an object gate."""
        exist_xyz, exist_radius = exist
        if stable_mask is None and c["obj"] is None:
            return mg.temp_points_filter_mask(c["xyz"], exist_xyz, exist_radius)
        if stable_mask is None:
            un = torch.ones((self.P,), dtype=torch.bool, device=self.device)
        else:  # the reference filters against its unstable cloud
            un = ~stable_mask.to(self.device).bool().reshape(-1)
        if live_rows is not None:
            un = un & live_rows  # (spare rows are no Gaussians of the map)
        un = un.nonzero().reshape(-1)  # (the unstable cloud is small: a few thousand rows of a 2 M map)
        if c["obj"] is not None:
            return mg.temp_points_filter_mask_per_object(c["xyz"], c["obj"], exist_xyz[un], exist_radius[un], self.gaussian_object[un],
                                                         cell=self.object_cell)
        return mg.temp_points_filter_mask(c["xyz"], exist_xyz[un], exist_radius[un])

    def _init_scales(self, c, exist, live_rows, min_radius, max_radius):
        """Step 2: (scales [n], invalid [n] bool) of the filter's survivors, both still on the device."""
        nsc = c["scales"]
        nrad = (nsc.sum(dim=1) - nsc.min(dim=1).values) / 2
        if c["obj"] is None:
            return mg.update_geometry_scales(c["xyz"], nrad, exist[0], exist[1], min_radius, max_radius)
        gobj_live = self.gaussian_object if live_rows is None else torch.where(live_rows, self.gaussian_object, -1)
        return mg.update_geometry_scales_per_object(c["xyz"], c["obj"], nrad, exist[0], exist[1], gobj_live, min_radius, max_radius,
                                                    cell=self.object_cell)

    def _lower_attached(self, c, idx, attached, Q, unstable_opacity_low):
        """Step 1b's answer (indices among all Q candidates) on the filter's survivors `idx`: their opacity is lowered; returns their number."""
        att_all = torch.zeros((Q,), dtype=torch.bool, device=self.device)
        att_all.index_fill_(0, attached, True)
        att = att_all[idx].nonzero().reshape(-1)
        c["opacity"] = c["opacity"].clone()
        c["opacity"].index_fill_(0, att, unstable_opacity_low)
        return int(att.numel())

    def _new_rows(self, c, scales, invalid, scale_factor, xyz_factor, stats):
        """The survivors with a valid scale as rows of the map: per-Gaussian buffer name -> values (gaussian_pointcloud.py:558-568 for
        the scales), plus `activated_opacity`, from which a mapping call that goes on takes their attach membership."""
        dev = self.device
        ok = torch.empty((0,), dtype=torch.long, device=dev)
        log_scales = torch.empty((0, 3), dtype=torch.float32, device=dev)
        if invalid is not None:
            stats["invalid_scale"] = int(invalid.sum().item())
            ok = (~invalid).nonzero().reshape(-1)
            if ok.numel() > 0:
                fac = scale_factor * scales[:, None].repeat(1, 3) * mg.const_tensor(xyz_factor, dev)
                log_scales = torch.log(fac)[ok]
        opacity = c["opacity"][ok]
        opc = opacity.clamp(1e-4, 1 - 1e-4)
        return dict(xyz=c["xyz"][ok], shs=c["shs"][ok], opacity_raw=torch.log(opc / (1 - opc)), scaling_raw=log_scales,
                    rotation_raw=c["rotations"][ok], gaussian_object=None if c["obj"] is None else c["obj"][ok], activated_opacity=opacity)

    def _store_in_place(self, new, del_rows, stable_mask, stats):
        """Deleted Gaussians become spare rows, the new ones take spare rows, lowest index first (row order then differs from the
        reference's cat; nothing depends on it), and the next mapping call starts — all rewritten in place: no buffer moves, P stays,
        and a captured graph stays valid.  stable_mask is cleared IN PLACE on the rows the new Gaussians take."""
        n_del, n_add = int(del_rows.numel()), int(new["xyz"].shape[0])
        if n_del:
            self._free_rows(del_rows)
        self._n_spare += n_del - n_add
        if n_add:
            rows = (self.alive == 0).nonzero().reshape(-1)[:n_add]
            self._fill_rows(rows, new)
            stats["rows"] = rows
            if stable_mask is not None:
                # what growth adds belongs to the UNSTABLE cloud (mapper.py:1438-1466) — also when it lands in a row a deleted stable
                # Gaussian just freed: the caller's mask is updated in place, so the next step's filter / stable-only render see the
                # row as unstable
                stable_mask.index_fill_(0, rows, False)
        # (a captured iteration starts from the activations its previous Adam launch left: bring them up to date for the new rows)
        self._act_valid = False
        self.activate()
        self.begin_mapping_call(reset_optimizer=True)  # in place too: fresh moments, fresh init_stat, the new attach set
        stats["in_place"] = True
        return stats

    def _store_reallocating(self, new, delete_mask, new_mapping_call, stats):
        """Every per-Gaussian buffer is re-allocated as cat(kept old rows, new rows) — the reference's row order — and P changes: every
        captured graph is dropped (capture() again).  The mapping call goes on with its moments, init_stat and attach set carried for the
        kept rows (the new ones start at their own values: they have not moved), or — new_mapping_call — the next one starts.  A map
        that had spare rows and ran out of them (stats["in_place"] is False) gets the same number again."""
        keep_old = None
        if delete_mask is not None:
            keep_old = (~delete_mask.to(self.device).bool().reshape(-1)).nonzero().reshape(-1)
            if "in_place" not in stats:  # (with spare rows "deleted" counts Gaussians, and the spare rows leave with them)
                stats["deleted"] = int(self.P - keep_old.numel())
        stats["kept_rows"] = keep_old  # (None = all of them, in place) the old rows that now lead the map, for per-row data of the caller's
        if not new_mapping_call:
            new["attach_mask"] = (new["activated_opacity"].reshape(-1) < 0.9).to(torch.uint8)
        self._compact_and_append(keep_old, new, carry_call=not new_mapping_call)
        self._row_count_changed()
        if new_mapping_call:
            self.begin_mapping_call(reset_optimizer=True)
        else:
            self._count_attach_set()
        if stats.get("in_place") is False:
            self.reserve(self._spare_rows)
        return stats

    def _temp_points_attach(self, temp_xyz, temp_opacity, stable_mask, unstable_opacity_low, temp_obj=None):
        """mapper.py:1384-1436 on this mapper's map: indices (into the temp points) that fall onto the stable cloud's surfaces.
        temp_obj (the per-object job): the stable cloud is rendered through the object gate — every pixel shows its owner object's
        stable Gaussians, exactly what a shard that owns the object renders there — and a candidate only attaches to a stable Gaussian of
        its own object; the zero fill of never-rendered tiles counts as no hit (the reference's alias of such a pixel to "Gaussian 0"
        would name a different Gaussian on every shard layout)."""
        st, dev = self.settings, self.device
        sm = stable_mask.to(dev).bool().reshape(-1)
        if self.alive is not None:
            sm = sm & self.alive.bool()
        self.activate()
        # the stable cloud alone = the map with every other Gaussian parked behind the camera (culled before the binning, so the tile
        # lists are the stable cloud's), indices in map rows.  One quirk to carry over: a tile that renders nothing keeps the op's
        # zero fill, which the reference's `>= 0` test reads as a hit on Gaussian 0 OF THE STABLE CLOUD (F3 / rasterize_points.cu:79-89)
        # — here that is the first stable row, and such a pixel is told from a real hit on row 0 by its zero weight.
        gated = temp_obj is not None and self.gaussian_object is not None
        if not gated:
            if not bool(sm.any()):
                return torch.empty((0,), dtype=torch.long, device=dev)
            first = torch.argmax(sm.to(torch.uint8)).reshape(1)  # (the first stable row)
        data = dict(xyz=torch.where(sm[:, None], self.xyz, self._park_position()[None, :]), opacity=self.opacity, scales=self.scales,
                    rotations=self.rotations, shs=self.shs)
        H, W = int(st.image_height), int(st.image_width)
        K = mg.const_tensor([[W / (2.0 * st.tanfovx), 0.0, st.cx], [0.0, H / (2.0 * st.tanfovy), st.cy], [0.0, 0.0, 1.0]], dev)
        if gated:
            # Only the candidates' own pixels are ever looked at (one pixel in twenty of a frame): the render goes through the object
            # gate with every OTHER pixel ownerless — such a pixel starts finished, an entry that reaches no owned pixel of a quadrant is
            # dropped by the quadrant's owner set, a (Gaussian, tile) pair whose object owns no candidate pixel of the tile is dropped by
            # the binning, a quadrant without a candidate ends at once; the owned pixels blend exactly what the full-frame gated
            # render blends for them (pixels are independent).  Two launches around the render (csrc/map_attach.hip) instead of the
            # reference's chain of boolean-index ops: the growth step is bound by the host's op issue rate.
            lin, sparse, tile_sets = mg.attach_pixels(temp_xyz, st.viewmatrix, W / (2.0 * st.tanfovx), H / (2.0 * st.tanfovy), st.cx, st.cy,
                                                      W, H, self.pixel_object)
            dgr.gate_ids_checked(sparse)  # (values of pixel_object, which has been checked, or -1)
            out = mapping.render(st, data, object_gate=(self.gaussian_object, sparse, tile_sets))
            ok = mg.attach_decide(temp_xyz, temp_opacity, temp_obj, lin, out["color_index_map"], out["color_hit_weight"], self.xyz,
                                  self.scaling_raw, self.rotation_raw, self.gaussian_object, self.add_depth_thres, unstable_opacity_low)
            return ok.nonzero().reshape(-1)
        out = mapping.render(st, data, object_gate=None)
        cim = out["color_index_map"]
        zero_fill = (cim == 0) & (out["color_hit_weight"] == 0)
        cim = torch.where(zero_fill, first.to(cim.dtype).reshape(1, 1, 1), cim)
        return mg.temp_points_attach_indices(temp_xyz, temp_opacity, st.viewmatrix.T.contiguous(), K, W, H, cim, self.xyz,
                                             lambda rows: self.normals(rows), self.add_depth_thres, unstable_opacity_low)

    def attach_loss(self):
        """The reference's reported "scale_loss" of the most recent iteration (attach loss at its pre-update parameters)."""
        return self.attach_partial[:self._attach_n].sum()

    def _attach_fields(self):
        if not self.use_attach:
            return dict(attach_mask=None, init_xyz=None, init_scaling_raw=None, init_rotation_raw=None, attach_count=0, attach_partial=None)
        # (attach_gains: the set's size is read from device memory when the launch runs — an empty set costs the mask read)
        return dict(attach_mask=N.ptr(self.attach_mask), init_xyz=N.ptr(self.init_xyz), init_scaling_raw=N.ptr(self.init_scaling),
                    init_rotation_raw=N.ptr(self.init_rotation), attach_count=self.attach_count, attach_partial=N.ptr(self.attach_partial),
                    attach_gains=N.ptr(self.attach_gains))

    @staticmethod
    def pick_list_split_pair(list_split, tile_mask, st, longest=0):
        """(forward, backward) values of DqoRastCtx.list_split for a capture: an int for both kernels, a pair (f, b) as given (b must be
        0 or f: the backward walks the forward's queue), or "auto" by the number of tiles the frame renders and the longest list of the
        state the capture is taken on.  Four waves per tile fill the 1024 SIMDs six deep at 1500 tiles; below that the blend kernels'
        time is the time of their longest lists, and the fewer tiles there are, the shorter the lists worth sharing between eight waves
        (measured on the shards of configs 4 and 5).  The eight-wave blocks cost the short lists occupancy (config 3's
        shards, whose lists all stay below 600 entries, lose 10 %), so a split is only taken when some list is long enough to be a tail
        worth cutting; and the fuller the GPU, the less the BACKWARD gains — it has no early exit, so its tail is the whole list's
        work, not a handful of quadrants' — so frames of more than 1300 tiles share lists in the forward only (config 5: half the
        frame 1.12 -> 0.96 ms, the full frame 1.69 -> 1.66 ms)."""
        if isinstance(list_split, (tuple, list)):
            f, b = int(list_split[0]), int(list_split[1])
            if f < 0 or b not in (0, f):
                raise ValueError("list_split pair: (forward threshold, 0 or the same threshold)")
            return f, b
        if list_split != "auto":
            if int(list_split) < 0:
                raise ValueError("list_split is 0 (off), a list length, a pair or 'auto'")
            return int(list_split), int(list_split)
        tiles = int((tile_mask != 0).sum().item()) if tile_mask is not None else ((st.image_width + 15) // 16) * ((st.image_height + 15) // 16)
        if tiles <= 1300:
            t = 256 if tiles <= 500 else 512 if tiles <= 800 else 1024
            return (t, t) if longest >= 1024 else (0, 0)
        if tiles <= 2600:
            return (1024, 0) if longest >= 2048 else (0, 0)
        return (2048, 0) if longest >= 4096 else (0, 0)

    @staticmethod
    def pick_list_split(list_split, tile_mask, st, longest=0):
        """The threshold BOTH blend kernels share under pick_list_split_pair's rule (0 when only the forward splits)."""
        return FusedMapper.pick_list_split_pair(list_split, tile_mask, st, longest)[1]

    # ------------------------------------------------------------------ hipGraph path ------------------------------------
    def capture(self, gt_color, gt_depth, render_mask, tile_mask=None, capacity_margin=1.15, tile_buckets=True, keep_tile_order=True,
                loss_tap=True, reuse_probe=False, fused_tail=True, list_split=0, unroll=1, settings=None, pixel_object=None, frame=None,
                run_unroll=1,
                short_bucket_margin=1.3, head=None):
        """Allocate persistent buffers for every intermediate of an iteration, run it once eagerly, then capture it into a
        hipGraph.  The inputs (gt images, masks) are read from the tensors passed here at every replay().

        settings / pixel_object / frame (round 6, the frame set of a mapping call — capture_window drives them): the camera of THIS
        graph (default: the mapper's), its pixel -> owner map when the object gate is on (default: set_object_gate's), and the slot of
        the window it fills (None = a single-frame mapper: the graph replaces whatever was captured before).  Every graph has its own
        camera tensors (copies: set_frame rewrites them), context buffers, capacities and outputs; parameters, moments, activations, the device-side step count, the row flags, the
        confidence counter and the learning-rate table are the mapper's and shared.

        The capture fixes two capacities from the state it is taken on: the instance capacity (candidates x capacity_margin)
        and, with tile_buckets, the per-tile list bucket (twice the longest list, power of two).  A replay that outgrows
        either leaves invalid outputs and raises the device-side overflow flag — check graph_overflowed() (one small D2H read,
        e.g. once per batch of replays) and call capture() again when it is set, or use run(), which does both; tile_buckets=False
        keeps the packed lists (any list length, two more kernels per iteration).

        keep_tile_order (bucket mode): the replays keep the tile launch order of the capture's eager iteration instead of
        recomputing it (DqoRastCtx.keep_tile_order: no scan kernel in a replay).  loss_tap: the masked loss is summed inside the
        forward's blend kernel and its gradient is formed inside the backward's (DqoRastCtx.loss_tap: no loss kernels; self.loss is
        written by the backward).  fused_tail: the per-Gaussian half of the backward and the Adam step run as ONE kernel
        (dqo_rast_backward_adam: record sum -> per-Gaussian chain -> Adam per block of 256 Gaussians, gradient rows in LDS) instead of
        two (gradient rows through HBM).  All three leave every parameter and moment bit for bit as it is without
        them.  reuse_probe: size the capacities from
        the previous capture's counts (scaled by the map's growth) instead of a probing forward — for a re-capture right after a small
        change of the map; falls back to probing if the eager iteration overflows.  unroll: iterations per graph — replay() then runs
        `unroll` iterations with one launch call (back-to-back graph launches leave the GPU idle for ~9 us each on MI355X; the
        iterations inside one graph follow each other without a gap); self._g.out / self.loss then show the last of them.
        head (capture_bank drives it, with frame="bank"): the keyframe bank whose select launch every iteration issues first — it moves
        the scheduled keyframe into this graph's input buffers — and whose probe() sizes the capacities over all its keyframes; None,
        the default: no such launch."""
        dev = self.device
        self._repose_table = None  # (update_poses' targets are the graphs' camera tensors: this capture makes new ones)
        st = self._settings_or_own(settings)
        # (the graph's own copies: set_frame rewrites them in place)
        st = st._replace(bg=st.bg.clone(), viewmatrix=st.viewmatrix.clone(), projmatrix=st.projmatrix.clone(), campos=st.campos.clone())
        H, W = int(st.image_height), int(st.image_width)
        if (H, W) != (int(self.settings.image_height), int(self.settings.image_width)):
            raise RuntimeError("FusedMapper.capture: every frame of a mapper has the mapper's image size")
        tile_mask = self.tile_mask if tile_mask is None else _checked_tile_mask(tile_mask, dev, H, W)
        pix_obj, tile_obj = self.pixel_object, self.tile_objects
        if pixel_object is not None:
            if self.gaussian_object is None:
                raise RuntimeError("FusedMapper.capture: a per-frame pixel_object needs set_object_gate first")
            pix_obj = torch.as_tensor(pixel_object).to(dev, torch.int32).contiguous().reshape(H, W)
            tile_obj = tile_object_sets(pix_obj)
        for name, t_, shape in (("gt_color", gt_color, (3, H, W)), ("gt_depth", gt_depth, (1, H, W))):
            if t_.dtype != torch.float32 or not t_.is_cuda or not t_.is_contiguous() or tuple(t_.shape) != shape:
                raise RuntimeError(f"FusedMapper.capture: {name} must be a contiguous float32 GPU tensor of shape {shape} "
                                   "(the graph reads it in place at every replay)")
        mask = None if render_mask is None else render_mask.to(torch.uint8).contiguous()
        g = _FrameGraph(frame, st, pix_obj, tile_obj, gt_color, gt_depth, mask, tile_mask,
                        dict(tile_buckets=tile_buckets, keep_tile_order=keep_tile_order, loss_tap=loss_tap, fused_tail=fused_tail,
                             list_split=list_split, unroll=unroll, run_unroll=run_unroll, short_bucket_margin=short_bucket_margin,
                             head=head))
        with torch.cuda.device(dev):
            # re-capture (e.g. after an overflow): replays of invalid frames did not advance the device-side step count
            # (DqoAdamStep.frame_header), the host count assumed they did — _settle_replays takes exactly those back; eager step()
            # calls since then advanced the host count alone (they never touch the device count) and stay counted
            self._settle_replays()
            if frame is None:
                self._drop_graphs()
            self.activate()
            reuse_probe, longest = self._size_graph(g, capacity_margin, reuse_probe)
            self._g = g
            if isinstance(frame, tuple):  # (camera / target of frame k, masks of frame m): global_optimization's second half
                self._mixed[frame] = g
            elif frame == "bank":
                self._bank.graph = g
            elif frame is not None:
                while len(self._frames) <= frame:
                    self._frames.append(None)
                self._frames[frame] = g
            self._allocate_graph(g)
            self._build_graph_structs(g, longest)
            if not self._warm_up_and_record(g, reuse_probe):  # the reused counts were too small after all: measure and start over
                self._last_probe = None
                return self._recapture(g, capacity_margin)
        return self

    def _recapture(self, g, capacity_margin):
        """capture() again for graph g on the current state, with a new capacity margin: its live inputs (set_frame may have rewritten
        them), its camera, its window slot and the options it was captured with."""
        own_pixel_object = self.gaussian_object is not None and g.pixel_object is not self.pixel_object
        return self.capture(g.gt_color, g.gt_depth, g.mask, tile_mask=g.tile_mask, capacity_margin=capacity_margin, settings=g.settings,
                            pixel_object=g.pixel_object if own_pixel_object else None, frame=g.frame, **g.options)

    def _size_graph(self, g, capacity_margin, reuse_probe):
        """The capacities of a new graph (g.cap, g.bucket).  Returns (whether the previous capture's counts were reused, the longest
        tile list they assume)."""
        # capacity: the reference's num_rendered of the current state (an upper bound of the instances kept) plus a margin
        # for the Gaussians that move while the graph is being replayed; the device header flags an overflow.  The probe runs
        # through the C ABI on buffers of its own (two header reads), so the operator's global state is not touched.
        # (reuse_probe: the counts of the previous capture, scaled by the growth of the map since — for a re-capture right after a
        # growth step, which changes the map by a fraction of a percent; if the eager iteration overflows, the capture
        # is redone with a real probe)
        P, last = self.P, self._last_probe
        if reuse_probe and last is not None and last[2] > 0:
            grown = max(1.0, P / last[2])
            cand, longest = int(last[0] * grown) + 1, int(last[1] * grown) + 1
        else:
            reuse_probe = False
            if g.head is not None:  # (the one graph of a keyframe bank serves every keyframe: the largest of their counts)
                cand, longest = g.head.probe(self)
            else:
                cand, longest = self._probe(g.tile_mask, g.settings, g.pixel_object, g.tile_objects)
        self._last_probe = (cand, longest, P)
        g.cap = capacity_for(cand, capacity_margin)
        # fixed per-tile list buckets (bucket_for; short_bucket_margin: how much margin over the longest list is worth keeping the
        # long-list sort launch away, 6 us on a map whose lists are all short).  A tile that outgrows its bucket flags the frame
        # (graph_overflowed(); run() / run_window() re-capture; the replays in between train nothing).
        if g.options["tile_buckets"]:
            g.bucket = bucket_for(longest, float(g.options["short_bucket_margin"]))
        return reuse_probe, longest

    def _allocate_graph(self, g):
        """The persistent buffers of a new graph: outputs, context buffers, the backward's workspace and gradient rows."""
        lib, dev, P, M = N.lib(), self.device, self.P, self.M
        f = dict(dtype=torch.float32, device=dev)
        g.ctx = c = _RenderContext(P, int(g.settings.image_width), int(g.settings.image_height), dev).size(g.cap, g.bucket)
        g.out, g.outputs, g.geom, g.img, g.binning = c.out, c.outputs, c.geom, c.img, c.binning
        g.ws = torch.empty((lib.dqo_rast_backward_workspace_bytes(g.cap),), dtype=torch.uint8, device=dev)
        # dL_dcolors / dL_dcov3D / dL_dmeans2D have no consumer in the mapping step: NULL = the backward does not store them
        g.grads = dict(means3D=torch.empty((P, 3), **f), sh=torch.empty((P, M, 3), **f),
                       opacity=torch.empty((P, 1), **f), scales=torch.empty((P, 3), **f), rot=torch.empty((P, 4), **f))
        g.step_dev, g.ticket, g.bias = self._step_dev, self._ticket, self._bias

    def _build_graph_structs(self, g, longest):
        """The C structs of a new graph's iteration over its buffers (their addresses are kernel arguments of the graph)."""
        st, opt = g.settings, g.options
        g.fused_tail = bool(opt["fused_tail"]) and self.M <= 16
        g.params = dgr._params(st, self.P, self.M)
        g.inputs = dgr._inputs(st, self.xyz, self.shs, self._empty, self.opacity, self.scales, self.rotations, self._empty, g.tile_mask,
                               row_flags=self.row_flags)
        # (DqoRastCtx.list_split is read by the forward and by the backward call: _static_iteration sets it before each)
        g.ls_fwd, g.ls_bwd = self.pick_list_split_pair(opt["list_split"], g.tile_mask, st, longest)
        g.cctx = g.ctx.cctx(list_split=g.ls_fwd)
        # DqoLossTap: the masked loss is summed by the forward's blend kernel and its gradient images are formed inside the
        # backward's (bit for bit what dqo_map_loss_fwd_bwd computes): no loss kernels, no passes over the full image.
        # The SSIM term's gradient (no render mask) is an image (an 11 x 11 window around every pixel): the tap, which forms
        # sign(error) x weight inside the backward's blend kernel, cannot carry it -> loss kernels + gradient images (three more
        # launches + the SSIM's three)
        loss_tap = opt["loss_tap"] and not (g.mask is None and self.ssim_weight != 0)
        if loss_tap:
            g.grad_scale = torch.zeros((2,), dtype=torch.float32, device=self.device)
            g.tap = N.DqoLossTap(gt_color=N.ptr(g.gt_color), gt_depth=N.ptr(g.gt_depth), render_mask=N.ptr(g.mask),
                                 out_color=g.out[0].data_ptr(), out_depth=g.out[1].data_ptr(), color_weight=self.color_weight,
                                 depth_weight=self.depth_weight, add_depth_thres=self.add_depth_thres, loss_out=N.ptr(self.loss),
                                 grad_scale=g.grad_scale.data_ptr(),
                                 per_object=1 if (self.per_object_loss and self.gaussian_object is not None) else 0)
            g.cctx.loss_tap = ctypes.addressof(g.tap)
        if self.gaussian_object is not None:
            g.gate = N.DqoObjectGate(gaussian_object=N.ptr(self.gaussian_object), pixel_object=N.ptr(g.pixel_object),
                                     tile_objects=N.ptr(g.tile_objects))
            g.cctx.object_gate = ctypes.addressof(g.gate)
            if self.per_object_loss and not loss_tap:
                raise RuntimeError("FusedMapper.capture: the per-object loss is computed by the loss tap (loss_tap=True)")
        gr = [g.grads[k].data_ptr() for k in ("means3D", "sh", "opacity", "scales", "rot")]
        g.cgrads = N.DqoRastGrads(dL_dmeans3D=gr[0], dL_dsh=gr[1], dL_dcolors=None, dL_dopacity=gr[2], dL_dscales=gr[3],
                                  dL_drotations=gr[4], dL_dcov3D=None, dL_dmeans2D=None, skip_culled_rows=1)
        g.adam = self._adam_step_args(gr, radii=g.out[8].data_ptr(), frame_header=g.geom.data_ptr(), step_dev=g.step_dev)
        # the three-kernel form (fused_tail=False) lists Adam's rows by the backward's record marks, like the fused tail (DqoAdamStep.record_ctx)
        g.adam.record_ctx = ctypes.addressof(g.cctx)
        g.adam.record_W, g.adam.record_H = int(st.image_width), int(st.image_height)

    def _warm_up_and_record(self, g, reuse_probe):
        """One eager iteration of graph g (warms every kernel up), then the capture of its graphs.  Returns False, recording nothing, if
        the iteration overflowed capacities sized on reused counts."""
        self._step_dev.fill_(self.step_count + 1)
        self._expected_step = self.step_count + 1
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._static_iteration()
        torch.cuda.current_stream().wait_stream(side)
        if not self.graph_overflowed():  # (an invalid frame is a no-op for the optimiser and its step count)
            self.step_count += 1
        elif reuse_probe:
            return False
        # the eager iteration left its tile launch order in g.img; the replays keep it (DqoRastCtx.keep_tile_order: the order is
        # a scheduling hint, and the lists of one camera change little between the iterations of a mapping call)
        g.cctx.keep_tile_order = 1 if (g.bucket > 0 and g.options["keep_tile_order"]) else 0
        # ... and start from the counters the previous iteration's per-Gaussian kernel cleared (DqoRastCtx.frame_prezeroed: no
        # zero-fill launch in a replay; only dqo_rast_backward_adam clears them, so only with the fused tail)
        g.cctx.frame_prezeroed = 1 if g.fused_tail else 0
        g.graph = torch.cuda.CUDAGraph()
        # thread_local: other threads of the process (e.g. a collective library's watchdog) may keep issuing runtime calls
        g.unroll = max(1, int(g.options["unroll"]))
        with torch.cuda.graph(g.graph, capture_error_mode="thread_local"):
            # (everything a caller can see after a launch is what the LAST iteration left: the ones before it run lean)
            for i in range(g.unroll):
                self._static_iteration(lean=i + 1 < g.unroll)
        # run_unroll (capture_window): a SECOND graph over the same context buffers with that many iterations, for the stretches of a
        # schedule that stay on one frame — the second half of local_optimize renders the newest frame only (mapper.py:574-576) —
        # where one launch per iteration leaves the GPU idle for ~9 us between graphs (replay_run)
        g.run_unroll = max(1, int(g.options["run_unroll"]))
        if g.run_unroll > 1:
            g.run_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g.run_graph, capture_error_mode="thread_local"):
                for i in range(g.run_unroll):
                    self._static_iteration(lean=i + 1 < g.run_unroll)
        self._expected_step = self.step_count + 1
        return True

    def _adam_step_args(self, grads, radii, frame_header, step=0, step_dev=None):
        """The DqoAdamStep of one iteration over this mapper's parameters, moments and activations.  grads: the five gradient-row
        pointers (means3D, sh, opacity, scales, rotations).  step_dev (the captured path): the device-side step count, with the
        block ticket and bias table when use_block_ticket is on and the learning rates from lr_table; without it (eager step()) the
        launch takes `step` and the learning rates as arguments."""
        stt, ticket = self.state, step_dev is not None and self.use_block_ticket
        return N.DqoAdamStep(P=self.P, M=self.M, step=step, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, lr_xyz=self.lrs["xyz"],
                             lr_f_dc=self.lrs["f_dc"], lr_f_rest=self.lrs["f_rest"], lr_opacity=self.lrs["opacity"],
                             lr_scaling=self.lrs["scaling"], lr_rotation=self.lrs["rotation"], xyz=N.ptr(self.xyz), shs=N.ptr(self.shs),
                             opacity_raw=N.ptr(self.opacity_raw), scaling_raw=N.ptr(self.scaling_raw),
                             rotation_raw=N.ptr(self.rotation_raw), g_means3D=grads[0], g_sh=grads[1], g_opacity=grads[2],
                             g_scales=grads[3], g_rotations=grads[4], m_xyz=N.ptr(stt["xyz"][0]), m_shs=N.ptr(stt["shs"][0]),
                             m_opacity=N.ptr(stt["opacity"][0]), m_scaling=N.ptr(stt["scaling"][0]), m_rotation=N.ptr(stt["rotation"][0]),
                             v_xyz=N.ptr(stt["xyz"][1]), v_shs=N.ptr(stt["shs"][1]), v_opacity=N.ptr(stt["opacity"][1]),
                             v_scaling=N.ptr(stt["scaling"][1]), v_rotation=N.ptr(stt["rotation"][1]), act_opacity=N.ptr(self.opacity),
                             act_scales=N.ptr(self.scales), act_rotations=N.ptr(self.rotations), radii=radii, step_dev=N.ptr(step_dev),
                             moment_live=N.ptr(self.moment_live), frame_header=frame_header,
                             block_ticket=N.ptr(self._ticket) if ticket else None, bias_table=N.ptr(self._bias) if ticket else None,
                             row_flags=N.ptr(self.row_flags), confidence=N.ptr(self.confidence) if self.count_confidence else None,
                             lr_table=N.ptr(self.lr_table) if step_dev is not None else None, **self._attach_fields())

    # ------------------------------------------------------------------ the frame set of a mapping call -----------------
    def _trained_state(self):
        return [a for _, a in self._rows("param", "moment")] + [self.confidence] + [a for b, a in self._rows("meta") if b.name in _LIFECYCLE_ROWS]

    def _snapshot_state(self):
        return dict(rows=[a.clone() for a in self._trained_state()], step=self.step_count)

    def _restore_state(self, snap):
        self._settle_replays()
        for a, old in zip(self._trained_state(), snap["rows"]):
            a.copy_(old)
        self.step_count = snap["step"]
        self._step_dev.fill_(self.step_count + 1)
        self._expected_step, self._unsettled = self.step_count + 1, False
        self._bias.zero_()
        self._act_valid = False
        self.activate()

    def capture_window(self, frames, **kw):
        """One captured graph per frame of a mapping call's frame set — the five `processed_frames` of local_optimize (mapper.py:549-555)
        or the selected keyframes of global_optimization (:1159-1180).  frames: list of dict(gt_color, gt_depth, render_mask=None,
        tile_mask=None, settings=None, pixel_object=None, row=None); row: the trajectory row the frame's camera follows under
        update_poses (set_frame's argument); kw: capture()'s other arguments.  Each graph owns its context buffers and
        capacities (a frame's tail clears ITS counters for ITS next replay: DqoRastCtx.frame_prezeroed holds per frame); they share the
        map, the optimiser state and the device step count, so replay(k) in any order is the reference's loop with its per-iteration
        frame choice = one graph launch.  The eager iterations the captures run are undone (parameters, moments, confidence, step
        count are put back): the mapping call starts from the state it was given."""
        snap = self._snapshot_state()
        self._settle_replays()
        self._drop_graphs()
        self._window_kw, self._window_frames = dict(kw), list(frames)
        for k, fr in enumerate(frames):
            if k:
                self._restore_state(snap)  # every frame is sized on the call's initial state
            self.capture(fr["gt_color"], fr["gt_depth"], fr.get("render_mask"), tile_mask=fr.get("tile_mask"), settings=fr.get("settings"),
                         pixel_object=fr.get("pixel_object"), frame=k, **kw)
            torch.cuda.synchronize()
        self._restore_state(snap)
        for k, fr in enumerate(frames):
            if fr.get("row") is not None:
                self._bind_row(self._frame_rows, k, fr["row"])
        return self

    def _bind_row(self, table, key, row):
        """update_poses' binding of a window frame / bank slot to a trajectory row (row < 0: unbound)."""
        row = int(row)
        if row < 0:
            if isinstance(table, dict):
                table.pop(key, None)
            else:
                table[key] = None
        else:
            table[key] = row
        self._repose_table = None

    def _repose_targets(self):
        """update_poses' target table from the bound rows: int64 [T,6] on the device (DqoReposeTarget: row, c2w,
        w2c, viewmatrix, projmatrix, campos), one entry per graph that renders a bound window frame's camera (its own settings tensors)
        and one per bound bank slot (its camera row: viewmatrix at float 3, projmatrix at 19, campos at 35 of the 40).  Built once and
        kept until a binding changes or a graph is captured again."""
        if self._repose_table is None:
            entries, held = [], []
            for k, row in sorted(self._frame_rows.items()):
                graphs = ([self._frames[k]] if k < len(self._frames) and self._frames[k] is not None else []) + \
                         [g for (a, b), g in self._mixed.items() if a == k]
                for g in graphs:
                    st = g.settings
                    for name in ("viewmatrix", "projmatrix", "campos"):
                        if getattr(st, name).data_ptr() == getattr(self.settings, name).data_ptr():
                            raise ValueError(f"FusedMapper.update_poses: frame {k}'s {name} is the mapper's default camera tensor; "
                                             "a correction would move every default-camera render with it")
                    entries.append((row, 0, 0, st.viewmatrix.data_ptr(), st.projmatrix.data_ptr(), st.campos.data_ptr()))
                    held.append(st)
            if self._bank is not None:
                base = self._bank.camera.data_ptr()
                at = {name: a for name, a, b in _CAMERA_ROW}
                for slot, row in enumerate(self._bank.rows):
                    if row is not None:
                        p = base + 160 * slot
                        entries.append((row, 0, 0, p + 4 * at["viewmatrix"], p + 4 * at["projmatrix"], p + 4 * at["campos"]))
            seen = {}
            for e in entries:
                for addr in e[3:]:
                    if seen.setdefault(addr, e[0]) != e[0]:
                        raise ValueError(f"FusedMapper.update_poses: one camera tensor is bound to trajectory rows {seen[addr]} and {e[0]}")
            table = torch.tensor(np.asarray(entries, np.int64).reshape(-1, 6), device=self.device)
            self._repose_table = (table, held)
        return self._repose_table[0]

    def update_poses(self, traj, new_poses=None):
        """Mapping.update_poses (SLAM/multiprocess/mapper.py:256-263; slam.py:126-127 before every mapping(), :181-182 before the final
        global_optimization) for the trajectory, the window and the bank in ONE launch (dqo_traj_repose, csrc/map_repose.hip): traj (a
        dqo_icp.Trajectory made with a projection) takes new_poses as Trajectory.update_poses does, and every window frame and bank
        slot bound to a trajectory row — set_frame(k, row=...), bank_set(slot, row=...), the "row" key of capture_window's and
        capture_bank's frame dicts — gets the viewmatrix / projmatrix / campos of its row's corrected pose, written where the captured
        graphs read them: a window graph's own settings tensors in place, a bank slot's camera row, whose next select copies it again
        (the launch sets the bank's force word).  new_poses None: the cameras are formed again from the stored poses (a new binding).
        Nothing is read back and the host does no work per keyframe; returns the device counts (int32 [4]: pose rows rewritten,
        targets written — the trajectory's own camera among them — targets skipped for a row outside the trajectory, 0) unread.
        ValueError before the launch: a bound frame whose camera tensors are the mapper's default camera's, or one camera tensor bound
        to two different rows.  Works on a sharded mapper: a camera needs nothing of the map.  bg, the images, the masks and the
        capacities stay: a frame that outgrows its capacities under the new view is run_window's / run_bank's overflow as ever.  A mixed
        graph (k, m) that run_window captures on first use AFTER a correction starts from the camera capture_window was given, as it
        does after set_frame: call update_poses(traj) once more when such a graph has been added."""
        if traj.projection is None:
            raise ValueError("FusedMapper.update_poses: the trajectory was made without a projection, so there is no projmatrix")
        table = self._repose_targets()
        return traj.update_poses(new_poses, targets=table, bank_state=None if self._bank is None else self._bank.state)

    @staticmethod
    def window_schedule(n_iters, n_frames, rng, final=False, random_keyframes=False, global_opt=False):
        """The per-iteration frame choice of the reference's loops as a list of frame indices:
          local_optimize (mapper.py:570-576):   random_index = random.randint(0, len - 1);  if iter > n / 2: random_index = -1
          global_optimization (:1186-1199):     the same draw — but the camera and the target images are taken BEFORE the index is
                                                overwritten (`frame_input = select_frame[random_index]` at :1188-1190, the `= -1` at
                                                :1194-1195), only the tile mask and the render mask follow it: in the second half of a
                                                (non-final) call a RANDOM keyframe is rendered and compared under the LAST keyframe's
                                                masks.  global_opt=True reproduces that: those entries are pairs (k, n_frames - 1) —
                                                replay() / run_window() capture such a mixed graph on first use.
        rng: a random.Random (the reference draws from the global `random` module).  Index -1 = the last frame of the set (the newest
        processed frame / select_frame[-1]); final = the `is_final` pass (random throughout)."""
        out = []
        for it in range(int(n_iters)):
            k = rng.randint(0, n_frames - 1)
            if it > n_iters / 2 and not final and not random_keyframes:
                k = (k, n_frames - 1) if (global_opt and k != n_frames - 1) else n_frames - 1
            out.append(k)
        return out

    def _graph_of(self, frame):
        """The captured graph of a schedule entry: a frame index, or a pair (k, m) = frame k's camera and target under frame m's render
        mask and tile mask (captured on first use from the window's frames, state untouched)."""
        if not isinstance(frame, tuple):
            return self._frames[frame]
        if frame not in self._mixed:
            k, m = frame
            fk, fm_ = self._window_frames[k], self._window_frames[m]
            snap = self._snapshot_state()
            cur = self._g
            self.capture(fk["gt_color"], fk["gt_depth"], fm_.get("render_mask"), tile_mask=fm_.get("tile_mask"), settings=fk.get("settings"),
                         pixel_object=fk.get("pixel_object"), frame=frame, **self._window_kw)
            self._restore_state(snap)
            self._g = cur
            # the window's frames were captured a while ago: set_frame / refresh_window have rewritten frame m's masks in place since
            g2, gm = self._mixed[frame], self._frames[m]
            for src, dst in ((gm.mask, g2.mask), (gm.tile_mask, g2.tile_mask)) if gm is not None else ():
                if src is not None and dst is not None and dst.data_ptr() not in (src.data_ptr(), self.tile_mask.data_ptr()):
                    dst.copy_(src.view(dst.shape))
        return self._mixed[frame]

    def run_window(self, schedule, check_every=64, capacity_margin=1.5):
        """The iterations of `schedule` (frame indices, see window_schedule) on the captured frame set: one graph launch each, one small
        D2H read per `check_every` launches (device step count).  A frame that outgrew its captured capacities made its iterations
        no-ops for the optimiser (parameters, moments, confidence, step count untouched): that frame is captured again on the current
        state with `capacity_margin` and the lost iterations are replayed on it at the end of the batch.  Returns the re-captures."""
        recaptures, i = 0, 0
        while i < len(schedule):
            batch = schedule[i:i + check_every]
            start = self.step_count
            self.replay_schedule(batch)
            lost = (start + len(batch)) - (int(self._step_dev.item()) - 1)
            if lost > 0:
                self._settle_replays()
                bad = [k for k in sorted(set(batch), key=str) if self.graph_overflowed(self._graph_of(k))]
                if not bad or recaptures > 8 * max(1, len(self._frames)):
                    raise RuntimeError("FusedMapper.run_window: the map keeps outgrowing the captured capacities")
                for k in bad:
                    g = self._graph_of(k)
                    snap = self._snapshot_state()
                    self._recapture(g, capacity_margin)
                    self._restore_state(snap)
                    recaptures += 1
                for j in range(lost):
                    self.replay(frame=bad[j % len(bad)])
                torch.cuda.synchronize()
            i += len(batch)
        return recaptures

    # ------------------------------------------------------------------ the keyframe bank (csrc/map_window_bank.hip) -----
    def _require_bank(self, who):
        if self._bank is None:
            raise RuntimeError(f"FusedMapper.{who}: this mapper has no keyframe bank; call capture_bank() first")
        return self._bank

    @torch.no_grad()
    def capture_bank(self, frames, slots=None, schedule_capacity=16384, capacity_margin=1.15, unroll=1, **capture_kw):
        """ONE captured graph that trains over a whole keyframe set — the call that ends every run of the reference,
        global_optimization(is_end=True) (SLAM/slam.py:183, mapper.py:1143-1148, 1196-1199: all keyframes, a random one per iteration),
        where one graph, one probe and one set of context buffers per keyframe (capture_window) cost more than the iterations they
        prepare.  frames: capture_window's dicts, every one with a render mask; they fill slots 0 .. len(frames) - 1 of a bank of
        `slots` (default len(frames)) keyframes in device memory — spare slots take keyframes that arrive later (bank_set) without a new
        capture.  The graph reads staging buffers of its own; every iteration of it starts with dqo_window_bank_select, which moves the
        keyframe the device-side schedule names into them (run_bank), so the frame choice costs no host work and iterations on
        DIFFERENT frames share a launch: unroll = iterations per launch of run_bank (a single-iteration graph serves the tail).
        The capacities are the maximum over the filled slots of what a probe under each slot's own camera and tile mask reports, with
        capacity_margin; schedule_capacity: entries of the device schedule (run_bank uploads a longer one in pieces).  capture_kw:
        capture()'s other options (list_split="auto" is refused: it is a per-frame choice; keep_tile_order defaults to False here: one frame's
        tile order would serve every keyframe).  The capture's eager iteration is undone as
        capture_window undoes it; the select state is left unarmed.  Parameters, moments and every result are bit for bit those of
        capture_window + run_window on the same schedule."""
        self._refuse_sharded("capture_bank", "would need a bank per shard and one schedule over them")
        if capture_kw.get("list_split", 0) == "auto":
            raise RuntimeError("FusedMapper.capture_bank: list_split='auto' is a per-frame choice; give a threshold")
        for name in ("run_unroll", "frame", "head", "settings", "pixel_object", "tile_mask", "reuse_probe"):
            if name in capture_kw:
                raise RuntimeError(f"FusedMapper.capture_bank: {name} is not an option of a bank's graph")
        frames = list(frames)
        K_cap = len(frames) if slots is None else int(slots)
        if not frames or K_cap < len(frames):
            raise RuntimeError("FusedMapper.capture_bank: slots must hold the frames given (at least one)")
        if any(fr.get("render_mask") is None for fr in frames):
            raise RuntimeError("FusedMapper.capture_bank: every keyframe needs a render mask")
        bank = _KeyframeBank(K_cap, self.settings, self.gaussian_object is not None, schedule_capacity, self.device)
        # keep_tile_order would keep the tile launch order of the ONE frame the capture's eager iteration ran on for every keyframe: a
        # stale order costs the blend kernels more (30 us on bench.py's window of five, profiles/window_bank.txt) than the scan that
        # recomputes it (20 us), and the keyframes of a bank lie further apart than a window's frames.  Off unless asked for; the order
        # is a scheduling hint, the results are the same bits either way
        capture_kw.setdefault("keep_tile_order", False)
        bank.capture_kw, bank.capacity_margin, bank.unroll = dict(capture_kw), float(capacity_margin), max(1, int(unroll))
        self._bank = bank
        for k, fr in enumerate(frames):
            self.bank_set(k, gt_color=fr["gt_color"], gt_depth=fr["gt_depth"], render_mask=fr["render_mask"], tile_mask=fr.get("tile_mask"),
                          settings=fr.get("settings", self.settings),
                          pixel_object=(self.pixel_object if fr.get("pixel_object") is None else fr["pixel_object"]) if bank.gate else None,
                          row=fr.get("row"))
        self._capture_bank_graph(bank.capacity_margin)
        return self

    def _capture_bank_graph(self, capacity_margin):
        """The bank's graph, captured (again) on the current state: staging buffers filled from the first keyframe for the eager
        iteration, whose select launch finds an empty schedule and copies nothing; the iteration is undone."""
        bank = self._bank
        self._settle_replays()  # (the snapshot's step count is the settled one)
        snap = self._snapshot_state()
        cur = self._g
        with torch.cuda.device(self.device):
            bank.stage_slot(bank.slots()[0])
            bank.arm(0, N.current_stream())
        self.capture(bank.stage["gt_color"], bank.stage["gt_depth"], bank.stage["render_mask"], tile_mask=bank.stage["tile_mask"],
                     settings=bank.camera_of(bank.slots()[0]), pixel_object=bank.stage["pixel_object"], frame="bank",
                     capacity_margin=capacity_margin, unroll=1, run_unroll=bank.unroll, head=bank, **bank.capture_kw)
        torch.cuda.synchronize()
        self._restore_state(snap)
        self._g = cur if cur is not None else bank.graph

    @torch.no_grad()
    def bank_set(self, slot, gt_color=None, gt_depth=None, render_mask=None, tile_mask=None, settings=None, pixel_object=None, row=None):
        """New inputs for slot `slot` of the keyframe bank, written in place, with set_frame's rules: same shapes, and the scalar
        intrinsics are captured kernel arguments that must not change.  A slot that was never filled needs gt_color, gt_depth,
        render_mask and settings; a new keyframe in a spare slot keeps the captured graph (if it outgrows the capacities, run_bank
        captures again as for any overflow).  The next select copies both groups whatever it copied last (force).  row: the trajectory
        row the slot's camera follows under update_poses (negative: none any more; None: as it was)."""
        bank = self._require_bank("bank_set")
        slot = int(slot)
        if not 0 <= slot < bank.K_cap:
            raise RuntimeError(f"FusedMapper.bank_set: slot {slot} outside the bank's {bank.K_cap}")
        H, W, dev = bank.H, bank.W, self.device
        if not bank.filled[slot] and any(x is None for x in (gt_color, gt_depth, render_mask, settings)):
            raise RuntimeError("FusedMapper.bank_set: a new keyframe needs gt_color, gt_depth, render_mask and settings")
        if pixel_object is not None and not bank.gate:
            raise RuntimeError("FusedMapper.bank_set: the bank was captured without an object gate")
        if settings is not None:
            new = _normalised_settings(settings, dev)
            for name in _CAPTURED_SCALARS:
                if getattr(new, name) != getattr(bank.scalars, name):
                    raise RuntimeError(f"FusedMapper.bank_set: {name} is a captured kernel argument; every keyframe of a bank shares it")
            for name, a, b in _CAMERA_ROW:
                bank.camera[slot, a:b].copy_(getattr(new, name).reshape(-1))
        for name, src, shape in (("gt_color", gt_color, (3, H, W)), ("gt_depth", gt_depth, (1, H, W))):
            if src is not None:
                if tuple(src.shape) != shape or src.dtype != torch.float32:
                    raise RuntimeError(f"FusedMapper.bank_set: {name} must be a float32 tensor of shape {shape}")
                getattr(bank, name)[slot].copy_(src)
        if render_mask is not None:
            bank.render_mask[slot].copy_(render_mask.to(torch.uint8).reshape(H, W))
        if tile_mask is not None:
            bank.tile_mask[slot].copy_(_checked_tile_mask(tile_mask, dev, H, W).view(bank.tile_mask.shape[1:]))
        if pixel_object is not None:
            bank.pixel_object[slot].copy_(torch.as_tensor(pixel_object).to(dev, torch.int32).reshape(H, W))
            bank.tile_objects[slot].copy_(tile_object_sets(bank.pixel_object[slot]))
        bank.filled[slot] = True
        if row is not None:
            self._bind_row(bank.rows, slot, row)
        bank.word("force").fill_(1)
        return self

    def _bank_launch(self, n):
        """n iterations of the bank's graph: launches of `unroll` iterations while that many remain, single ones for the rest."""
        g = self._bank.graph
        self._g, k = g, g.run_unroll
        while n >= k and k > 1:
            self._launch(g, g.run_graph, k)
            n -= k
        for _ in range(n):
            self._launch(g, g.graph, 1)

    def run_bank(self, schedule, check_every=64, capacity_margin=1.5):
        """The iterations of `schedule` — window_schedule's list: slot indices, or pairs (k, m) = slot k's camera, targets and gate
        under slot m's render mask and tile mask — on the bank's ONE graph: one upload of the schedule, one arm launch, then graph
        launches with no host work per iteration.  One small read per `check_every` iterations: the device step count, the select
        state's overrun and lost_count words and the overflow flag of the batch's last frame.  A frame that outgrew the captured
        capacities was a no-op for the optimiser; the select launch behind it logged its schedule position, so the lost positions are
        known exactly: the graph is captured again on the current state with `capacity_margin`, the rest of the schedule goes on, and
        the lost entries are replayed as a new armed schedule after it — the call trains the schedule less the retried positions, then
        the retried positions.  Returns the retried schedule positions (a position retried twice is listed twice)."""
        bank = self._require_bank("run_bank")
        entries = [tuple(int(x) for x in e) if isinstance(e, (tuple, list)) else (int(e), int(e)) for e in schedule]
        for k, m in entries:
            if not (0 <= k < bank.K_cap and 0 <= m < bank.K_cap and bank.filled[k] and bank.filled[m]):
                raise RuntimeError(f"FusedMapper.run_bank: schedule entry ({k}, {m}) names a slot that holds no keyframe")
        if bank.graph is None:
            self._capture_bank_graph(bank.capacity_margin)
        retried, pending, recaptures = [], list(range(len(entries))), [0]
        while pending:
            lost = self._run_bank_pass([entries[p] for p in pending], check_every, capacity_margin, recaptures)
            pending = [pending[i] for i in lost]
            retried += pending
        return retried

    def _run_bank_pass(self, entries, check_every, capacity_margin, recaptures):
        """One armed pass over `entries`; returns the positions (indices into entries) whose frames were lost.  recaptures: [count]."""
        bank, dev = self._bank, self.device
        room, lost_all = bank.schedule.shape[0], []
        i, first, end, logged = 0, 0, 0, 0  # the armed piece is entries[first:end]; `logged` entries of its log have been read
        with torch.cuda.device(dev):
            while i < len(entries):
                if i >= end:
                    first, end, logged = i, min(len(entries), i + room), 0
                    bank.schedule[:end - first].copy_(torch.from_numpy(np.asarray(entries[first:end], np.int32).reshape(-1, 2)))
                    bank.arm(end - first, N.current_stream())
                b = min(int(check_every), end - i)
                self._bank_launch(b)
                i += b
                words = torch.cat([self._step_dev, bank.state[N.TICKET_WORDS:N.TICKET_WORDS + len(N.WINDOW_BANK_WORDS)],
                                   header_words(bank.graph.geom)[2:3]]).tolist()
                dev_step, state, last_lost = words[0], dict(zip(N.WINDOW_BANK_WORDS, words[1:])), words[-1] != 0
                if state["overrun"]:
                    raise RuntimeError(f"FusedMapper.run_bank: the select launch ran off its schedule (overrun {state['overrun']})")
                lost = bank.lost[logged:state["lost_count"]].tolist() if state["lost_count"] > logged else []
                if last_lost:  # (the next select would log it; the schedule is armed anew before that)
                    lost.append(i - 1 - first)
                if (self.step_count + 1) - dev_step != len(lost):
                    raise RuntimeError("FusedMapper.run_bank: the device step count and the lost-frame log disagree")
                if lost:
                    lost_all += [first + p for p in lost]
                    self._settle_replays()
                    recaptures[0] += 1
                    if recaptures[0] > 8 * max(1, len(bank.slots())):
                        raise RuntimeError("FusedMapper.run_bank: the map keeps outgrowing the captured capacities")
                    self._capture_bank_graph(capacity_margin)
                    end = i  # (the capture's eager select used the state: the rest of the schedule is armed anew)
        return lost_all

    @torch.no_grad()
    def set_frame(self, frame, gt_color=None, gt_depth=None, render_mask=None, tile_mask=None, settings=None, pixel_object=None, row=None):
        """New inputs for a captured frame WITHOUT a new capture: the next mapping call's window keeps four of its five frames and every
        call re-evaluates the masks (mapper.py:549-555).  Everything a graph reads per frame lives in device buffers the capture fixed:
        the camera's matrices / position / background, the ground-truth images, the render mask, the tile mask, the owner map — they
        are overwritten in place (same shapes; a frame captured without a render mask cannot get one later, and the scalar intrinsics
        — image size, tan(fov), principal point, thresholds — are kernel arguments: they must not change).  The captured capacities
        were sized on the old view: check graph_overflowed(frame) / use run_window, which re-captures a frame that outgrew them.
        row: the trajectory row the frame's camera follows under update_poses (negative: none any more; None: as it was)."""
        if row is not None:
            self._bind_row(self._frame_rows, frame, row)
        cams = [self._frames[frame]] + [g for (k, m), g in self._mixed.items() if k == frame]    # graphs that render frame's camera / target
        masks = [self._frames[frame]] + [g for (k, m), g in self._mixed.items() if m == frame]   # graphs that use frame's masks
        done = set()

        def once(t):  # (graphs of one window share the tensors they were given: write each buffer once)
            if t.data_ptr() in done:
                return False
            done.add(t.data_ptr())
            return True

        for g in cams:
            if gt_color is not None and once(g.gt_color):
                g.gt_color.copy_(gt_color)
            if gt_depth is not None and once(g.gt_depth):
                g.gt_depth.copy_(gt_depth)
        for g in masks:
            if render_mask is not None:
                if g.mask is None:
                    raise RuntimeError("FusedMapper.set_frame: the frame was captured without a render mask")
                if once(g.mask):
                    g.mask.copy_(render_mask.to(torch.uint8))
            if tile_mask is not None and once(g.tile_mask):
                g.tile_mask.copy_(_checked_tile_mask(tile_mask, self.device, int(g.settings.image_height), int(g.settings.image_width)))
        if settings is not None:
            new = _normalised_settings(settings, self.device)
            for g in cams:
                for name in _CAPTURED_SCALARS:
                    if getattr(new, name) != getattr(g.settings, name):
                        raise RuntimeError(f"FusedMapper.set_frame: {name} is a captured kernel argument; capture the frame again")
                for name in ("bg", "viewmatrix", "projmatrix", "campos"):
                    getattr(g.settings, name).copy_(getattr(new, name))
        if pixel_object is not None:
            for g in cams:
                if g.pixel_object is None:
                    raise RuntimeError("FusedMapper.set_frame: the frame was captured without an object gate")
                if once(g.pixel_object):
                    g.pixel_object.copy_(torch.as_tensor(pixel_object).to(self.device, torch.int32).reshape(g.pixel_object.shape))
                    g.tile_objects.copy_(tile_object_sets(g.pixel_object))
        return self

    def capture_placed(self, *args, trials=4, probe_replays=12, **kw):
        """capture() on the best of `trials` PLACEMENTS of the context buffers.  Where the allocator puts the geometry / binning / image
        buffers in physical memory moves the binning kernel by +-5 us and the per-Gaussian tail by +-3 us on cfg 3 — same code, same
        virtual layout, another set of pages (tools/bin_count_place.py: 52-62 us between the buffer sets of ONE process; the device
        atomics and partial-line writes of those kernels meet the memory channels differently).  So: capture `trials` times, every time
        on freshly allocated buffers while the earlier sets are still held (the allocator must place the next set elsewhere), time
        `probe_replays` replays of each, keep the fastest graph and hand the other buffers back.  The optimisation state is put back
        in between and at the end — parameters, moments, step count: the iterations of the trials never happened; what remains is
        exactly capture()'s own eager iteration, re-run on the kept buffers.  Results do not depend on the placement (bit for bit)."""
        if int(trials) <= 1:
            return self.capture(*args, **kw)
        self._settle_replays()  # (the snapshot's step count is the settled one)
        snap = self._snapshot_state()

        def restore():
            self._restore_state(snap)

        cands = []
        for t in range(int(trials)):
            if t:
                restore()
                self._g = None  # (the earlier sets stay referenced by `cands`: this capture's buffers land elsewhere)
            self.capture(*args, **kw)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                self.replay()
            e0.record()
            for _ in range(int(probe_replays)):
                self.replay()
            e1.record()
            torch.cuda.synchronize()
            self._settle_replays()
            if self.graph_overflowed():  # (an overflowed trial replays no-ops: fast, and worthless)
                continue
            cands.append((e0.elapsed_time(e1) / probe_replays / self._g.unroll, self._g))
        if not cands:
            raise RuntimeError("FusedMapper.capture_placed: every trial overflowed its captured capacities")
        best = min(range(len(cands)), key=lambda i: cands[i][0])
        self.placement_trials_ms = [round(c[0], 4) for c in cands]
        restore()
        self._g = cands[best][1]
        if self._g.frame is not None:
            self._frames[self._g.frame] = self._g
        del cands
        self.step_static()    # capture()'s eager iteration, on the kept buffers
        torch.cuda.synchronize()
        return self

    def _probe(self, tile_mask, st=None, pixel_object=None, tile_objects=None):
        """(num_candidates, longest tile list) of the current state: one forward on scratch buffers with packed lists."""
        P, M = self.P, self.M
        st = self.settings if st is None else st
        if pixel_object is None:
            pixel_object, tile_objects = self.pixel_object, self.tile_objects
        c = _RenderContext(P, int(st.image_width), int(st.image_height), self.device)
        params = dgr._params(st, P, M)
        inputs = dgr._inputs(st, self.xyz, self.shs, self._empty, self.opacity, self.scales, self.rotations, self._empty, tile_mask,
                             row_flags=self.row_flags)
        fields = {}
        if self.gaussian_object is not None:
            # the lists of the gated job (the binning drops a pair whose object owns no pixel of the tile): its longest list, not the
            # ungated frame's, sizes the buckets
            gate = N.DqoObjectGate(gaussian_object=N.ptr(self.gaussian_object), pixel_object=N.ptr(pixel_object), tile_objects=N.ptr(tile_objects))
            fields["object_gate"] = ctypes.addressof(gate)
        stream = N.current_stream()
        cand = int(c.measure(params, inputs, c.outputs, stream, **fields).num_candidates)
        c.size(max(cand, 1))
        c.render(params, inputs, c.outputs, stream, **fields)
        return cand, int(c.header(stream).max_tile_count)

    def _static_iteration(self, lean=False):
        """The five C-ABI calls of one iteration over the persistent buffers (no allocation, no host-side per-step state).  lean: the
        forward in its training form (dqo_rast_forward_train) — for an iteration whose outputs the next one overwrites unread; honoured
        where nothing behind the forward reads an auxiliary output (loss tap on, no split forward)."""
        lib, g = N.lib(), self._g
        forward = lib.dqo_rast_forward_train if (lean and g.tap is not None and g.ls_fwd <= 0) else lib.dqo_rast_forward
        st = self.settings
        H, W = int(st.image_height), int(st.image_width)
        stream = N.current_stream()
        if g.head is not None:  # (a bank graph: the scheduled keyframe moves into the buffers the calls below read)
            g.head.select(g, stream)
        g.cctx.list_split = g.ls_fwd
        N.check(forward(ctypes.byref(g.params), ctypes.byref(g.inputs), ctypes.byref(g.outputs), ctypes.byref(g.cctx), stream))
        g.cctx.list_split = g.ls_bwd  # (0 with a split forward: the single-wave backward walks every list, the queue is ignored)
        o = g.out
        if g.tap is None:
            N.check(lib.dqo_map_loss_fwd_bwd(W, H, o[0].data_ptr(), o[1].data_ptr(), o[3].data_ptr(), N.ptr(g.gt_color), N.ptr(g.gt_depth),
                                             N.ptr(g.mask), self.color_weight, self.depth_weight, self.add_depth_thres, N.ptr(self.loss),
                                             N.ptr(self.dL_dcolor), N.ptr(self.dL_ddepth), N.ptr(self.loss_ws), self.loss_ws.numel(), stream))
            if g.mask is None and self.ssim_weight != 0:
                self._ssim_term(o[0].data_ptr(), g.gt_color, stream)
        dLc, dLd = (self.dL_dcolor.data_ptr(), self.dL_ddepth.data_ptr()) if g.tap is None else (None, None)
        self._attach_n = ((self.P + 255) // 256) * (4 if g.fused_tail else 1)
        if g.fused_tail:
            N.check(lib.dqo_rast_backward_adam(ctypes.byref(g.params), ctypes.byref(g.inputs), ctypes.byref(g.cctx), dLc, dLd,
                                               ctypes.byref(g.adam), g.ws.data_ptr(), g.ws.numel(), stream))
            return
        N.check(lib.dqo_rast_backward(ctypes.byref(g.params), ctypes.byref(g.inputs), ctypes.byref(g.cctx), dLc, dLd, o[3].data_ptr(),
                                      ctypes.byref(g.cgrads), g.ws.data_ptr(), g.ws.numel(), stream))
        N.check(lib.dqo_map_adam_step(ctypes.byref(g.adam), stream))

    def _ssim_term(self, color_ptr, gt_color, stream):
        """Without a render mask the loss carries the SSIM term (mapper.py:839-845; with one the reference skips it, B14): its gradient
        is added onto the colour-gradient image dqo_map_loss_fwd_bwd just wrote, its value onto self.loss[0] (slot 3 = 1 - ssim)."""
        lib = N.lib()
        H, W = int(self.settings.image_height), int(self.settings.image_width)
        if self.ssim_ws is None:
            self.ssim_ws = torch.empty((lib.dqo_map_ssim_workspace_bytes(W, H),), dtype=torch.uint8, device=self.device)
            self.ssim_out = torch.zeros((2,), dtype=torch.float32, device=self.device)
        N.check(lib.dqo_map_ssim_fwd_bwd(W, H, color_ptr, N.ptr(gt_color), self.ssim_weight, N.ptr(self.ssim_out), N.ptr(self.dL_dcolor), 1,
                                         N.ptr(self.loss), N.ptr(self.ssim_ws), self.ssim_ws.numel(), stream))

    def replay(self, frame=None):
        """One mapping iteration (capture(unroll=k): k of them) by replaying a captured graph — `frame`: which one of capture_window's
        (None: the one replayed last / the single-frame mapper's); outputs are the persistent tensors in self._g.out."""
        if frame is not None:
            self._g = self._graph_of(frame)
        return self._launch(self._g, self._g.graph, self._g.unroll)

    def replay_run(self, frame, n):
        """n consecutive iterations on ONE frame of the window: launches of the frame's run graph (capture_window(run_unroll=k): k
        iterations each) while at least k remain, single launches for the rest — the same kernels in the same order as n replay(frame)
        calls, bit for bit.  Returns the outputs like replay()."""
        g = self._graph_of(frame)
        k = g.run_unroll
        out = None
        while n >= k and k > 1:
            self._g = g
            out = self._launch(g, g.run_graph, k)
            n -= k
        for _ in range(n):
            out = self.replay(frame=frame)
        return out

    def replay_schedule(self, schedule):
        """The iterations of `schedule` (window_schedule) with every stretch on one frame handed to replay_run."""
        i = 0
        while i < len(schedule):
            j = i
            while j < len(schedule) and schedule[j] == schedule[i]:
                j += 1
            self.replay_run(schedule[i], j - i)
            i = j

    def _settle_replays(self):
        """Make the host step count agree with what the device counted.  replay() assumes a valid frame; the device count only advances
        on valid ones (DqoAdamStep.frame_header: an overflowed frame is a no-op for the optimiser), so what it falls short of the count
        expected after the last replay is the number of invalid replays — taken back here, BEFORE anything else (an eager step(), a
        re-capture, a resynchronisation) builds on the host count or overwrites the device count.  One 4-byte read, and only when
        replays happened since the last time."""
        if not self._unsettled:
            return
        dev_step = int(self._step_dev.item())
        invalid = int(self._expected_step) - dev_step
        if invalid > 0:
            self.step_count -= invalid
        self._expected_step = dev_step
        self._unsettled = False

    def _resync_step_count(self):
        """Eager step() calls between two replays advanced the host count alone: bring the device count up to it."""
        self._settle_replays()
        self._step_dev.fill_(self.step_count + 1)
        self._expected_step = self.step_count + 1

    def run(self, n_iters, check_every=64, capacity_margin=1.5):
        """`n_iters` VALID mapping iterations on the captured graph: replays in batches of `check_every`, one small D2H read per batch
        (device-side step count + overflow flag); if the map outgrew the captured capacities in a batch, the invalid replays were no-ops for the
        optimiser (DqoAdamStep.frame_header: parameters, moments and the device step count are untouched), so the graph is captured
        again on the current state with `capacity_margin` and the missing iterations are replayed.  Returns the number of
        re-captures.  The inputs of the last capture() (ground-truth images, masks) are reused."""
        if self._g.unroll != 1:
            raise RuntimeError("FusedMapper.run counts single iterations: capture with unroll=1")
        target = self.step_count + n_iters
        recaptures = 0
        while self.step_count < target:
            k = min(check_every, target - self.step_count)
            for _ in range(k):
                self.replay()
            # the device-side step count only advances on valid frames: one 4-byte read tells whether ANY replay of the batch was invalid
            # (the header's flag alone would only tell about the last one)
            if int(self._step_dev.item()) - 1 != self.step_count or self.graph_overflowed():
                if recaptures > 8:
                    raise RuntimeError("FusedMapper.run: the map keeps outgrowing the captured capacities")
                # (capture() re-reads the device-side step count: the valid replays of this batch stay counted, the others do not)
                self._recapture(self._g, capacity_margin)
                recaptures += 1
        return recaptures

    def step_static(self):
        """One iteration over the persistent buffers issued eagerly — exactly the calls the captured graph holds (for per-kernel
        profiling: events cannot be recorded inside a replay)."""
        return self._launch(self._g, None, 1)

    def _launch(self, g, graph, n):
        """n iterations of graph g: a launch of `graph` (one of g's captured graphs), or None = g's calls issued eagerly (n = 1)."""
        if g.stale:
            raise RuntimeError("FusedMapper: the attach set / object gate changed since capture(); capture again")
        if self._expected_step != self.step_count + 1:  # eager step() calls in between: resynchronise the device-side step count
            self._resync_step_count()
        if graph is None:
            with torch.cuda.device(self.device):
                self._static_iteration()
        else:
            graph.replay()
        self._unsettled = True
        self._attach_n = ((self.P + 255) // 256) * (4 if g.fused_tail else 1)  # (a new mapping call in between had reset it)
        self.step_count += n  # (assumes valid frames; _settle_replays re-reads the device-side count)
        self._expected_step = self.step_count + 1
        return g.out

    def header(self, g=None):
        """Device header of the captured iteration's last forward (one small D2H read, synchronises)."""
        return read_header((self._g if g is None else g).geom)

    def graph_overflowed(self, g=None):
        """True if the last replayed iteration (of graph g: a frame of the window; default the current one) produced more instances than
        the captured capacity (one small D2H read)."""
        return overflowed((self._g if g is None else g).geom)

    def _params(self):
        return dict(xyz=self.xyz, shs=self.shs, opacity=self.opacity_raw, scaling=self.scaling_raw, rotation=self.rotation_raw)

    @torch.no_grad()
    def step(self, gt_color, gt_depth, render_mask, tile_mask=None):
        """One mapping iteration; returns the op's 9-tuple (views of this iteration's outputs) — losses are in self.loss."""
        lib = N.lib()
        self._settle_replays()  # (replays of invalid frames since the last check do not count: this step's bias corrections depend on it)
        with torch.cuda.device(self.device):
            stream = N.current_stream()
            self.activate()  # (later iterations get the activations from the previous Adam step)
            ctx = _Ctx()
            ctx.row_flags = self.row_flags  # (hidden rows are not rendered, as in the captured iteration; the backward reads it too)
            out = dgr._RasterizeGaussians.forward(ctx, self.xyz, self.shs, self._empty, self.opacity, self.scales, self.rotations,
                                                  self._empty, self.tile_mask if tile_mask is None else tile_mask, self.settings,
                                                  self.gaussian_object, self.pixel_object)
            # NOTE: an eager step on an overflowed frame (lazy mode) is a no-op for the optimiser (DqoAdamStep.frame_header), but the
            # host-side step_count below still advances; the operator raises at its next synchronisation point in that case.
            color, depth, hit_depth = out[0], out[1], out[3]
            H, W = color.shape[1], color.shape[2]
            mask_u8 = None if render_mask is None else render_mask
            if mask_u8 is not None and mask_u8.dtype != torch.uint8:
                mask_u8 = mask_u8.to(torch.uint8)
            if self.per_object_loss and self.gaussian_object is not None:
                # the per-object loss in eager torch (the captured path computes it in the blend kernels: DqoLossTap.per_object)
                with torch.enable_grad():
                    c_, d_ = color.detach().requires_grad_(True), depth.detach().requires_grad_(True)
                    tot, parts = mapping.per_object_loss(dict(render=c_, depth=d_, depth_index_map=hit_depth), gt_color, gt_depth,
                                                         self.pixel_object, render_mask=mask_u8, add_depth_thres=self.add_depth_thres)
                    gc_, gd_ = torch.autograd.grad(tot, [c_, d_])
                self.dL_dcolor.copy_(gc_), self.dL_ddepth.copy_(gd_)
                self.loss[:3] = torch.stack([parts["total_loss"], parts["color_loss"], parts["depth_loss"]])
            else:
                N.check(lib.dqo_map_loss_fwd_bwd(W, H, N.ptr(color), N.ptr(depth), N.ptr(hit_depth), N.ptr(gt_color), N.ptr(gt_depth),
                                                 N.ptr(mask_u8), self.color_weight, self.depth_weight, self.add_depth_thres,
                                                 N.ptr(self.loss), N.ptr(self.dL_dcolor), N.ptr(self.dL_ddepth), N.ptr(self.loss_ws),
                                                 self.loss_ws.numel(), stream))
                if mask_u8 is None and self.ssim_weight != 0:
                    self._ssim_term(N.ptr(color), gt_color, stream)
            ctx.sparse_grad_rows = True  # gradient rows of culled Gaussians stay unwritten; the Adam kernel gets radii instead
            grads = dgr._RasterizeGaussians.backward(ctx, self.dL_dcolor, self.dL_ddepth, None, None, None, None, None, None, None)
            self.step_count += 1
            # (no DqoAdamStep.record_ctx here: the drop-in op owns this frame's context, so the eager step deliberately keeps the radii
            # rule — it updates every in-view row and sets its moment_live byte.  Same bits as the captured iteration's rule, which skips
            # the in-view rows without a gradient record; more rows touched, and those rows stay listed until the next mapping call.)
            st = self._adam_step_args([N.ptr(grads[i]) for i in (0, 1, 3, 4, 5)], radii=N.ptr(out[8]),
                                      frame_header=N.ptr(ctx.saved_tensors[8]), step=self.step_count)
            N.check(lib.dqo_map_adam_step(ctypes.byref(st), stream))
            self._attach_n = (self.P + 255) // 256
        return out
