"""Keyframe evaluation on MI355X: the metrics the reference reports for a rendered frame — eval_picture, SLAM/eval.py:38-188, called per
frame from slam.py:155,184 and from metric.py — without a host round trip per number.

    eval_picture(render_output, gt_color, gt_depth, min_depth, max_depth)  ->  float32 [8] on the device (ROW)
    ms_ssim(image, gt)                                                     ->  float32 [20] on the device (MS_ROW)
    lpips(image, gt, weights)                                              ->  float32 [8] on the device (LPIPS_ROW)
    eval_picture_dict(row, ms_row=None, lpips_row=None)                    ->  the reference's dict (the ONE host read)

One HIP launch (libdqoraster.so: dqo_eval_picture, csrc/map_eval.hip) forms psnr (eval.py:63), the colour L1 (:70) and the depth
statements (:115-126) from double sums added in a fixed order: a row is bitwise reproducible.  The SSIM slot is filled by
dqo_map_ssim_fwd_bwd in value-only mode (two more launches).  Nothing is read back, so a keyframe set is evaluated into a [K, 8] table
(`out=`, `row=`) and read once; the calls can be captured in a graph.

The reference's "ssim" key is MS-SSIM (pytorch_msssim's `ms_ssim`, eval.py:19-25, :64), NOT the single-scale SSIM of slot 4: `ms_ssim`
(libdqoraster.so: dqo_eval_ms_ssim, csrc/map_msssim.hip — nine launches, nothing read back) forms it with its fifteen per-level factors
into a row of its own, and eval_picture_dict(row, ms_row) reports it under "ssim".  pytorch_msssim does not exist on this platform: the
kernels follow the algorithm as its published source states it (tests/msssim_oracle.py restates it), and are held to that restatement,
not to a value recorded from the library.

The reference's third number, "lpips" (`lpips` AlexNet through torchmetrics, :28-30, :65-68), is `lpips` (libdqoraster.so: dqo_eval_lpips,
csrc/map_lpips.hip — five convolutions on the f32 matrix cores, two pools, five heads, nothing read back) on weights the CALLER brings
as a LpipsWeights: none are shipped and nothing is fetched, so the number is the reference's only on the reference's weights.  Its row
holds the five layer terms beside the value, and eval_picture_dict(row, ms_row, lpips_row) reports it under "lpips".  Neither `lpips`
nor `torchmetrics` exists on this platform: the kernels follow the algorithm as the published sources state it (tests/lpips_oracle.py
restates it) and are held to that restatement on seeded random weights of the real shapes, not to a value recorded from the libraries.

What is NOT here: slot 4 of ROW stays the SINGLE-SCALE SSIM of utils/loss_utils.py:60-100 (the one the mapping loss uses).  The picture
dumps (`save_picture`) and the semantic / instance branches are not built.

Geometry evaluation — eval_pcd, SLAM/eval.py:190-282: accuracy, completion, chamfer distance and precision / recall / F1 per distance
threshold of a reconstruction against a ground-truth point set — stays on the device as well:

    eval_pcd(gt_points, rec_points, dist_thres, transform)  ->  float32 [32] on the device (PCD_ROW)
    eval_pcd_dict(row, dist_thres)                          ->  the reference's `results` dict plus `chamfer` (the ONE host read)
    nearest(query, ref)                                     ->  (dist2, idx): the exact nearest reference of every query (dqo_nn1)

Two dense exact 1-NN searches (dqo_nn1, csrc/knn.hip) replace the 4 + 2 T scipy KDTree builds and single-threaded queries of the
reference, one reduction launch (dqo_eval_pcd, csrc/map_eval.hip) forms every number from double sums added in a fixed order.

The reconstruction the reference evaluates where a config sets `pcd_densify` (replica, aithor, real, Cube_Diorama) is not one point per
Gaussian but the DENSIFIED stable cloud — GaussianPointCloud.densify(1, 30, 5), SLAM/gaussian_pointcloud.py:67-130, 150 points on five
ellipses per surfel — of which eval_pcd keeps `sample_nums` by np.random.choice (eval.py:244):

    densify(xyz, scaling_raw, rotation_raw, ...)            ->  dict(points, normals, index, keep, header), all on the device

One call (dqo_surfel_densify, csrc/map_densify.hip) forms the subsample of the densified cloud without ever holding the cloud; `keep`
goes to eval_pcd as `rec_keep`.  (The Python function uploads the 2 * circle_num floats of its angle table per call: a host-blocking
copy; the C entry itself does not synchronise.)  The draw is the key rule of csrc/dqo_sample_hash.h, not numpy's stream: the same distribution, a pure
function of the arguments.

The ground truth the reference evaluates against is `trimesh.sample.sample_surface(mesh_gt, sample_nums)` (eval.py:236, :247): points
drawn on the mesh's surface, a face picked in proportion to its area and a uniform point inside it:

    sample_surface(vertices, faces, count, seed)            ->  dict(points, face_index, keep, header), all on the device

Four launches (dqo_mesh_sample, csrc/map_meshsample.hip) from the mesh's tensors (dqo_ply.read_mesh_ply reads the file on the host);
`keep` goes to eval_pcd as `gt_keep`.  trimesh does not exist on this platform: the kernels follow its four public steps (face areas,
their cumulative sum, one draw located in it, two draws folded back into the triangle where u + v > 1) and are held to a restatement
(tests/mesh_oracle.py), not to a value recorded from the library.  Two departures, both so that a sample is a pure function of the
arguments: the draws are the key rule of csrc/dqo_sample_hash.h instead of numpy's stream (the same distribution), and the cumulative
table counts integer quanta of area instead of float sums (no summation order can reach it).

The geometry number the reference reports PER OBJECT — metric_obj.py:169-236: eval_pcd of each object's stable cloud against that
object's own mesh, dist_threshs=[0.01] — is one call for up to 64 objects, an integer object id per row on both sides:

    nearest_grouped(query, query_group, ref, ref_group)     ->  (dist2, idx): the nearest reference OF THE QUERY'S OWN GROUP
    eval_pcd_objects(gt_points, gt_object, rec_points, rec_object, dist_thres)  ->  float32 [64,32] on the device, a PCD_ROW per object
    eval_pcd_objects_dict(table, dist_thres)                ->  {object id: eval_pcd_dict's dict} (the ONE host read)
    sample_surface_objects(meshes, count, seed)             ->  (points, object): sample_surface of every object's mesh

One build of the reference set, one sort of the queries (by object, then along the Morton grid) and one scan per direction
(dqo_nn1_grouped, csrc/knn.hip), one reduction launch (dqo_eval_pcd_grouped, csrc/map_eval.hip) — instead of one masked eval_pcd per
object, each of which sorts and scans every row of both sets.  Not built: metric_obj.py's hard-coded mesh paths and id -> name table,
its CSV, and the per-frame picture half of its loop (FusedMapper.evaluate serves that).

What is NOT here: writing `pcd_densify.ply` (open3d's layout) is not built; the unused bounding box of eval.py:237-239 is not formed.

Tracking evaluation — Tracker.eval_total_ate, SLAM/multiprocess/tracker.py:341-346, 426-430: the absolute trajectory error after Horn's
alignment (eval_ate, SLAM/utils.py:486-532) for EVERY prefix of the trajectory, which the reference forms with one numpy alignment per
prefix and a Python loop over its points:

    eval_ate(pose_es, pose_gt)                              ->  float64 [N] on the device, centimetres
    eval_ate_dict(curve)                                    ->  {"ate": curve[-1]} (the ONE host read)

One launch (dqo_eval_ate, csrc/map_traj.hip), one block per prefix, sums added in a fixed order.  dqo_icp.Trajectory keeps the two pose
stacks on the device and calls it (`Trajectory.ate()`).  The ATE figure (matplotlib) and scripts/eval_ate.py are not built.

The map as a triangle mesh — make_mesh.py and eval_frame(..., volume=..., scale=...), SLAM/eval.py:299, 316-343, which integrate every
frame's render into an open3d TSDF volume; open3d does not exist on this platform, so the volume and the extraction are the library's
own (csrc/map_tsdf.hip: a dense grid, the integration rule restated in include/dqo_raster.h, marching tetrahedra):

    TsdfVolume(origin, voxel_length, dims, sdf_trunc, device)   tsdf, weight, color: public device tensors
        .clear()  .integrate(depth, color, K, w2c, depth_trunc, render_header)  .extract(cap_vertices, cap_faces)  .counts()

FusedMapper.make_mesh(frames, volume) renders and integrates a camera list; dqo_ply.write_mesh_ply writes the mesh.  Sparse volumes are
not built.

The mesh's clean-up (csrc/map_meshops.hip; the rules in include/dqo_raster.h follow open3d's published algorithms, tests/mesh_ops_oracle.py
restates them), on the mesh dict extract() returns, nothing read back:

    mesh_components(mesh, min_faces, largest_only, ...)   cluster_connected_triangles + remove_triangles_by_mask + remove_unreferenced_vertices
    mesh_simplify(mesh, voxel_size, origin)               simplify_vertex_clustering, the Average contraction, on a grid the caller places
    mesh_smooth(mesh, iterations, lam, mu, scope)         filter_smooth_laplacian / filter_smooth_taubin (configs' mesh_smooth_iter, mesh_smooth_lambda)
    mesh_normals(mesh)                                    compute_vertex_normals
    mesh_counts(mesh)                                     the one host read

FusedMapper.make_clean_mesh chains them behind make_mesh (make_simplified_mesh: with mesh_simplify); dqo_ply.write_mesh_ply_normals writes the result.

Depth L1 — the one number of the dense-SLAM evaluation protocols (the NICE-SLAM lineage) that needs a mesh as an IMAGE: both meshes
rendered to depth from the frames' cameras and compared pixel by pixel (csrc/map_meshrender.hip, a triangle depth rasteriser whose rule
include/dqo_raster.h states and tests/mesh_render_oracle.py restates; csrc/map_eval.hip, dqo_eval_depth_l1):

    mesh_render_depth(mesh, w2c, K, W, H, ...)              ->  dict(depth [n,H,W], face_index | None, header, header_names)
    mesh_render_depth_clip(mesh, w2c, K, W, H, ...)         ->  the same, a face that crosses a view's near plane clipped, not dropped
    mesh_cull_visible(mesh, w2c, K, W, H, depth, ...)       ->  the mesh's faces that win pixels in that render (eval_mesh's visibility="faces")
    depth_l1(depth_gt, depth_rec, view_keep, depth_trunc)   ->  float32 [n + 1, 8] on the device (DEPTH_L1_ROW), a row per view and the set's
    depth_l1_dict(table)                                    ->  the rows as dicts (the ONE host read)
    eval_mesh_depth(rec_mesh, gt_mesh, views)               ->  both meshes rendered, the table

FusedMapper.evaluate_mesh_depth forms the views from frames, and with mesh=None compares the map's own render.  Not built: back-face
culling, per-view intrinsics, colour or normal shading of the mesh.

Exact point-to-triangle distance — the nearest FACE of a mesh per point (csrc/knn.hip, dqo_mesh_nearest: dqo_nn1's walk over the faces;
include/dqo_raster.h states the float32 rule and tests/mesh_dist_oracle.py restates it), and eval_pcd's row on those distances, free of
the nearest-sample floor of about 0.5 / sqrt(samples per square metre) that the sampled form adds to accuracy and completion:

    nearest_on_mesh(points, mesh, ...)                      ->  (dist2 [Q], face [Q] | None, closest [Q,3] | None, header: MESH_NEAREST_HEADER)
    eval_pcd_surface(gt_points, rec_points, gt_mesh, rec_mesh, ...)  ->  float32 [32] (PCD_ROW); a side without a mesh keeps eval_pcd's search
    eval_mesh_surface(rec_mesh, gt_mesh, ...)               ->  eval_mesh's culls and samples, the distances to the culled surfaces

GPU only: there is no CPU path.
"""
import ctypes
import functools

import torch

import _dqo_native as N

ROW = ("psnr", "color_loss", "depth_loss", "valid_pixel_ratio", "ssim", "mse_r", "mse_g", "mse_b")

MS_ROW = (("ms_ssim", "ms_r", "ms_g", "ms_b") + tuple(f"F{l}_{c}" for l in range(5) for c in "rgb") + ("unused19",))
MS_MIN_SIDE = 161  # pytorch_msssim asserts smaller_side > (11 - 1) * 2 ** 4

PCD_THRES_MAX = 8
PCD_ROW = (("accuracy", "completion", "chamfer", "n_thres") + tuple(f"{n}{t}" for t in range(PCD_THRES_MAX) for n in ("P", "R", "F1_"))
           + ("unused28", "unused29", "unused30", "unused31"))

_workspaces = {}  # the module's own workspaces, one per (operator, device, sizes)


def _workspace(key, nbytes, dev):
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _ws(workspace_buffer, dev, nbytes, tag, *sizes):
    """The caller's workspace, or the module's own for (tag, device, sizes).  nbytes: its size, or a function that gives it and raises
    for bad sizes — asked only when the workspace is the module's."""
    if workspace_buffer is not None:
        return workspace_buffer
    return _workspace((tag, _dev_index(dev)) + sizes, nbytes() if callable(nbytes) else nbytes, dev)


_nan_table = functools.partial(torch.full, fill_value=float("nan"))  # (a launch)


def _table_row(out, row, width, who, dev, rows=1, fresh=_nan_table):
    """(out, row) of a result table: the caller's contiguous float32 [K, width] table and the first of the `rows` rows the call writes,
    checked, or a new [rows, width] table made by `fresh` and row 0."""
    if out is None:
        out, row = fresh((rows, width), dtype=torch.float32, device=dev), 0
    if (out.dim() != 2 or out.shape[1] != width or out.dtype != torch.float32 or not out.is_contiguous()
            or not 0 <= int(row) <= out.shape[0] - rows):
        which = "row one of its rows" if rows == 1 else f"[row, row + {rows}) rows of it"
        raise RuntimeError(f"dqo_eval.{who}: out must be a contiguous float32 [K,{width}] table and {which}")
    return out, int(row)


def _picture_bytes(W, H):
    lib = N.lib()
    n = lib.dqo_eval_picture_workspace_bytes(W, H)
    if n == 0:
        raise RuntimeError(f"dqo_eval: bad image size {W} x {H}")
    return n + lib.dqo_map_ssim_workspace_bytes(W, H)


def workspace(W, H, device):
    """The two workspaces of one evaluation at W x H as one uint8 tensor: dqo_eval_picture's (zero when first used, handed back ready by
    every call) followed by dqo_map_ssim_fwd_bwd's.  Calls that share one must be ordered on one stream."""
    return torch.zeros((_picture_bytes(W, H),), dtype=torch.uint8, device=device)


def _image(t, channels, H, W, dtype, name):
    if t.dim() == 2 and channels == 1:
        t = t[None]
    if tuple(t.shape) != (channels, H, W):
        raise RuntimeError(f"dqo_eval.eval_picture: {name} must be [{channels},{H},{W}], got {tuple(t.shape)}")
    return t.to(dtype).contiguous()  # (no copy, no launch, when it already is)


def eval_picture(render_output, gt_color, gt_depth, min_depth, max_depth, out=None, row=0, ssim=True, *, workspace_buffer=None,
                 render_header=None):
    """eval_picture (SLAM/eval.py:38-188) of one frame, on the device.

    render_output: the dict of dqo_harness.mapping.render / Renderer.render, or any dict with `render` [3,H,W], `depth` [1,H,W] and
    `depth_index_map` int32 [1,H,W].  gt_color [3,H,W] (frame.original_image), gt_depth [1,H,W] in metres (the reference's
    255 * frame.original_depth, :115), min_depth / max_depth: the valid range (:116).
    Returns the float32 [8] device row (names: ROW)
        0 psnr   1 color_loss   2 depth_loss   3 valid_pixel_ratio   4 ssim   5..7 mse of r, g, b
    — a new tensor, or out[row] of a caller-owned float32 [K,8] table, whose other rows are not touched.  Nothing is read back and the
    call does not synchronise; eval_picture_dict(row) does the single host read.  Identical images give psnr = +inf, a frame without a
    valid depth pixel depth_loss = NaN: the reference's values.  ssim=False leaves slot 4 alone (NaN in a new row).

    Slot 4 is the single-scale SSIM of utils/loss_utils.py:60-100 (dqo_map_ssim_fwd_bwd, value only).  The reference's `ssim` key is
    MS-SSIM (pytorch_msssim's `ms_ssim`): that is ms_ssim()'s row, which eval_picture_dict takes as `ms_row`.  LPIPS is lpips()'s row
    (`lpips_row`), on weights the caller brings.

    workspace_buffer: a tensor of workspace(W, H, device) the caller keeps (default: one per device and image size, kept by this
    module — calls that share it must be on one stream).  render_header: the geometry buffer of the forward that rendered the frame
    (uint8 tensor); a frame that overflowed its context then gets a row of NaN.  GPU tensors only: a CPU tensor raises RuntimeError."""
    render, depth, index = render_output["render"], render_output["depth"], render_output["depth_index_map"]
    N.require_gpu_op(render, depth, index, gt_color, gt_depth, out)
    lib, dev = N.lib(), render.device
    H, W = int(render.shape[-2]), int(render.shape[-1])
    f32 = torch.float32
    render, gt_color = _image(render, 3, H, W, f32, "render"), _image(gt_color, 3, H, W, f32, "gt_color")
    depth, gt_depth = _image(depth, 1, H, W, f32, "depth"), _image(gt_depth, 1, H, W, f32, "gt_depth")
    index = _image(index, 1, H, W, torch.int32, "depth_index_map")
    out, row = _table_row(out, row, 8, "eval_picture", dev)
    ws = _ws(workspace_buffer, dev, lambda: _picture_bytes(W, H), "picture", W, H)
    n_eval = lib.dqo_eval_picture_workspace_bytes(W, H)
    with torch.cuda.device(dev):
        stream = N.current_stream()
        if ssim:
            # dqo_map_ssim_fwd_bwd writes TWO floats (the value, weight * (1 - value)): into slots 4 and 5, BEFORE dqo_eval_picture writes
            # mse_r over slot 5 on the same stream — no staging buffer, no copy launch
            N.check(lib.dqo_map_ssim_fwd_bwd(W, H, N.ptr(render), N.ptr(gt_color), 0.0, out.data_ptr() + 4 * (8 * row + 4), None, 0, None,
                                             ws.data_ptr() + n_eval, ws.numel() - n_eval, stream))
        N.check(lib.dqo_eval_picture(W, H, N.ptr(render), N.ptr(gt_color), N.ptr(depth), N.ptr(gt_depth), N.ptr(index), float(min_depth),
                                     float(max_depth), N.ptr(render_header), out.data_ptr(), row, ws.data_ptr(), n_eval, stream))
    return out[row]


def _ms_ssim_bytes(W, H):
    n = N.lib().dqo_eval_ms_ssim_workspace_bytes(int(W), int(H))
    if n == 0:
        raise RuntimeError(f"dqo_eval.ms_ssim: bad image size {W} x {H}: both sides must be at least {MS_MIN_SIDE} (five levels of an "
                           "11-tap window)")
    return n


def ms_ssim_workspace(W, H, device):
    """dqo_eval_ms_ssim's workspace at W x H as a uint8 tensor (zero when first used, handed back ready by every call): the ticket words,
    the level means and the pooled levels 1..4 of both images."""
    return torch.zeros((_ms_ssim_bytes(W, H),), dtype=torch.uint8, device=device)


def ms_ssim(image, gt, out=None, row=0, *, workspace_buffer=None, render_header=None):
    """MS-SSIM of a rendered image against its target, on the device: the reference's eval_ssim (SLAM/eval.py:19-25) —
    pytorch_msssim.ms_ssim(image[None], gt[None], data_range=1.0, size_average=True), the `ssim` of eval_picture (:64).

    image, gt: [3,H,W], used as they are (no clamp); both sides above 160 (the library's assertion), else RuntimeError before any launch.
    Returns the float32 [20] device row (names: MS_ROW)
        0 ms_ssim   1..3 the value per channel   4 + 3 l + c the factor of level l, channel c, after the clamp at 0   19 unused (NaN)
    — a new tensor initialised to NaN, or out[row] of a caller-owned contiguous float32 [K,20] table, whose other rows are not touched.
    The factors are in the row on purpose: an error at one level shows at that level.  Nothing is read back and the call does not
    synchronise; a row is bitwise reproducible and the call can be captured in a graph.  The algorithm is pytorch_msssim's as its
    published source states it; the library does not exist on this platform, so no value here was recorded from it.

    workspace_buffer: a tensor of ms_ssim_workspace(W, H, device) the caller keeps (default: one per device and image size, kept by this
    module — calls that share it must be on one stream).  render_header: as eval_picture's — a frame that overflowed its context gets
    a row of NaN.  GPU tensors only: a CPU tensor raises RuntimeError."""
    N.require_gpu_op(image, gt, out)
    lib, dev = N.lib(), image.device
    H, W = int(image.shape[-2]), int(image.shape[-1])
    f32 = torch.float32
    image, gt = _image(image, 3, H, W, f32, "image"), _image(gt, 3, H, W, f32, "gt")
    if min(H, W) < MS_MIN_SIDE:
        raise RuntimeError(f"dqo_eval.ms_ssim: image size {W} x {H}: both sides must be at least {MS_MIN_SIDE} (the reference's library "
                           "asserts smaller_side > 160)")
    out, row = _table_row(out, row, 20, "ms_ssim", dev)
    ws = _ws(workspace_buffer, dev, lambda: _ms_ssim_bytes(W, H), "ms", W, H)
    with torch.cuda.device(dev):
        N.check(lib.dqo_eval_ms_ssim(W, H, N.ptr(image), N.ptr(gt), N.ptr(render_header), out.data_ptr(), row, ws.data_ptr(), ws.numel(),
                                     N.current_stream()))
    return out[row]


LPIPS_ROW = ("lpips", "d0", "d1", "d2", "d3", "d4", "unused6", "unused7")
LPIPS_MIN_SIDE = 31  # every AlexNet map needs a pixel
LPIPS_NET = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))  # Cin, Cout, kernel, stride, pad
LPIPS_NORMS = {"torchmetrics": N.CONSTANTS["DQO_LPIPS_NORM_TORCHMETRICS"], "lpips": N.CONSTANTS["DQO_LPIPS_NORM_LPIPS"]}
_LPIPS_FEATURES_OFFSET = N.CONSTANTS["DQO_LPIPS_FEATURES_OFFSET"]


def lpips_sizes(W, H):
    """The sides ((h0, w0), .., (h4, w4)) of the five feature maps of an H x W image: h0 = (H - 7) // 4 + 1 (11-tap, stride 4, pad 2),
    h1 = (h0 - 3) // 2 + 1, h2 = h3 = h4 = (h1 - 3) // 2 + 1 (the two 3 / 2 max-pools, floor mode; the other convolutions keep the side)."""
    def side(n):
        a = (int(n) - 7) // 4 + 1
        b = (a - 3) // 2 + 1
        c = (b - 3) // 2 + 1
        return a, b, c, c, c
    return tuple(zip(side(H), side(W)))


class LpipsWeights:
    """The weights of LPIPS' AlexNet, which the CALLER brings (nothing is shipped or fetched), packed once into the one buffer
    dqo_eval_lpips reads (include/dqo_raster.h states the layout): per layer W[k][co] with k = (kh * KW + kw) * Cin + ci — the k order is
    the accumulation order of a convolution output — then bias[Cout], then lin[Cout].

    conv_w: five [Cout,Cin,k,k] tensors (LPIPS_NET: 3 -> 64 k 11, 64 -> 192 k 5, 192 -> 384 k 3, 384 -> 256 k 3, 256 -> 256 k 3), conv_b: five
    [Cout] biases, lin: five [Cout] (or [1,Cout,1,1]) vectors of the linear heads.  Any other shape raises RuntimeError.  The packing is
    torch ops on the tensors' own device and not hot; `packed` is the float32 [2 470 848] result on `device`."""

    def __init__(self, conv_w, conv_b, lin, device):
        if len(conv_w) != 5 or len(conv_b) != 5 or len(lin) != 5:
            raise RuntimeError("dqo_eval.LpipsWeights: five convolution weights, five biases and five lin vectors")
        parts = []
        for l, (cin, cout, k, _, _) in enumerate(LPIPS_NET):
            w, b, v = conv_w[l], conv_b[l], lin[l]
            if tuple(w.shape) != (cout, cin, k, k):
                raise RuntimeError(f"dqo_eval.LpipsWeights: conv_w[{l}] must be [{cout},{cin},{k},{k}], got {tuple(w.shape)}")
            if tuple(b.shape) != (cout,):
                raise RuntimeError(f"dqo_eval.LpipsWeights: conv_b[{l}] must be [{cout}], got {tuple(b.shape)}")
            if tuple(v.shape) not in ((cout,), (1, cout, 1, 1)):
                raise RuntimeError(f"dqo_eval.LpipsWeights: lin[{l}] must be [{cout}] or [1,{cout},1,1], got {tuple(v.shape)}")
            parts += [w.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(-1), b.detach().to(torch.float32).reshape(-1),
                      v.detach().to(torch.float32).reshape(-1)]
        self.packed = torch.cat([t.to(device) for t in parts]).contiguous()
        self.device = self.packed.device

    @classmethod
    def from_state_dicts(cls, alexnet_state, lin_state, device=None):
        """From torchvision's AlexNet state dict (`features.{0,3,6,8,10}.{weight,bias}`) and the `lpips` package's linear heads
        (`lin{0..4}.model.1.weight`, [1,Cout,1,1]): the key names of the published sources.  The tensor constructor is the contract.
        device None: where the first convolution's weight is."""
        idx = (0, 3, 6, 8, 10)
        device = alexnet_state["features.0.weight"].device if device is None else device
        return cls([alexnet_state[f"features.{i}.weight"] for i in idx], [alexnet_state[f"features.{i}.bias"] for i in idx],
                   [lin_state[f"lin{l}.model.1.weight"] for l in range(5)], device)


def _lpips_bytes(W, H):
    n = N.lib().dqo_eval_lpips_workspace_bytes(int(W), int(H))
    if n == 0:
        raise RuntimeError(f"dqo_eval.lpips: bad image size {W} x {H}: both sides must be at least {LPIPS_MIN_SIDE} (every AlexNet map "
                           "needs a pixel)")
    return n


def lpips_workspace(W, H, device):
    """dqo_eval_lpips' workspace at W x H as a uint8 tensor (its ticket words zero when first used, handed back at zero by every call): the
    five feature maps of both images, the two pooled maps and the reduction's partials."""
    return torch.zeros((_lpips_bytes(W, H),), dtype=torch.uint8, device=device)


def lpips(image, gt, weights, out=None, row=0, *, norm="torchmetrics", workspace_buffer=None, render_header=None):
    """LPIPS of a rendered image against its target, on the device: the reference's `lpips` (SLAM/eval.py:28-30, :65-68) —
    LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True) of clamp(gt, 0, 1) and clamp(image, 0, 1), a batch of one — on
    `weights`, a LpipsWeights the caller made from ITS AlexNet and linear heads.  The number is the reference's only on the reference's
    weights.

    image, gt: [3,H,W] (clamped to [0, 1] in the kernel); both sides at least 31, else RuntimeError before any launch.
    Returns the float32 [8] device row (names: LPIPS_ROW)
        0 lpips   1..5 the layer terms d_0 .. d_4 (lpips is their sum)   6, 7 unused (NaN)
    — a new tensor initialised to NaN, or out[row] of a caller-owned contiguous float32 [K,8] table, whose other rows are not touched.
    The layer terms are in the row on purpose: an error at one layer shows at that layer.  norm: "torchmetrics" (a / sqrt(1e-8 + sum a^2),
    what the reference calls) or "lpips" (a / (sqrt(sum a^2) + 1e-10), the `lpips` package's form).  Nothing is read back and the call does
    not synchronise; a row is bitwise reproducible, symmetric in (image, gt), and the call can be captured in a graph.  The five
    convolutions run on the f32 matrix cores, an output element one fmaf chain in the packed k order (include/dqo_raster.h states every
    step).  The algorithm is the one the published sources of `lpips` and `torchmetrics` state; neither package exists on this platform,
    so no value here was recorded from them (tests/lpips_oracle.py restates the steps).

    workspace_buffer: a tensor of lpips_workspace(W, H, device) the caller keeps (default: one per device and image size, kept by this
    module — calls that share it must be on one stream); lpips_feature_view reads the maps the call left in it.  render_header: as
    eval_picture's — a frame that overflowed its context gets a row of NaN.  GPU tensors only: a CPU tensor raises RuntimeError."""
    if not isinstance(weights, LpipsWeights):
        raise RuntimeError("dqo_eval.lpips: weights must be a LpipsWeights")
    N.require_gpu_op((image, weights.packed), gt, out)
    lib, dev = N.lib(), image.device
    if weights.packed.device != dev:
        raise RuntimeError(f"dqo_eval.lpips: the weights are on {weights.packed.device}, the image on {dev}")
    if norm not in LPIPS_NORMS:
        raise RuntimeError(f"dqo_eval.lpips: norm must be one of {sorted(LPIPS_NORMS)}, got {norm!r}")
    H, W = int(image.shape[-2]), int(image.shape[-1])
    f32 = torch.float32
    image, gt = _image(image, 3, H, W, f32, "image"), _image(gt, 3, H, W, f32, "gt")
    if min(H, W) < LPIPS_MIN_SIDE:
        raise RuntimeError(f"dqo_eval.lpips: image size {W} x {H}: both sides must be at least {LPIPS_MIN_SIDE} (every AlexNet map needs a "
                           "pixel)")
    out, row = _table_row(out, row, 8, "lpips", dev)
    ws = _ws(workspace_buffer, dev, lambda: _lpips_bytes(W, H), "lpips", W, H)
    with torch.cuda.device(dev):
        N.check(lib.dqo_eval_lpips(W, H, N.ptr(image), N.ptr(gt), N.ptr(weights.packed), LPIPS_NORMS[norm], N.ptr(render_header), out.data_ptr(),
                                   row, ws.data_ptr(), ws.numel(), N.current_stream()))
    return out[row]


def lpips_feature_view(workspace_buffer, W, H, layer):
    """Feature map `layer` (0..4) the last lpips call left in its workspace: float32 [2,h,w,C], pixel-major, 0 = image, 1 = gt
    (lpips_sizes; C = LPIPS_NET[layer][1]).  A view, for tests and inspection: the next call overwrites it."""
    sizes, off = lpips_sizes(W, H), _LPIPS_FEATURES_OFFSET
    for l in range(int(layer)):
        off += (4 * 2 * sizes[l][0] * sizes[l][1] * LPIPS_NET[l][1] + 255) // 256 * 256
    (h, w), C = sizes[int(layer)], LPIPS_NET[int(layer)][1]
    return workspace_buffer[off:off + 4 * 2 * h * w * C].view(torch.float32).view(2, h, w, C)


def eval_picture_dict(row_tensor, ms_row=None, lpips_row=None):
    """The reference's `losses` dict (eval.py:178-185) from a device row — ONE host read.  Keys: valid_pixel_ratio, depth_loss,
    normal_loss (0, as eval.py:167), psnr, ssim, plus color_loss.
    ms_row=None: `ssim` is slot 4, the single-scale SSIM (see eval_picture).  With ms_ssim()'s row of the same frame, `ssim` is that
    row's slot 0 — the reference's quantity — and the single-scale value moves to `ssim_single_scale`.  With lpips()'s row of the same
    frame (lpips_row) the dict gains `lpips`, that row's slot 0; without it there is no such key.  Rows that are views of one tensor
    (one storage, at most 4 096 floats apart) are read in one transfer of the span that holds them all; otherwise there is one read per row."""
    if ms_row is None and lpips_row is None:
        v = row_tensor.detach().reshape(-1)[:8].cpu().tolist()
        return {"valid_pixel_ratio": v[3], "depth_loss": v[2], "normal_loss": 0, "psnr": v[0], "ssim": v[4], "color_loss": v[1]}
    want = [(row_tensor.detach(), 8)] + [(t.detach(), 1) for t in (ms_row, lpips_row) if t is not None]
    r = want[0][0]
    lo, hi = min(t.storage_offset() for t, _ in want), max(t.storage_offset() + n for t, n in want)
    if (all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n
            and t.untyped_storage().data_ptr() == r.untyped_storage().data_ptr() for t, n in want) and hi - lo <= 4096):
        span = torch.as_strided(r, (hi - lo,), (1,), lo).cpu().tolist()
        got = [span[t.storage_offset() - lo:t.storage_offset() - lo + n] for t, n in want]
    else:
        got = [t.reshape(-1)[:n].cpu().tolist() for t, n in want]
    v = got[0]
    d = {"valid_pixel_ratio": v[3], "depth_loss": v[2], "normal_loss": 0, "psnr": v[0], "ssim": v[4], "color_loss": v[1]}
    if ms_row is not None:
        d["ssim"], d["ssim_single_scale"] = got[1][0], v[4]
    if lpips_row is not None:
        d["lpips"] = got[-1][0]
    return d


def _points(t, name):
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"dqo_eval: {name} must be [N,3], got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()  # (no copy, no launch, when it already is)


def _keep(t, n, name):
    if t is None:
        return None
    if t.numel() != n or t.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError(f"dqo_eval: {name} must be a uint8 / bool mask of {n} rows")
    return t.reshape(-1).contiguous().view(torch.uint8)


def _xform(t, dev, name):
    """A [3,4] or [4,4] transform (tensor, numpy array or nested list) as 12 floats on the device; None stays None."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if tuple(t.shape) not in ((3, 4), (4, 4)):
        raise RuntimeError(f"dqo_eval: {name} must be [3,4] or [4,4], got {tuple(t.shape)}")
    if torch.is_tensor(t) and t.is_cuda:
        return t[:3].to(torch.float32).contiguous()
    return t[:3].to(torch.float32).contiguous().to(dev)  # (a host transform: one small upload, no read)


def nearest(query, ref, query_keep=None, ref_keep=None, query_transform=None, ref_transform=None, want_idx=True, workspace_buffer=None):
    """The exact nearest reference of every query, both sets large (dqo_nn1): query [Q,3], ref [R,3] -> (dist2 float32 [Q], idx int32 [Q]
    or None).  dist2 is the smallest float32 dx*dx + dy*dy + dz*dz over the kept references, idx a reference attaining it (ties:
    arbitrary).  *_keep: uint8 / bool masks, 0 = the row is neither found nor searched for (a dropped query: FLT_MAX / -1); no kept
    reference: FLT_MAX / -1 everywhere.  *_transform: [3,4] / [4,4], applied to the rows as they are loaded.  No host read, no
    synchronisation; workspace_buffer: a uint8 tensor of dqo_nn1_workspace_bytes(Q, R) the caller keeps (default: one per device and
    size, kept by this module — calls that share it must be on one stream)."""
    return _nearest(False, query, query_keep, ref, ref_keep, query_transform, ref_transform, want_idx, workspace_buffer)


OBJECTS = 64  # object ids of a grouped call: [0, OBJECTS); any other id = the row has no object


def _group(t, n, dev, name):
    """One object id per row as a contiguous int32 [n] tensor on the device (an int32 tensor goes in as it is)."""
    if not torch.is_tensor(t) or t.numel() != n or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f"dqo_eval: {name} must be an integer tensor with one object id for each of the {n} rows")
    if t.numel() > 0 and t.device != dev:
        raise RuntimeError(f"dqo_eval: {name} must be on {dev}")
    return t.reshape(-1).to(torch.int32).contiguous()


def nearest_grouped(query, query_group, ref, ref_group, query_transform=None, ref_transform=None, want_idx=True, workspace_buffer=None):
    """nearest() for up to 64 objects in one search (dqo_nn1_grouped): query [Q,3] with query_group [Q], ref [R,3] with ref_group [R] ->
    (dist2 float32 [Q], idx int32 [Q] or None).  A group id in [0, 64) is the row's object, any other value (-1, 64, ...) means the row
    has none and takes no part on either side.  dist2 is the smallest float32 dx*dx + dy*dy + dz*dz over the references of the query's
    own group, idx one of them attaining it; FLT_MAX / -1 for a query without a group or whose group has no reference.  Bit for bit
    nearest() with query_keep = (query_group == g) and ref_keep = (ref_group == g), for every g — from one build of the reference set,
    one sort of the queries and one scan.  Transforms, workspace (dqo_nn1_grouped_workspace_bytes(Q, R)) and contract as nearest():
    no host read, no synchronisation."""
    return _nearest(True, query, query_group, ref, ref_group, query_transform, ref_transform, want_idx, workspace_buffer)


def _nearest(grouped, query, q_rows, ref, r_rows, query_transform, ref_transform, want_idx, workspace_buffer):
    """nearest (q_rows, r_rows: the keep masks) and nearest_grouped (the group ids): one search, one workspace key."""
    N.require_gpu_op((query, ref), q_rows, r_rows)
    lib, dev = N.lib(), query.device
    query, ref = _points(query, "query"), _points(ref, "ref")
    Q, R = int(query.shape[0]), int(ref.shape[0])
    if grouped:
        qr, rr = _group(q_rows, Q, dev, "query_group"), _group(r_rows, R, dev, "ref_group")
    else:
        qr, rr = _keep(q_rows, Q, "query_keep"), _keep(r_rows, R, "ref_keep")
    qx, rx = _xform(query_transform, dev, "query_transform"), _xform(ref_transform, dev, "ref_transform")
    n = (lib.dqo_nn1_grouped_workspace_bytes if grouped else lib.dqo_nn1_workspace_bytes)(Q, R)
    if n == 0:
        raise RuntimeError(f"dqo_eval.nearest{'_grouped' if grouped else ''}: bad sizes {Q}, {R} (at most 2^25 - 1 rows per set)")
    ws = _ws(workspace_buffer, dev, n, "nn1", Q, R)
    dist2 = torch.empty((Q,), dtype=torch.float32, device=dev)
    idx = torch.empty((Q,), dtype=torch.int32, device=dev) if want_idx else None
    if Q > 0 or not grouped:  # (the grouped C entry wants the ids even when R = 0; an empty tensor has no pointer)
        with torch.cuda.device(dev):
            N.check((lib.dqo_nn1_grouped if grouped else lib.dqo_nn1)(Q, N.ptr(query), N.ptr(qr), R, N.ptr(ref), N.ptr(rr), N.ptr(qx), N.ptr(rx),
                                                                      N.ptr(dist2), N.ptr(idx), ws.data_ptr(), ws.numel(), N.current_stream()))
    return dist2, idx


DENSIFY_HEADER = ("kept_rows", "N_lo", "N_hi", "n", "M", "threshold_key", "frame", "zero")
DENSIFY_FRAMES = {"reference": N.CONSTANTS["DQO_DENSIFY_FRAME_REFERENCE"], "surfel": N.CONSTANTS["DQO_DENSIFY_FRAME_SURFEL"]}


def densify_theta(circle_num, seed=0):
    """The reference's angles (gaussian_pointcloud.py:79): torch.rand(1, circle_num) * torch.pi * 2 from a CPU generator seeded with
    `seed`, as a float32 [circle_num] CPU tensor."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return (torch.rand(1, int(circle_num), generator=g) * torch.pi * 2).reshape(-1)


def densify(xyz, scaling_raw, rotation_raw, sigma=1, circle_num=30, levels=5, theta=None, keep=None, sample_nums=None, seed=0,
            frame="reference", want_normals=True, want_index=False, workspace_buffer=None):
    """GaussianPointCloud.densify(sigma, circle_num, levels) (SLAM/gaussian_pointcloud.py:67-130) of the rows `keep` names, and of its
    N = M * (kept rows) points (M = circle_num * levels * sigma per row) the n = min(N, sample_nums) that eval_pcd would evaluate
    (SLAM/eval.py:244) — one device step that never holds the densified cloud (dqo_surfel_densify, include/dqo_raster.h).

    xyz [P,3], scaling_raw [P,3] (log scales), rotation_raw [P,4] (r, x, y, z): contiguous float32 device tensors, the map's raw
    parameters.  theta: [circle_num] angles (None: densify_theta(circle_num, seed), the reference's torch.rand on the CPU); their float32
    torch.cos / torch.sin are formed on the CPU and uploaded, so the kernel calls no device cosine.  keep: uint8 / bool [P], 0 = the row
    gives no point.  sample_nums None: cap = P * M, every point of the kept rows comes out; else cap = min(P * M, sample_nums).
    frame "reference": the points the reference writes to pcd_densify.ply — its matmul has the plane vectors as ROWS, so a rotated
    surfel's points do not lie in its plane; "surfel": mean + x p0 + z p1, the evident intent.
    Returns dict(points [cap,3], normals [cap,3] | None, index int64 [cap] | None (the virtual index v = row * M + column of every
    point), keep uint8 [cap] (1 for the first n rows, 0 behind: eval_pcd's `rec_keep`), header int32 [8] (DENSIFY_HEADER)).  Rows of
    points / normals / index at and behind n are not written.  The subsample takes the n smallest keys of csrc/dqo_sample_hash.h (draw
    3) in ascending v: not numpy's stream, the same distribution.  Nothing is read back.  The C entry does not synchronise; this
    function forms the cos / sin table on the CPU and uploads it from pageable memory on every call, a small copy the host waits for
    (it is inside every time measured through this function).
    GPU tensors only: a CPU tensor raises RuntimeError."""
    N.require_gpu_op((xyz, scaling_raw, rotation_raw), keep)
    lib, dev = N.lib(), xyz.device
    P = int(xyz.shape[0]) if xyz.dim() == 2 else -1
    for t, w, name in ((xyz, 3, "xyz"), (scaling_raw, 3, "scaling_raw"), (rotation_raw, 4, "rotation_raw")):
        if t.dim() != 2 or tuple(t.shape) != (P, w) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"dqo_eval.densify: {name} must be a contiguous float32 [{max(P, 0)},{w}] tensor on {dev}, got "
                               f"{t.dtype} {tuple(t.shape)} on {t.device}")
    if frame not in DENSIFY_FRAMES:
        raise RuntimeError(f"dqo_eval.densify: frame must be one of {sorted(DENSIFY_FRAMES)}, got {frame!r}")
    sigma, circle_num, levels = int(sigma), int(circle_num), int(levels)
    nbytes = lib.dqo_surfel_densify_workspace_bytes(P, circle_num, levels, sigma)
    if nbytes == 0:
        raise RuntimeError(f"dqo_eval.densify: bad sizes P = {P}, (sigma, circle_num, levels) = ({sigma}, {circle_num}, {levels}): each at "
                           "least 1, circle_num at most 1024, at most 65535 points per row and fewer than 2^32 in all")
    M = circle_num * levels * sigma
    if sample_nums is not None and int(sample_nums) < 1:
        raise RuntimeError(f"dqo_eval.densify: sample_nums must be at least 1, got {sample_nums}")
    cap = P * M if sample_nums is None else min(P * M, int(sample_nums))
    rk = _keep(keep, P, "keep")
    if rk is not None and rk.device != dev:
        raise RuntimeError(f"dqo_eval.densify: keep must be on {dev}")
    if theta is None:
        theta = densify_theta(circle_num, seed)
    theta = torch.as_tensor(theta).detach().to("cpu", torch.float32).reshape(-1)
    if theta.numel() != circle_num:
        raise RuntimeError(f"dqo_eval.densify: theta must have circle_num = {circle_num} entries, got {theta.numel()}")
    circle_cs = torch.cat([torch.cos(theta), torch.sin(theta)]).contiguous().to(dev)  # (gaussian_pointcloud.py:104-105, on the CPU)
    ws = _ws(workspace_buffer, dev, nbytes, "densify", P, M)
    points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((cap, 3), dtype=torch.float32, device=dev) if want_normals else None
    index = torch.empty((cap,), dtype=torch.int64, device=dev) if want_index else None
    keep_out = torch.empty((cap,), dtype=torch.uint8, device=dev)
    header = torch.empty((8,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.dqo_surfel_densify(P, N.ptr(xyz), N.ptr(scaling_raw), N.ptr(rotation_raw), N.ptr(rk), circle_num, levels, sigma,
                                       N.ptr(circle_cs), DENSIFY_FRAMES[frame], int(seed) & (2 ** 64 - 1), cap, N.ptr(points), N.ptr(normals),
                                       N.ptr(index), N.ptr(keep_out), N.ptr(header), ws.data_ptr(), ws.numel(), N.current_stream()))
    return dict(points=points, normals=normals, index=index, keep=keep_out, header=header)


MESH_HEADER = ("n", "F", "bad_index_faces", "zero_area_faces", "quantum_exponent", "total_lo", "total_hi", "zero")
MESH_SCAN_BLOCK = N.CONSTANTS["DQO_MESH_SCAN_BLOCK"]  # faces per block of the table's scan


def mesh_sample_workspace(F, count, device):
    """dqo_mesh_sample's workspace for a mesh of F faces and `count` samples as a uint8 tensor (zero when first used, handed back ready
    by every call)."""
    n = N.lib().dqo_mesh_sample_workspace_bytes(int(F), int(count))
    if n == 0:
        raise RuntimeError(f"dqo_eval.sample_surface: bad sizes F = {F}, count = {count}: each in [1, 2^25 - 1]")
    return torch.zeros((n,), dtype=torch.uint8, device=device)


def mesh_cum_view(workspace_buffer, F):
    """The cumulative table the last sample_surface call left in its workspace: int64 [F], cum[f] = the quanta of faces 0..f (below
    2^61).  A view, for tests and inspection: the next call overwrites it."""
    n = (8 * int(F) + 255) // 256 * 256  # (the workspace's last block)
    return workspace_buffer[workspace_buffer.numel() - n:].view(torch.int64)[:int(F)]


def _sample_outs(count, want_face_index, dev):
    """The sampler's outputs, new: (dict(points, face_index | None, keep, header), their pointers in the entries' order)."""
    o = dict(points=torch.empty((count, 3), dtype=torch.float32, device=dev),
             face_index=torch.empty((count,), dtype=torch.int32, device=dev) if want_face_index else None,
             keep=torch.empty((count,), dtype=torch.uint8, device=dev), header=torch.empty((8,), dtype=torch.int32, device=dev))
    return o, [N.ptr(t) for t in o.values()]


def sample_surface(vertices, faces, count, seed=0, want_face_index=False, workspace_buffer=None):
    """trimesh.sample.sample_surface(mesh, count) (SLAM/eval.py:247) on the device: `count` points on the surface of a triangle mesh, a
    face picked in proportion to its area, a uniform point inside it (dqo_mesh_sample, include/dqo_raster.h, states every statement).

    vertices [V,3] float32, faces [F,3] int32 (dqo_ply.read_mesh_ply's arrays as device tensors), contiguous; count and F in
    [1, 2^25 - 1]; seed: 64 bits — the draws are the key rule of csrc/dqo_sample_hash.h (draws 4-7), not numpy's stream.  A face with
    an index outside [0, V), or of zero or non-finite area, gets no sample; both are counted in the header.
    Returns dict(points float32 [count,3], face_index int32 [count] | None, keep uint8 [count] (1 everywhere, or all 0 when the mesh
    has no area and no point was written: eval_pcd's `gt_keep`), header int32 [8] (MESH_HEADER)).  Nothing is read back, the call does
    not synchronise and can be captured in a graph; the same arguments give the same bits.
    workspace_buffer: a tensor of mesh_sample_workspace(F, count, device) the caller keeps (default: one per device and sizes, kept by
    this module — calls that share it must be on one stream).  GPU tensors only: a CPU tensor raises RuntimeError."""
    N.require_gpu_op((vertices, faces), workspace_buffer)
    lib, dev = N.lib(), vertices.device
    for t, dt, name in ((vertices, torch.float32, "vertices"), (faces, torch.int32, "faces")):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"dqo_eval.sample_surface: {name} must be a contiguous {dt} [n,3] tensor on {dev}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}")
    V, F, count = int(vertices.shape[0]), int(faces.shape[0]), int(count)
    nbytes = lib.dqo_mesh_sample_workspace_bytes(F, count) if V >= 1 else 0
    if nbytes == 0:
        raise RuntimeError(f"dqo_eval.sample_surface: bad sizes V = {V}, F = {F}, count = {count}: at least one vertex, F and count in "
                           "[1, 2^25 - 1]")
    ws = _ws(workspace_buffer, dev, nbytes, "mesh", F, count)
    o, ptrs = _sample_outs(count, want_face_index, dev)
    with torch.cuda.device(dev):
        N.check(lib.dqo_mesh_sample(V, N.ptr(vertices), F, N.ptr(faces), count, int(seed) & (2 ** 64 - 1), *ptrs, ws.data_ptr(), ws.numel(),
                                    N.current_stream()))
    return o


def _pcd_bytes(n_gt, n_rec, query="dqo_eval_pcd_workspace_bytes"):
    n = getattr(N.lib(), query)(int(n_gt), int(n_rec))
    if n == 0:
        raise RuntimeError(f"dqo_eval: bad point counts {n_gt}, {n_rec} (at most 2^25 - 1 rows per set)")
    return n


def pcd_workspace(n_gt, n_rec, device):
    """dqo_eval_pcd's workspace for these sizes as a uint8 tensor (zero when first used, handed back ready by every call)."""
    return torch.zeros((_pcd_bytes(n_gt, n_rec),), dtype=torch.uint8, device=device)


def eval_pcd(gt_points, rec_points, dist_thres=(0.03,), transform=None, gt_keep=None, rec_keep=None, out=None, row=0, workspace_buffer=None):
    """eval_pcd (SLAM/eval.py:190-282) of a reconstruction against a ground-truth point set, on the device.

    gt_points [G,3]: the ground-truth points (the reference samples them from the mesh with trimesh, :247: sample_surface, whose
    `keep` is gt_keep); rec_points [P,3]: the reconstructed points; transform: [3,4] / [4,4], applied to rec_points
    (rec_pc.transform(transform), :241); dist_thres: up to 8 distances in metres (:229, :263); gt_keep / rec_keep: uint8 / bool masks,
    0 = the row takes no part (the mapper's row buffers go in as stored).
    Returns the float32 [32] device row (names: PCD_ROW)
        0 accuracy (cm)   1 completion (cm)   2 chamfer (m)   3 n_thres   4+3t P   5+3t R   6+3t F1 of threshold t   (the rest NaN)
    — a new tensor, or out[row] of a caller-owned float32 [K,32] table, whose other rows are not touched.  Nothing is read back and the
    call does not synchronise; eval_pcd_dict does the single host read.  An empty (kept) set on either side gives a row of NaN; a
    threshold no distance is under gives F1 = NaN, as numpy's division in the reference.  A row is bitwise reproducible.

    workspace_buffer: a tensor of pcd_workspace(G, P, device) the caller keeps (default: one per device and sizes, kept by this module —
    calls that share it must be on one stream).  GPU tensors only: a CPU tensor raises RuntimeError."""
    N.require_gpu_op((gt_points, rec_points), gt_keep, rec_keep, out)
    lib, dev = N.lib(), rec_points.device
    gt, rec = _points(gt_points, "gt_points"), _points(rec_points, "rec_points")
    G, P = int(gt.shape[0]), int(rec.shape[0])
    gk, rk = _keep(gt_keep, G, "gt_keep"), _keep(rec_keep, P, "rec_keep")
    xf = _xform(transform, dev, "transform")
    thres = [float(t) for t in dist_thres]
    if len(thres) > PCD_THRES_MAX:
        raise RuntimeError(f"dqo_eval.eval_pcd: at most {PCD_THRES_MAX} thresholds, got {len(thres)}")
    out, row = _table_row(out, row, 32, "eval_pcd", dev, fresh=torch.empty)
    ws = _ws(workspace_buffer, dev, lambda: _pcd_bytes(G, P), "pcd", G, P)
    with torch.cuda.device(dev):
        N.check(lib.dqo_eval_pcd(G, N.ptr(gt), N.ptr(gk), P, N.ptr(rec), N.ptr(rk), N.ptr(xf), len(thres), (ctypes.c_float * len(thres))(*thres),
                                 out.data_ptr(), row, ws.data_ptr(), ws.numel(), N.current_stream()))
    return out[row]


def eval_pcd_dict(row_tensor, dist_thres=(0.03,)):
    """The reference's `results` dict (eval.py:263-281) from a device row — ONE host read.  Keys: accuracy, completion (cm),
    "P (< th)", "R (< th)", "F1 (< th)" for every th of dist_thres (the thresholds the row was made with: a row holds their count, not
    their values), plus chamfer (metres), which the reference only prints (:253-254)."""
    v = row_tensor.detach().reshape(-1)[:32].cpu().tolist()
    thres = list(dist_thres)
    if v[3] == v[3] and int(v[3]) != len(thres):
        raise RuntimeError(f"dqo_eval.eval_pcd_dict: the row was made with {int(v[3])} thresholds, got {len(thres)}")
    results = {"accuracy": v[0], "completion": v[1]}
    for name, off in (("P", 4), ("R", 5), ("F1", 6)):  # (the reference's order: every P, every R, every F1 — :279-281)
        for t, th in enumerate(thres):
            results["{} (< {})".format(name, th)] = v[off + 3 * t]
    results["chamfer"] = v[2]
    return results


def _pcd_objects_bytes(n_gt, n_rec):
    return _pcd_bytes(n_gt, n_rec, "dqo_eval_pcd_grouped_workspace_bytes")


def pcd_objects_workspace(n_gt, n_rec, device):
    """dqo_eval_pcd_grouped's workspace for these sizes as a uint8 tensor (zero when first used, handed back ready by every call)."""
    return torch.zeros((_pcd_objects_bytes(n_gt, n_rec),), dtype=torch.uint8, device=device)


def eval_pcd_objects(gt_points, gt_object, rec_points, rec_object, dist_thres=(0.01,), transform=None, out=None, row=0, workspace_buffer=None):
    """The per-object geometry numbers of the reference (metric_obj.py:169-236: eval_pcd of every object's stable cloud against that
    object's own ground-truth mesh, dist_threshs=[0.01]) for up to 64 objects in one call (dqo_eval_pcd_grouped): two grouped searches
    and one reduction launch, instead of one eval_pcd with keep masks per object.

    gt_points [G,3] with gt_object [G], rec_points [P,3] with rec_object [P]: an integer id per row, [0, 64) = the row's object, any
    other value (-1, 64, ...) = none, the row takes no part; transform: applied to rec_points; dist_thres: up to 8 distances in metres.
    Returns a float32 [64,32] device table — row g is eval_pcd's row (PCD_ROW) of object g's rows on both sides, 32 NaN for an object
    without a row on either side — a new tensor, or rows [row, row + 64) of a caller-owned contiguous float32 [K,32] table, whose other
    rows are not touched.  Nothing is read back, the call does not synchronise and can be captured in a graph; a table is bitwise
    reproducible.  eval_pcd_objects_dict does the single host read.

    workspace_buffer: a tensor of pcd_objects_workspace(G, P, device) the caller keeps (default: one per device and sizes, kept by this
    module — calls that share it must be on one stream).  GPU tensors only: a CPU tensor raises RuntimeError."""
    N.require_gpu_op((gt_points, rec_points), gt_object, rec_object, out)
    lib, dev = N.lib(), rec_points.device
    gt, rec = _points(gt_points, "gt_points"), _points(rec_points, "rec_points")
    G, P = int(gt.shape[0]), int(rec.shape[0])
    gg, rg = _group(gt_object, G, dev, "gt_object"), _group(rec_object, P, dev, "rec_object")
    xf = _xform(transform, dev, "transform")
    thres = [float(t) for t in dist_thres]
    if len(thres) > PCD_THRES_MAX:
        raise RuntimeError(f"dqo_eval.eval_pcd_objects: at most {PCD_THRES_MAX} thresholds, got {len(thres)}")
    out, row = _table_row(out, row, 32, "eval_pcd_objects", dev, rows=OBJECTS, fresh=torch.empty)
    ws = _ws(workspace_buffer, dev, lambda: _pcd_objects_bytes(G, P), "pcd_objects", G, P)
    with torch.cuda.device(dev):
        N.check(lib.dqo_eval_pcd_grouped(G, N.ptr(gt), N.ptr(gg), P, N.ptr(rec), N.ptr(rg), N.ptr(xf), len(thres),
                                         (ctypes.c_float * len(thres))(*thres), out.data_ptr(), int(out.shape[0]), row, ws.data_ptr(),
                                         ws.numel(), N.current_stream()))
    return out[row:row + OBJECTS]


def eval_pcd_objects_dict(table, dist_thres=(0.01,)):
    """{object id: eval_pcd_dict's dict} from eval_pcd_objects' [64,32] table, for the rows that are not all NaN (the objects with rows on
    both sides), ids ascending — ONE host read."""
    if tuple(table.shape) != (OBJECTS, 32):
        raise RuntimeError(f"dqo_eval.eval_pcd_objects_dict: a [{OBJECTS},32] table, got {tuple(table.shape)}")
    host = table.detach().to("cpu", torch.float32)
    return {g: eval_pcd_dict(host[g], dist_thres) for g in range(OBJECTS) if not bool(torch.isnan(host[g]).all())}


def object_seed(seed, obj):
    """The seed of object `obj`'s draw in sample_surface_objects: (seed + 0x9E3779B97F4A7C15 * (obj + 1)) mod 2^64 — a different stream
    per object, a pure function of the two."""
    return (int(seed) + 0x9E3779B97F4A7C15 * (int(obj) + 1)) & (2 ** 64 - 1)


def sample_surface_objects(meshes, count, seed=0):
    """The ground truth of the per-object evaluation: `count` points on the surface of every object's mesh (metric_obj.py evaluates each
    object against its own mesh with sample_nums points).  meshes = {object id in [0, 64): (vertices [V,3] float32, faces [F,3] int32)},
    device tensors.  Returns (points float32 [n,3], object int32 [n]), n = count * len(meshes), ids ascending: each object's part is
    exactly sample_surface(vertices, faces, count, seed=object_seed(seed, id))["points"], and the rows its `keep` drops (a mesh without
    area) get object -1 — eval_pcd_objects' gt_points / gt_object.  Nothing is read back."""
    ids = sorted(int(g) for g in meshes)
    if not ids or ids[0] < 0 or ids[-1] >= OBJECTS:
        raise RuntimeError(f"dqo_eval.sample_surface_objects: object ids must be in [0, {OBJECTS}), got {ids}")
    points, objects = [], []
    for g in ids:
        v, f = meshes[g]
        s = sample_surface(v, f, count, seed=object_seed(seed, g))
        points.append(s["points"])
        objects.append(torch.where(s["keep"] != 0, g, -1).to(torch.int32))
    return torch.cat(points), torch.cat(objects)


def _positions(t, name):
    """(tensor kept alive, pointer, doubles between points, doubles between components, N) of a float64 [N,3] or [N,4,4] GPU tensor:
    a view's strides are used as they are — the translation column of a pose stack is read in place."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
    if t.dtype != torch.float64:
        raise RuntimeError(f"dqo_eval.eval_ate: {name} must be float64, got {t.dtype}")
    if t.dim() == 3 and tuple(t.shape[1:]) == (4, 4):
        t = t[:, :3, 3]
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise RuntimeError(f"dqo_eval.eval_ate: {name} must be [N,3] positions or [N,4,4] poses, got {tuple(t.shape)}")
    if t.stride(0) < 0 or t.stride(1) < 0:
        t = t.contiguous()
    return t, t.data_ptr(), int(t.stride(0)), int(t.stride(1)), int(t.shape[0])


def eval_ate(pose_es, pose_gt, out=None, fit=None, workspace_buffer=None):
    """The ATE curve of Tracker.eval_total_ate (SLAM/multiprocess/tracker.py:341-346) on the device, in one launch (dqo_eval_ate,
    csrc/map_traj.hip): returns float64 [N] with out[i-1] = Tracker.eval_ate(pose_es, pose_gt, i) (:426-430) — the RMSE in centimetres
    after Horn's alignment of the first i ground-truth positions onto the first i estimated ones (eval_ate, SLAM/utils.py:486-532).

    pose_es, pose_gt: float64 GPU tensors, [N,3] positions or [N,4,4] poses (their translation column is read in place).  out: a
    contiguous float64 [N] tensor to fill; fit: a contiguous float64 [12] tensor that receives rot (row-major) and trans of the full
    trajectory's alignment.  Nothing is read back and the call does not synchronise; eval_ate_dict does the single host read.  The
    reference runs one alignment per prefix with a Python loop over its points.  A curve is bitwise reproducible.

    workspace_buffer: a uint8 tensor of at least dqo_eval_ate_workspace_bytes(N) bytes the caller keeps (default: one per device and N,
    kept by this module — calls that share it must be on one stream); on return it holds every prefix's alignment, [N,12] float64."""
    es, es_p, es_s, es_c, n = _positions(pose_es, "pose_es")
    gt, gt_p, gt_s, gt_c, n_gt = _positions(pose_gt, "pose_gt")
    if n != n_gt or es.device != gt.device:
        raise RuntimeError(f"dqo_eval.eval_ate: {n} estimated and {n_gt} ground-truth poses (or different devices)")
    lib, dev = N.lib(), es.device
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("dqo_eval.eval_ate: out must be a contiguous float64 [N] tensor on the poses' device")
    if fit is not None and (fit.dtype != torch.float64 or fit.numel() != 12 or not fit.is_contiguous() or fit.device != dev):
        raise RuntimeError("dqo_eval.eval_ate: fit must be a contiguous float64 tensor of 12 elements on the poses' device")
    need = lib.dqo_eval_ate_workspace_bytes(n)
    if need == 0:
        raise RuntimeError(f"dqo_eval.eval_ate: bad point count {n}")
    ws = _ws(workspace_buffer, dev, need, "ate", n)
    with torch.cuda.device(dev):
        # model = ground truth, data = estimate: Tracker.eval_ate calls eval_ate(pose_gt, pose_es) (:429)
        N.check(lib.dqo_eval_ate(n, gt_p, gt_s, gt_c, es_p, es_s, es_c, out.data_ptr(), N.ptr(fit), ws.data_ptr(), ws.numel(), N.current_stream()))
    return out


def eval_ate_dict(curve):
    """{"ate": the full trajectory's ATE in cm} — what save_traj prints (tracker.py:406-407) — from a device curve: ONE host read."""
    return {"ate": float(curve.detach().reshape(-1)[-1].cpu())}


# ---- the map as a triangle mesh (csrc/map_tsdf.hip) ---------------------------------------------------------------------------------------
TSDF_HEADER = ("vertices", "faces", "vertices_dropped", "faces_dropped", "frames", "frames_skipped", "unused6", "unused7")
TSDF_MAX_VOXELS = 1 << 28


def _intrinsics(K):
    """(fx, fy, cx, cy) from a sequence of the four, or from a host 3 x 3 pinhole matrix."""
    if torch.is_tensor(K):
        if K.is_cuda:
            raise RuntimeError("dqo_eval.TsdfVolume.integrate: K is host data (fx, fy, cx, cy or a 3 x 3 matrix); a device tensor would be a host read")
        K = K.tolist()
    K = list(K)
    if len(K) == 4 and not hasattr(K[0], "__len__"):
        return tuple(float(v) for v in K)
    if len(K) == 3 and all(len(r) == 3 for r in K):
        return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    raise RuntimeError("dqo_eval.TsdfVolume.integrate: K is (fx, fy, cx, cy) or a 3 x 3 matrix")


class TsdfVolume:
    """A dense uniform TSDF volume on the device and its mesh — what make_mesh.py and eval_frame(..., volume=..., scale=...)
    (SLAM/eval.py:299, 316-343) use open3d for, which does not exist on this platform.  include/dqo_raster.h (dqo_tsdf_integrate,
    dqo_tsdf_extract) states both rules; tests/tsdf_oracle.py restates them in numpy.  A dense grid over the caller's box, not open3d's
    hashed blocks; marching tetrahedra, not open3d's marching cubes.

    origin: the box's lowest corner (three floats); voxel_length; dims = (nx, ny, nz), every side >= 2, fewer than 2^28 voxels;
    sdf_trunc: the truncation distance in metres.  Lattice point (x, y, z) sits at origin + (index + 0.5) * voxel_length.
    Public tensors (float32, x fastest): tsdf [nz,ny,nx], weight [nz,ny,nx], color [3,nz,ny,nx]; header int32 [8] (TSDF_HEADER).
    The constructor allocates the volume and the extraction workspace and clears the volume (one launch); after the first call of a
    shape no method allocates.  Nothing is read back except by counts().  GPU only: there is no CPU path."""

    def __init__(self, origin, voxel_length, dims, sdf_trunc, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")
        nx, ny, nz = (int(d) for d in dims)
        if min(nx, ny, nz) < 2:
            raise RuntimeError(f"dqo_eval.TsdfVolume: bad dims {nx} x {ny} x {nz}: every side is at least 2")
        if nx * ny * nz >= TSDF_MAX_VOXELS:
            raise RuntimeError(f"dqo_eval.TsdfVolume: too many voxels: {nx} x {ny} x {nz} is not below 2^28")
        if not (float(voxel_length) > 0.0 and float(sdf_trunc) > 0.0):
            raise RuntimeError("dqo_eval.TsdfVolume: voxel_length and sdf_trunc are above 0")
        self.device, self.dims = dev, (nx, ny, nz)
        self.origin = tuple(float(v) for v in origin)
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        f32 = dict(dtype=torch.float32, device=dev)
        self.tsdf, self.weight = torch.empty((nz, ny, nx), **f32), torch.empty((nz, ny, nx), **f32)
        self.color = torch.empty((3, nz, ny, nx), **f32)
        self.header = torch.empty((8,), dtype=torch.int32, device=dev)
        self._ws = torch.zeros((N.lib().dqo_tsdf_workspace_bytes(nx, ny, nz),), dtype=torch.uint8, device=dev)
        self._meshes = {}
        self.clear()

    def clear(self):
        """tsdf = 1, weight = 0, color = 0, header = 0: one launch."""
        with torch.cuda.device(self.device):
            N.check(N.lib().dqo_tsdf_clear(*self.dims, self.tsdf.data_ptr(), self.weight.data_ptr(), self.color.data_ptr(),
                                           self.header.data_ptr(), N.current_stream()))
        return self

    def integrate(self, depth, color, K, w2c, depth_trunc=30.0, render_header=None):
        """One RGB-D frame into the volume, one launch.  depth: float32 [H,W] or [1,H,W] device tensor in metres; color: float32 [3,H,W];
        K: (fx, fy, cx, cy) or a 3 x 3 matrix, HOST numbers; w2c: float32 device tensor of 16 elements, the world-to-camera matrix row
        major; depth_trunc: pixels deeper than this are ignored, as are pixels with depth <= 0.  render_header: the geometry buffer of
        the forward that rendered the frame; a render that outgrew its context integrates nothing and counts in header[5]."""
        N.require_gpu_op((depth, color, w2c), render_header)
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        if depth.numel() != H * W or tuple(color.shape) != (3, H, W):
            raise RuntimeError(f"dqo_eval.TsdfVolume.integrate: depth is [{H},{W}] and color [3,{H},{W}], got {tuple(depth.shape)} and {tuple(color.shape)}")
        for t, name in ((depth, "depth"), (color, "color"), (w2c, "w2c")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.tsdf.device:
                raise RuntimeError(f"dqo_eval.TsdfVolume.integrate: {name} must be a contiguous float32 tensor on the volume's device")
        if w2c.numel() != 16:
            raise RuntimeError("dqo_eval.TsdfVolume.integrate: w2c holds 16 floats, row major")
        fx, fy, cx, cy = _intrinsics(K)
        with torch.cuda.device(self.device):
            N.check(N.lib().dqo_tsdf_integrate(*self.dims, *self.origin, self.voxel_length, self.sdf_trunc, self.tsdf.data_ptr(),
                                               self.weight.data_ptr(), self.color.data_ptr(), self.header.data_ptr(), W, H, depth.data_ptr(),
                                               color.data_ptr(), fx, fy, cx, cy, w2c.data_ptr(), float(depth_trunc), N.ptr(render_header),
                                               N.current_stream()))
        return self

    def extract(self, cap_vertices, cap_faces, out=None):
        """The volume's mesh: dict(vertices float32 [cap_vertices,3], colors float32 [cap_vertices,3], faces int32 [cap_faces,3], header),
        all on the device; header[0..3] = vertices written, faces written, vertices dropped, faces dropped (rows behind the written
        counts are not touched).  out: such a dict to write into (default: this volume's own buffers for the two capacities, made on the
        first call and overwritten by the next).  Four launches, no host read; the same bits on every run."""
        cv, cf = int(cap_vertices), int(cap_faces)
        if cv < 0 or cf < 0:
            raise RuntimeError(f"dqo_eval.TsdfVolume.extract: bad capacity: {cv} vertices, {cf} faces")
        dev = self.tsdf.device
        if out is None:
            out = self._meshes.get((cv, cf))
            if out is None:
                out = self._meshes[(cv, cf)] = dict(vertices=torch.empty((cv, 3), dtype=torch.float32, device=dev),
                                                    colors=torch.empty((cv, 3), dtype=torch.float32, device=dev),
                                                    faces=torch.empty((cf, 3), dtype=torch.int32, device=dev))
        v, c, f = out["vertices"], out["colors"], out["faces"]
        N.require_gpu_op((self.tsdf,), v, c, f)
        for t, shape, dtype, name in ((v, (cv, 3), torch.float32, "vertices"), (c, (cv, 3), torch.float32, "colors"), (f, (cf, 3), torch.int32, "faces")):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or (t.numel() and t.device != dev):
                raise RuntimeError(f"dqo_eval.TsdfVolume.extract: out[{name!r}] must be a contiguous {dtype} {list(shape)} tensor on the volume's device")
        with torch.cuda.device(self.device):
            N.check(N.lib().dqo_tsdf_extract(*self.dims, *self.origin, self.voxel_length, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                             self.color.data_ptr(), N.ptr(v), N.ptr(c), N.ptr(f), cv, cf, self.header.data_ptr(),
                                             self._ws.data_ptr(), self._ws.numel(), N.current_stream()))
        out["header"] = self.header
        return out

    def counts(self):
        """{name: int} of the header (TSDF_HEADER): the last extract's written and dropped counts, the frames integrated and skipped
        since clear() — the ONE host read."""
        h = self.header.cpu().tolist()
        return {n: int(x) for n, x in zip(TSDF_HEADER, h) if not n.startswith("unused")}


# ---- the mesh's clean-up (csrc/map_meshops.hip) ------------------------------------------------------------------------------------------
MESHOPS_HEADER = ("vertices", "faces", "components", "components_kept", "faces_bad_index", "largest_component_faces", "vertices_removed",
                  "faces_removed")
_MESH_SCOPES = {"positions": N.CONSTANTS["DQO_MESH_SMOOTH_POSITIONS"], "colors": N.CONSTANTS["DQO_MESH_SMOOTH_COLOURS"],
                "colours": N.CONSTANTS["DQO_MESH_SMOOTH_COLOURS"], "all": N.CONSTANTS["DQO_MESH_SMOOTH_BOTH"],
                "both": N.CONSTANTS["DQO_MESH_SMOOTH_BOTH"]}
_mesh_outs = {}  # the module's own out meshes and normals, one per (device, capacities)


def _mesh(mesh, who):
    """(vertices, colors or None, faces, counts or None, cap_v, cap_f) of a mesh dict, checked."""
    v, f, c, h = mesh["vertices"], mesh["faces"], mesh.get("colors"), mesh.get("header")
    N.require_gpu_op((v, f), c, h)
    cv, cf = int(v.shape[0]), int(f.shape[0])
    if tuple(v.shape) != (cv, 3) or v.dtype != torch.float32 or not v.is_contiguous():
        raise RuntimeError(f"dqo_eval.{who}: mesh['vertices'] must be a contiguous float32 [V,3] tensor")
    if tuple(f.shape) != (cf, 3) or f.dtype != torch.int32 or not f.is_contiguous() or f.device != v.device:
        raise RuntimeError(f"dqo_eval.{who}: mesh['faces'] must be a contiguous int32 [F,3] tensor on the vertices' device")
    if c is not None and (tuple(c.shape) != (cv, 3) or c.dtype != torch.float32 or not c.is_contiguous() or c.device != v.device):
        raise RuntimeError(f"dqo_eval.{who}: mesh['colors'] must be a contiguous float32 [{cv},3] tensor on the vertices' device")
    if h is not None and (h.dtype != torch.int32 or h.numel() < 2 or not h.is_contiguous() or h.device != v.device):
        raise RuntimeError(f"dqo_eval.{who}: mesh['header'] must be a contiguous int32 tensor of at least two words (vertices, faces) on the vertices' device")
    if not (1 <= cv < (1 << 28) and 1 <= cf < (1 << 28)):
        raise RuntimeError(f"dqo_eval.{who}: bad capacity: {cv} vertices, {cf} faces: both are at least 1 and below 2^28")
    return v, c, f, h, cv, cf


def _mesh_ws(kind, workspace_buffer, dev, cv, cf):
    if workspace_buffer is not None:
        N.require_gpu_op(workspace_buffer)
    return _ws(workspace_buffer, dev, lambda: getattr(N.lib(), f"dqo_mesh_{kind}_workspace_bytes")(cv, cf), "mesh_" + kind, cv, cf)


def _own_mesh_out(tag, dev, cv, cf, colors):
    """This module's own out mesh of one operator (`tag`) for a device and capacities, made on first use."""
    key = (tag, _dev_index(dev), cv, cf, colors)
    out = _mesh_outs.get(key)
    if out is None:
        out = _mesh_outs[key] = dict(vertices=torch.empty((cv, 3), dtype=torch.float32, device=dev),
                                     faces=torch.empty((cf, 3), dtype=torch.int32, device=dev),
                                     header=torch.empty((8,), dtype=torch.int32, device=dev))
        if colors:
            out["colors"] = torch.empty((cv, 3), dtype=torch.float32, device=dev)
    return out


def _out_mesh(who, out, dev, cv, cf, colors, header_is="out['header'] is int32 [8]"):
    """The out mesh of mesh_components, mesh_simplify and mesh_cull: the caller's, or (None) the module's own for the operator — its
    cache is the operator's alone — with a header; checked as a mesh whose header has 8 words.  Returns (out, _mesh(out)'s tuple)."""
    if out is None:
        out = _own_mesh_out(who, dev, cv, cf, colors)
    if "header" not in out:
        out["header"] = torch.empty((8,), dtype=torch.int32, device=dev)
    if colors and "colors" not in out:
        raise RuntimeError(f"dqo_eval.{who}: the mesh has colors, out has none")
    parts = _mesh(out, who)
    if parts[3].numel() != 8:
        raise RuntimeError(f"dqo_eval.{who}: {header_is}")
    return out, parts


def mesh_components(mesh, min_faces=0, largest_only=False, out=None, want_labels=False, workspace_buffer=None):
    """Connected components of a mesh and the mesh without its small ones — open3d's cluster_connected_triangles +
    remove_triangles_by_mask + remove_unreferenced_vertices (include/dqo_raster.h, dqo_mesh_components, states the rule: faces are
    connected through shared vertex indices, a component's label is its smallest vertex id, a face is kept iff its component has at
    least max(min_faces, largest_only ? the largest component's size : 0) faces).  mesh: the dict TsdfVolume.extract returns (vertices,
    faces, optionally colors, and header, whose words 0 and 1 are the counts; without a header the capacities are the counts).
    Returns a mesh dict of the same shape in OTHER buffers (`out`, whose capacities must not be below the input's; default: this module's
    own for the capacities, overwritten by the next call) whose header is the int32 [8] MESHOPS_HEADER; with want_labels also
    "labels", int32 [cap_faces] (-1: a face with a bad index).  The returned dict also carries "header_names" = MESHOPS_HEADER, a tuple,
    not a tensor: the mesh-dict contract's one host-side key, by which mesh_counts names the header's words; a dict without it has
    TsdfVolume.extract's header (so do not hand a dict this function filled to extract(out=...) without dropping that key).  out's
    header must not be the input mesh's: the first launch clears it.  Eleven launches, nothing read back; mesh_counts reads a header."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_components")
    dev = v.device
    own, shapes = out is None, "out['header'] is int32 [8], out['labels'] a contiguous int32 [cap_faces] device tensor"
    out, (ov, oc, of, oh, ocv, ocf) = _out_mesh("mesh_components", out, dev, cv, cf, c is not None, shapes)
    if own and not want_labels:
        out.pop("labels", None)  # (an earlier call's)
    if want_labels and "labels" not in out:
        out["labels"] = torch.empty((cf,), dtype=torch.int32, device=dev)
    labels = out["labels"] if want_labels else None
    if labels is not None and (labels.dtype != torch.int32 or labels.numel() < cf or not labels.is_contiguous() or not labels.is_cuda):
        raise RuntimeError(f"dqo_eval.mesh_components: {shapes}")
    ws = _mesh_ws("components", workspace_buffer, dev, cv, cf)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_components(v.data_ptr(), N.ptr(c), f.data_ptr(), N.ptr(h), cv, cf, int(min_faces), 1 if largest_only else 0,
                                            ov.data_ptr(), N.ptr(oc) if c is not None else None, of.data_ptr(), ocv, ocf, N.ptr(labels),
                                            oh.data_ptr(), ws.data_ptr(), ws.numel(), N.current_stream()))
    out["header_names"] = MESHOPS_HEADER  # (what mesh_counts calls the words)
    return out


MESH_SIMPLIFY_HEADER = ("vertices", "faces", "clusters", "vertices_outside", "faces_bad_index", "faces_outside", "faces_collapsed",
                        "faces_duplicate")


def mesh_simplify(mesh, voxel_size, origin=(0.0, 0.0, 0.0), out=None, workspace_buffer=None):
    """The mesh with fewer triangles, by vertex clustering — open3d's simplify_vertex_clustering(voxel_size, Average)
    (include/dqo_raster.h, dqo_mesh_simplify, states the rule: the vertices of a cell of the grid of `voxel_size` at `origin` become
    one vertex at their average position and colour, summed in double in ascending vertex id; a face two of whose corners share a
    cell collapses; of the faces that name the same three clusters in the same orientation the first stays; a cluster that no face
    names any more goes).  The caller places the grid: for a TsdfVolume's mesh, the volume's origin.  mesh: a mesh dict, as for
    mesh_components — often mesh_components' own output.  Returns a mesh dict in OTHER buffers (`out`, whose capacities must not be
    below the input's; default: this module's own for the capacities — not mesh_components' —, overwritten by the next call) whose
    header is the int32 [8] MESH_SIMPLIFY_HEADER, words 0 and 1 the counts, and whose "header_names" names it for mesh_counts.
    Twelve launches, nothing read back."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_simplify")
    dev = v.device
    out, (ov, oc, of, oh, ocv, ocf) = _out_mesh("mesh_simplify", out, dev, cv, cf, c is not None)
    ox, oy, oz = (float(x) for x in origin)
    ws = _mesh_ws("simplify", workspace_buffer, dev, cv, cf)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_simplify(v.data_ptr(), N.ptr(c), f.data_ptr(), N.ptr(h), cv, cf, float(voxel_size), ox, oy, oz, ov.data_ptr(),
                                          N.ptr(oc) if c is not None else None, of.data_ptr(), ocv, ocf, oh.data_ptr(), ws.data_ptr(),
                                          ws.numel(), N.current_stream()))
    out["header_names"] = MESH_SIMPLIFY_HEADER  # (what mesh_counts calls the words)
    return out


def mesh_smooth(mesh, iterations, lam=0.5, mu=None, scope="all", workspace_buffer=None):
    """Laplacian smoothing in place — open3d's filter_smooth_laplacian(iterations, lam), the reference configs' mesh_smooth_iter and
    mesh_smooth_lambda (configs/Cube_Diorama_base.yaml:45-46) — and, with mu (open3d's default -0.53 beside lam 0.5),
    filter_smooth_taubin: every iteration a step with lam, then one with mu.  include/dqo_raster.h (dqo_mesh_smooth) states the step:
    inverse-distance weights over the vertices that share a face, in double, rounded to float32 between steps.  scope: "positions",
    "colors" (the positions give the weights and stay) or "all" (both; positions only when the mesh has no colors).  Returns `mesh`.
    Five launches for the adjacency, one per step, nothing read back."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_smooth")
    if scope not in _MESH_SCOPES:
        raise RuntimeError(f"dqo_eval.mesh_smooth: scope is 'positions', 'colors' or 'all', got {scope!r}")
    sc = _MESH_SCOPES[scope]
    if sc == _MESH_SCOPES["all"] and c is None:
        sc = _MESH_SCOPES["positions"]
    if sc == _MESH_SCOPES["colors"] and c is None:
        raise RuntimeError("dqo_eval.mesh_smooth: scope 'colors' on a mesh without colors")
    ws = _mesh_ws("smooth", workspace_buffer, v.device, cv, cf)
    with torch.cuda.device(v.device):
        N.check(N.lib().dqo_mesh_smooth(v.data_ptr(), N.ptr(c), f.data_ptr(), N.ptr(h), cv, cf, int(iterations), float(lam),
                                        0.0 if mu is None else float(mu), sc, ws.data_ptr(), ws.numel(), N.current_stream()))
    return mesh


def mesh_normals(mesh, out=None, workspace_buffer=None):
    """Area-weighted vertex normals — open3d's compute_vertex_normals (include/dqo_raster.h, dqo_mesh_normals): the sum of the incident
    faces' un-normalised normals in ascending face index, in double, normalised, (0, 0, 1) where the sum has no direction.  Adds
    mesh["normals"], float32 [cap_vertices,3] (`out`, or this module's own for the capacities, overwritten by the next call), and
    returns `mesh`.  Six launches, nothing read back."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_normals")
    dev = v.device
    if out is None:
        key = ("normals", _dev_index(dev), cv, cf)
        out = _mesh_outs.get(key)
        if out is None:
            out = _mesh_outs[key] = torch.empty((cv, 3), dtype=torch.float32, device=dev)
    N.require_gpu_op(out)
    if tuple(out.shape) != (cv, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"dqo_eval.mesh_normals: out must be a contiguous float32 [{cv},3] tensor on the mesh's device")
    ws = _mesh_ws("normals", workspace_buffer, dev, cv, cf)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_normals(v.data_ptr(), f.data_ptr(), N.ptr(h), cv, cf, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         N.current_stream()))
    mesh["normals"] = out
    return mesh


def mesh_counts(mesh):
    """{name: int} of a mesh dict's header, or the capacities of a mesh without one: the ONE host read.  The words are named by the
    dict's "header_names" (mesh_components puts MESHOPS_HEADER there); a dict without that key has TsdfVolume.extract's header, whose
    first four words are TSDF_HEADER's."""
    h = mesh.get("header")
    if h is None:
        return dict(vertices=int(mesh["vertices"].shape[0]), faces=int(mesh["faces"].shape[0]))
    names = mesh.get("header_names", TSDF_HEADER[:4])
    return {n: int(x) for n, x in zip(names, h.cpu().tolist())}


# ---- mesh evaluation: cull to the views, sample by count, compare (csrc/map_meshcull.hip, map_meshsample.hip) ------------------------------
MESH_CULL_HEADER = ("vertices", "faces", "vertices_seen", "views_used", "faces_bad_index", "faces_removed", "vertices_removed", "zero")


def _views(who, w2c, view_keep, dev):
    """(n, view_keep as uint8 or None) of an operator's views, checked: w2c float32 [n,16] or [n,4,4], view_keep uint8 / bool [n]."""
    if w2c.dtype != torch.float32 or not w2c.is_contiguous() or w2c.numel() % 16 != 0 or w2c.numel() == 0 or w2c.device != dev:
        raise RuntimeError(f"dqo_eval.{who}: w2c must be a contiguous float32 [n,16] or [n,4,4] tensor on the mesh's device")
    n = w2c.numel() // 16
    if view_keep is not None:
        if view_keep.dtype == torch.bool:
            view_keep = view_keep.view(torch.uint8)
        if view_keep.dtype != torch.uint8 or view_keep.numel() != n or not view_keep.is_contiguous() or view_keep.device != dev:
            raise RuntimeError(f"dqo_eval.{who}: view_keep must be a contiguous uint8 / bool [{n}] tensor on the mesh's device")
    return n, view_keep


def mesh_cull(mesh, w2c, K, W, H, depth=None, view_keep=None, eps=0.03, near=0.0, depth_trunc=float("inf"), min_corners=3, out=None,
              want_views=False, workspace_buffer=None):
    """The mesh restricted to what the views see — the culling every mesh-evaluation protocol of dense SLAM applies to both meshes
    before it samples them: frustum, then occlusion against the frames' depth (include/dqo_raster.h, dqo_mesh_cull, states the rule: a
    vertex is seen by a view iff it lies in front of it beyond `near`, projects into the image by TsdfVolume.integrate's own float32
    statements and, with `depth`, is not more than `eps` behind the depth of its pixel, which is above 0 and at most depth_trunc; a face
    is kept iff at least min_corners of its corners are seen by some used view; vertices no kept face names go).
    mesh: a mesh dict, as for mesh_components.  w2c: float32 device tensor [n,16] or [n,4,4], the views' world-to-camera matrices, row
    major; K: (fx, fy, cx, cy) or a 3 x 3 matrix, HOST numbers, and W, H: the camera all views share; depth: float32 [n,H,W] device
    tensor in metres (None: frustum only) — the frames' depth, or, where no sensor depth exists, mesh_render_depth's stack of the
    ground-truth mesh; view_keep: uint8 / bool [n] device tensor, 0 = the view is not used (None: all are).
    Returns a mesh dict in OTHER buffers (`out`, whose capacities must not be below the input's; default: this module's own for the
    capacities, overwritten by the next call) with header = the int32 [8] MESH_CULL_HEADER, words 0 and 1 the counts, "header_names"
    naming it for mesh_counts, and "vertex_views": with want_views int32 [cap_vertices], how many used views see each vertex (rows
    behind the count untouched), else None.  dqo_ply.write_mesh_ply writes it once cut at its counts.  Six launches, nothing read
    back, no synchronise; capturable in a graph."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_cull")
    dev = v.device
    N.require_gpu_op((v, w2c), depth, view_keep)
    n, view_keep = _views("mesh_cull", w2c, view_keep, dev)
    W, H = int(W), int(H)
    if depth is not None and (tuple(depth.shape) != (n, H, W) or depth.dtype != torch.float32 or not depth.is_contiguous() or depth.device != dev):
        raise RuntimeError(f"dqo_eval.mesh_cull: depth must be a contiguous float32 [{n},{H},{W}] tensor on the mesh's device")
    fx, fy, cx, cy = _intrinsics(K)
    out, (ov, oc, of, oh, ocv, ocf) = _out_mesh("mesh_cull", out, dev, cv, cf, c is not None)
    vv = None
    if want_views:
        vv = out.get("vertex_views")
        if vv is None:
            vv = out.get("_views_buffer")  # (an earlier call's, kept while a call without want_views set the public key to None)
        if vv is None:
            vv = out["_views_buffer"] = torch.empty((cv,), dtype=torch.int32, device=dev)
        if vv.dtype != torch.int32 or vv.numel() < cv or not vv.is_contiguous() or vv.device != dev:
            raise RuntimeError("dqo_eval.mesh_cull: out['vertex_views'] is a contiguous int32 [cap_vertices] tensor on the mesh's device")
    ws = _mesh_ws("cull", workspace_buffer, dev, cv, cf)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_cull(v.data_ptr(), N.ptr(c), f.data_ptr(), N.ptr(h), cv, cf, n, w2c.data_ptr(), N.ptr(view_keep), W, H, fx, fy,
                                      cx, cy, N.ptr(depth), float(near), float(eps), float(depth_trunc), int(min_corners), ov.data_ptr(),
                                      N.ptr(oc) if c is not None else None, of.data_ptr(), ocv, ocf, N.ptr(vv), oh.data_ptr(), ws.data_ptr(),
                                      ws.numel(), N.current_stream()))
    out["header_names"] = MESH_CULL_HEADER  # (what mesh_counts calls the words)
    out["vertex_views"] = vv
    return out


def sample_surface_counted(mesh, count, seed=0, want_face_index=False, workspace_buffer=None):
    """sample_surface on a mesh dict (as for mesh_components: vertices, faces and, when it has one, a header whose words 0 and 1 are
    the counts — TsdfVolume.extract's, mesh_components', mesh_simplify's, mesh_cull's): the counts stay on the device
    (dqo_mesh_sample_counted, include/dqo_raster.h).  Every byte of the returned dict — sample_surface's: points, face_index | None,
    keep, header (MESH_HEADER) — is what sample_surface(vertices[:V], faces[:F], count, seed) gives; a mesh without faces or without
    area gives keep all 0 (eval_pcd's mask) and no point.  Without a header the capacities are the counts.  The face capacity and count
    lie in [1, 2^25 - 1].  workspace_buffer: a tensor of mesh_sample_workspace(cap_faces, count, device) the caller keeps (default: one
    per device and sizes, kept by this module).  Four launches, nothing read back, no synchronise; capturable in a graph."""
    v, c, f, h, cv, cf = _mesh(mesh, "sample_surface_counted")
    dev, count = v.device, int(count)
    nbytes = N.lib().dqo_mesh_sample_counted_workspace_bytes(cf, count)
    if nbytes == 0:
        raise RuntimeError(f"dqo_eval.sample_surface_counted: bad sizes: {cf} faces of capacity, count = {count}: each in [1, 2^25 - 1]")
    if workspace_buffer is not None:
        N.require_gpu_op(workspace_buffer)
    ws = _ws(workspace_buffer, dev, nbytes, "mesh_counted", cf, count)
    o, ptrs = _sample_outs(count, want_face_index, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_sample_counted(v.data_ptr(), f.data_ptr(), N.ptr(h), cv, cf, count, int(seed) & (2 ** 64 - 1), *ptrs,
                                                ws.data_ptr(), ws.numel(), N.current_stream()))
    return o


# ---- exact point-to-triangle distance: the nearest face of a mesh per point (csrc/knn.hip: dqo_mesh_nearest) ------------------------------
MESH_NEAREST_HEADER = ("faces", "faces_valid", "faces_bad_index", "faces_degenerate", "queries", "zero5", "zero6", "zero7")


def nearest_on_mesh(points, mesh, query_keep=None, query_transform=None, mesh_transform=None, want_face=True, want_closest=False,
                    workspace_buffer=None):
    """The nearest face of a mesh for every point and the exact squared point-to-triangle distance to it (dqo_mesh_nearest;
    include/dqo_raster.h states the float32 rule): points [Q,3], mesh a mesh dict (as for mesh_components: vertices, faces and, when it
    has one, a header whose words 0 and 1 are the counts) -> (dist2 float32 [Q], face int32 [Q] or None, closest float32 [Q,3] or None,
    header int32 [8]: MESH_NEAREST_HEADER).  dist2 is the minimum over the VALID faces (indices inside the vertices, an area above 0) of
    the rule's D — bit for bit, whatever the search order —, face one of the faces attaining it, closest the point of that face nearest
    to the query.  query_keep: uint8 / bool mask, 0 = the point is not searched for (FLT_MAX / -1, its closest row left as
    torch.empty made it); a mesh without a valid face gives FLT_MAX / -1 everywhere.  *_transform: [3,4] / [4,4], applied to the points /
    the vertices as they are loaded.  Q and the face capacity lie in [1, 2^25 - 1].  No host read, no synchronisation, capturable;
    workspace_buffer: a uint8 tensor of dqo_mesh_nearest_workspace_bytes(Q, cap_vertices, cap_faces) the caller keeps (default: one per
    device and sizes, kept by this module — calls that share it must be on one stream)."""
    v, c, f, h, cv, cf = _mesh(mesh, "nearest_on_mesh")
    N.require_gpu_op((points, v), query_keep, workspace_buffer)
    lib, dev = N.lib(), v.device
    points = _points(points, "points")
    Q = int(points.shape[0])
    qk = _keep(query_keep, Q, "query_keep")
    qx, mx = _xform(query_transform, dev, "query_transform"), _xform(mesh_transform, dev, "mesh_transform")
    n = lib.dqo_mesh_nearest_workspace_bytes(Q, cv, cf)
    if n == 0:
        raise RuntimeError(f"dqo_eval.nearest_on_mesh: bad sizes: {Q} points, {cf} faces of capacity: each in [1, 2^25 - 1]")
    ws = _ws(workspace_buffer, dev, n, "mesh_nearest", Q, cv, cf)
    dist2 = torch.empty((Q,), dtype=torch.float32, device=dev)
    face = torch.empty((Q,), dtype=torch.int32, device=dev) if want_face else None
    closest = torch.empty((Q, 3), dtype=torch.float32, device=dev) if want_closest else None
    header = torch.empty((8,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.dqo_mesh_nearest(Q, N.ptr(points), N.ptr(qk), N.ptr(qx), v.data_ptr(), f.data_ptr(), N.ptr(h), cv, cf, N.ptr(mx),
                                     N.ptr(dist2), N.ptr(face), N.ptr(closest), header.data_ptr(), ws.data_ptr(), ws.numel(),
                                     N.current_stream()))
    return dist2, face, closest, header


def _surface_mesh(mesh, who, dev):
    """(vertices ptr, faces ptr, counts ptr, cap_v, cap_f) of an optional mesh dict of eval_pcd_surface; None: no mesh on that side."""
    if mesh is None:
        return None, None, None, 0, 0
    v, c, f, h, cv, cf = _mesh(mesh, who)
    if v.device != dev:
        raise RuntimeError(f"dqo_eval.{who}: the mesh must be on {dev}")
    return v.data_ptr(), f.data_ptr(), N.ptr(h), cv, cf


def eval_pcd_surface(gt_points, rec_points, gt_mesh=None, rec_mesh=None, dist_thres=(0.03,), transform=None, gt_keep=None, rec_keep=None,
                     out=None, row=0, workspace_buffer=None):
    """eval_pcd with exact point-to-SURFACE distances wherever a side has a mesh (dqo_eval_pcd_surface): the same float32 [32] row
    (PCD_ROW), arguments and contract as eval_pcd, and two optional mesh dicts (as for mesh_components).
    gt_mesh: every reconstructed point (under `transform`) is measured to the nearest FACE of gt_mesh instead of the nearest gt point —
    accuracy and precision; rec_mesh: every ground-truth point is measured to the nearest face of rec_mesh, whose vertices go under
    `transform` — completion and recall.  A side without a mesh keeps eval_pcd's nearest-point search; with neither mesh the row is
    eval_pcd's.  The points of both sides are still given: they are the queries, and their keep masks decide which rows count.
    A mesh without a valid face makes every distance to it FLT_MAX: that accuracy / completion is then 100 * sqrt(FLT_MAX) (about
    1.8447e21), its P / R 0 and F1 with it; a side without a kept point gives a row of NaN, as in eval_pcd.
    workspace_buffer: a zeroed uint8 tensor of dqo_eval_pcd_surface_workspace_bytes(...) the caller keeps (default: one per device and
    sizes, kept by this module).  Nothing is read back, no synchronisation."""
    N.require_gpu_op((gt_points, rec_points), gt_keep, rec_keep, out, workspace_buffer)
    lib, dev = N.lib(), rec_points.device
    gt, rec = _points(gt_points, "gt_points"), _points(rec_points, "rec_points")
    G, P = int(gt.shape[0]), int(rec.shape[0])
    gk, rk = _keep(gt_keep, G, "gt_keep"), _keep(rec_keep, P, "rec_keep")
    xf = _xform(transform, dev, "transform")
    gm, rm = _surface_mesh(gt_mesh, "eval_pcd_surface", dev), _surface_mesh(rec_mesh, "eval_pcd_surface", dev)
    thres = [float(t) for t in dist_thres]
    if len(thres) > PCD_THRES_MAX:
        raise RuntimeError(f"dqo_eval.eval_pcd_surface: at most {PCD_THRES_MAX} thresholds, got {len(thres)}")
    out, row = _table_row(out, row, 32, "eval_pcd_surface", dev, fresh=torch.empty)

    def nbytes():
        n = lib.dqo_eval_pcd_surface_workspace_bytes(G, gm[3], gm[4], P, rm[3], rm[4])
        if n == 0:
            raise RuntimeError(f"dqo_eval.eval_pcd_surface: bad sizes: {G}, {P} points (at most 2^25 - 1 rows per set), face capacities "
                               f"{gm[4]}, {rm[4]} (at most 2^25 - 1)")
        return n
    ws = _ws(workspace_buffer, dev, nbytes, "pcd_surface", G, P, gm[3], gm[4], rm[3], rm[4])
    with torch.cuda.device(dev):
        N.check(lib.dqo_eval_pcd_surface(G, N.ptr(gt), N.ptr(gk), *gm, P, N.ptr(rec), N.ptr(rk), *rm, N.ptr(xf), len(thres),
                                         (ctypes.c_float * len(thres))(*thres), out.data_ptr(), row, ws.data_ptr(), ws.numel(),
                                         N.current_stream()))
    return out[row]


def eval_mesh(rec_mesh, gt_mesh, sample_nums=1000000, seed=0, rec_seed=None, dist_thres=(0.03,), transform=None, views=None, out=None, row=0):
    """How good a reconstructed MESH is against the ground-truth mesh, in one call on the device: both meshes culled to what the
    cameras saw, both sampled, the two point sets compared — mesh_cull -> sample_surface_counted -> eval_pcd.
    rec_mesh, gt_mesh: mesh dicts (as for mesh_components; the ground truth of dqo_ply.read_mesh_ply as device tensors, without a
    header, is one).  views: None (no culling) or a dict of mesh_cull's keywords — w2c, K, W, H and optionally depth, view_keep, eps,
    near, depth_trunc, min_corners — applied to BOTH meshes, each in its own coordinates, before anything is sampled (so with `views`
    the two meshes share the cameras' frame); visibility="faces" (default "vertices") culls by mesh_cull_visible in its place — a face
    is kept by the pixels it wins in a clipped render of its mesh, min_pixels (default 1) of them, so a wall whose corners all lie
    outside the image stays — and a key of the rule not chosen, or eval_mesh_depth's clip_near, is ignored; the culled meshes live
    in buffers of this module's own, one pair per device and capacities.  sample_nums points are drawn on each: gt_mesh with `seed`, rec_mesh with rec_seed (None: seed + 1).  transform:
    eval_pcd's, applied to the reconstruction's points; dist_thres, out, row: eval_pcd's.
    Returns the float32 [32] device row (PCD_ROW); nothing is read back and the call does not synchronise.  A side that is empty — no
    faces, no area, a cull that keeps nothing — gives a row of NaN, eval_pcd's rule.  Without `views`, a gt_mesh without a header yields
    the very points sample_surface(gt vertices, gt faces, sample_nums, seed) yields.
    The distances are point to nearest sampled POINT, as the reference's; eval_mesh_surface measures to the surface itself (this
    function's signature is pinned, so that rule is a function of its own)."""
    return _eval_mesh("eval_mesh", "samples", rec_mesh, gt_mesh, sample_nums, seed, rec_seed, dist_thres, transform, views, out, row)


def eval_mesh_surface(rec_mesh, gt_mesh, sample_nums=1000000, seed=0, rec_seed=None, dist_thres=(0.03,), transform=None, views=None, out=None,
                      row=0):
    """eval_mesh with the distances taken to the SURFACE: the same culling and the same sampling — byte for byte the meshes and points
    eval_mesh compares — but the chain ends in eval_pcd_surface on the culled meshes: a reconstructed sample is measured to the nearest
    FACE of the (culled) ground-truth mesh, a ground-truth sample to the nearest face of the (culled) reconstruction under `transform`
    (nearest_on_mesh's exact point-to-triangle distance).  eval_mesh's sampled form adds the mean nearest-sample distance of the other
    side, about 0.5 / sqrt(samples per square metre), to accuracy and completion, and its result depends on `seed` through BOTH sides'
    samples; here a side's samples are only the places where the other surface's distance is read.  Arguments, the returned float32
    [32] device row and the contract (nothing read back, no synchronisation) are eval_mesh's; a side whose culled mesh keeps no valid
    face has no kept sample either, so the row is NaN, as eval_mesh's."""
    return _eval_mesh("eval_mesh_surface", "surface", rec_mesh, gt_mesh, sample_nums, seed, rec_seed, dist_thres, transform, views, out, row)


def _eval_mesh(who, distance, rec_mesh, gt_mesh, sample_nums, seed, rec_seed, dist_thres, transform, views, out, row):
    """eval_mesh's and eval_mesh_surface's chain; distance: "samples" (eval_pcd) or "surface" (eval_pcd_surface on the culled meshes)."""
    if views is not None:
        kw = dict(views)
        for k in ("out", "want_views", "want_pixels", "workspace_buffer"):
            if k in kw:
                raise RuntimeError(f"dqo_eval.{who}: views is a dict of mesh_cull's view keywords; {k!r} is {who}'s own")
        kw.pop("clip_near", None)  # (eval_mesh_depth's)
        visibility = kw.pop("visibility", "vertices")
        if visibility not in ("vertices", "faces"):
            raise RuntimeError(f"dqo_eval.{who}: views['visibility'] is 'vertices' or 'faces', got {visibility!r}")
        kw.pop("min_pixels" if visibility == "vertices" else "min_corners", None)  # (the other rule's)
        cull = mesh_cull if visibility == "vertices" else mesh_cull_visible
        meshes = []
        for tag, m in (("cull_rec", rec_mesh), ("cull_gt", gt_mesh)):
            v, c, f, h, cv, cf = _mesh(m, who)
            meshes.append(cull(m, out=_own_mesh_out(tag, v.device, cv, cf, c is not None), **kw))
        rec_mesh, gt_mesh = meshes
    gt = sample_surface_counted(gt_mesh, sample_nums, seed=seed)
    rec = sample_surface_counted(rec_mesh, sample_nums, seed=int(seed) + 1 if rec_seed is None else rec_seed)
    if distance == "surface":
        return eval_pcd_surface(gt["points"], rec["points"], gt_mesh, rec_mesh, dist_thres, transform, gt_keep=gt["keep"], rec_keep=rec["keep"],
                                out=out, row=row)
    return eval_pcd(gt["points"], rec["points"], dist_thres, transform, gt_keep=gt["keep"], rec_keep=rec["keep"], out=out, row=row)


# ---- mesh depth and Depth L1 (csrc/map_meshrender.hip, map_eval.hip) ------------------------------------------------------------------------
MESH_RENDER_HEADER = ("views_used", "faces_bad_index", "pairs_rasterised", "pairs_near_dropped", "pairs_degenerate", "pairs_cooperative",
                      "pixels_hit", "zero")
DEPTH_L1_ROW = ("l1_valid", "l1_image", "rmse_valid", "both", "only_a", "only_b", "neither", "max_abs")
_render_outs = {}  # the module's own depth stacks, one per (tag, device, n, H, W)


def _own_render_out(tag, dev, n, H, W):
    key = (tag, _dev_index(dev), n, H, W)
    out = _render_outs.get(key)
    if out is None:
        out = _render_outs[key] = dict(depth=torch.empty((n, H, W), dtype=torch.float32, device=dev),
                                       header=torch.empty((8,), dtype=torch.int32, device=dev))
    return out


def _mesh_render(who, entry, names, mesh, w2c, K, W, H, view_keep, near, depth_trunc, want_face_index, out, workspace_buffer):
    """mesh_render_depth's and mesh_render_depth_clip's body: the same checks, buffers and workspace, the entry and the header's names
    apart."""
    v, c, f, h, cv, cf = _mesh(mesh, who)
    dev = v.device
    N.require_gpu_op((v, w2c), view_keep, workspace_buffer)
    n, view_keep = _views(who, w2c, view_keep, dev)
    W, H = int(W), int(H)
    fx, fy, cx, cy = _intrinsics(K)
    nbytes = N.lib().dqo_mesh_render_depth_workspace_bytes(n, W, H)
    if nbytes == 0:
        raise RuntimeError(f"dqo_eval.{who}: bad image size {W} x {H} for {n} views")
    if out is None:
        out = _own_render_out("render", dev, n, H, W)
    if "depth" not in out:
        out["depth"] = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    if "header" not in out:
        out["header"] = torch.empty((8,), dtype=torch.int32, device=dev)
    fi = None
    if want_face_index:
        fi = out.get("face_index")
        if fi is None:
            fi = out.get("_face_index_buffer")  # (an earlier call's, kept while a call without want_face_index set the public key to None)
        if fi is None:
            fi = out["_face_index_buffer"] = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    d, oh = out["depth"], out["header"]
    N.require_gpu_op((v, d, oh), fi)
    for t, dt, name in ((d, torch.float32, "depth"), (fi, torch.int32, "face_index")):
        if t is not None and (tuple(t.shape) != (n, H, W) or t.dtype != dt or not t.is_contiguous() or t.device != dev):
            raise RuntimeError(f"dqo_eval.{who}: out['{name}'] is a contiguous {dt} [{n},{H},{W}] tensor on the mesh's device")
    if oh.dtype != torch.int32 or oh.numel() != 8 or not oh.is_contiguous() or oh.device != dev:
        raise RuntimeError(f"dqo_eval.{who}: out['header'] is int32 [8] on the mesh's device")
    ws = _ws(workspace_buffer, dev, nbytes, "mesh_render", n, W, H)
    with torch.cuda.device(dev):
        N.check(getattr(N.lib(), entry)(v.data_ptr(), f.data_ptr(), N.ptr(h), cv, cf, n, w2c.data_ptr(), N.ptr(view_keep), W, H, fx, fy, cx, cy,
                                        float(near), float(depth_trunc), d.data_ptr(), N.ptr(fi), oh.data_ptr(), ws.data_ptr(), ws.numel(),
                                        N.current_stream()))
    out["face_index"] = fi
    out["header_names"] = names  # (what mesh_counts calls the words)
    return out


def mesh_render_depth(mesh, w2c, K, W, H, view_keep=None, near=0.0, depth_trunc=float("inf"), want_face_index=False, out=None,
                      workspace_buffer=None):
    """The mesh rasterised to depth in n views — the render whose depths the Depth L1 number compares (include/dqo_raster.h,
    dqo_mesh_render_depth, states the rule: corners projected by mesh_cull's own float32 statements without its + 0.5, so pixel centres
    sit at integer coordinates; edge functions in double, ordered by vertex id, so two faces that share an edge leave no pixel between
    them; coverage inclusive, both sides of a face; depth by ray-plane intersection in double; a pixel keeps the nearest face, the
    lower face id at equal depth, whatever order the faces arrive in).  A face that crosses the near plane of a view is dropped there
    and counted, not clipped.
    mesh: a mesh dict, as for mesh_components.  w2c, K, W, H, view_keep, near, depth_trunc: mesh_cull's.  Returns dict(depth float32
    [n,H,W], 0 = no hit; face_index int32 [n,H,W], -1 = no hit, or None without want_face_index; header int32 [8]; header_names =
    MESH_RENDER_HEADER, by which mesh_counts reads the header) in `out` (a dict with such tensors; default: this module's own for the
    device and sizes, overwritten by the next call); the images of unused views are written as no hit.  The depth stack is a `depth`
    for mesh_cull: the ground-truth mesh's own render serves its occlusion test where no sensor depth exists.
    workspace_buffer: a uint8 tensor of dqo_mesh_render_depth_workspace_bytes(n, W, H) bytes the caller keeps, zero when first used
    (default: one per device and sizes, kept by this module).  Three launches, nothing read back, no synchronise; capturable in a graph."""
    return _mesh_render("mesh_render_depth", "dqo_mesh_render_depth", MESH_RENDER_HEADER, mesh, w2c, K, W, H, view_keep, near, depth_trunc,
                        want_face_index, out, workspace_buffer)


MESH_RENDER_CLIP_HEADER = MESH_RENDER_HEADER[:3] + ("pairs_near_clipped",) + MESH_RENDER_HEADER[4:]


def mesh_render_depth_clip(mesh, w2c, K, W, H, view_keep=None, near=0.0, depth_trunc=float("inf"), want_face_index=False, out=None,
                           workspace_buffer=None):
    """mesh_render_depth with the near plane CLIPPED (include/dqo_raster.h, dqo_mesh_render_depth_clip): a face that crosses the near
    plane of a view is rasterised there — homogeneous edge functions for its edges that leave the front, the depth test d > near as the
    clip — where mesh_render_depth drops it, so a wall of two triangles seen from inside the room is an image, not a hole.  A mesh that
    no view crosses gives mesh_render_depth's bytes.  Arguments, buffers, workspace and the returned dict are mesh_render_depth's
    (without `out` the two share this module's buffers for a device and sizes); header_names = MESH_RENDER_CLIP_HEADER, whose word 3 is
    pairs_near_clipped.  Its face_index is what mesh_cull_visible culls by.  mesh_render_depth's signature is pinned, so the switch
    is this twin; eval_mesh_depth's views take clip_near=True.  Three launches, nothing read back; capturable in a graph."""
    return _mesh_render("mesh_render_depth_clip", "dqo_mesh_render_depth_clip", MESH_RENDER_CLIP_HEADER, mesh, w2c, K, W, H, view_keep, near,
                        depth_trunc, want_face_index, out, workspace_buffer)


MESH_CULL_FACES_HEADER = ("vertices", "faces", "faces_with_pixels", "views_used", "faces_bad_index", "faces_removed", "vertices_removed",
                          "pixels_counted")


def mesh_cull_visible(mesh, w2c, K, W, H, depth=None, view_keep=None, eps=0.03, near=0.0, depth_trunc=float("inf"), min_pixels=1, out=None,
                      want_pixels=False):
    """The mesh restricted to the faces the views SEE, decided per face by the pixels it wins: the mesh is rendered from the views with
    the near plane clipped (mesh_render_depth_clip, with face_index; near is the render's, whose own depth_trunc is +inf), and a face
    is kept iff it wins at least min_pixels pixels of the used views (include/dqo_raster.h, dqo_mesh_cull_faces) — with `depth`, the
    frames' depth, only pixels where that depth is above 0, at most depth_trunc and not more than eps in front of the render's count:
    mesh_cull's occlusion statement per pixel.  Where mesh_cull tests vertices, and so drops a wall of two triangles that fills every
    frame because its corners lie outside them, this keeps it; a face hidden behind another wins no pixel and goes.
    mesh, w2c, K, W, H, depth, view_keep, eps, depth_trunc, out: mesh_cull's.  Returns a mesh dict like mesh_cull's: header = the int32
    [8] MESH_CULL_FACES_HEADER (words 0 and 1 the counts), "header_names", "face_pixels": with want_pixels int32 [cap_faces], the
    pixels each face won (rows behind the count untouched), else None, and "render": mesh_render_depth_clip's dict of this call (depth,
    face_index, header), in buffers of this module's own per device and sizes.  Nine launches, nothing read back, no synchronise;
    capturable in a graph."""
    v, c, f, h, cv, cf = _mesh(mesh, "mesh_cull_visible")
    dev = v.device
    N.require_gpu_op((v, w2c), depth, view_keep)
    n, view_keep = _views("mesh_cull_visible", w2c, view_keep, dev)
    W, H = int(W), int(H)
    if depth is not None and (tuple(depth.shape) != (n, H, W) or depth.dtype != torch.float32 or not depth.is_contiguous() or depth.device != dev):
        raise RuntimeError(f"dqo_eval.mesh_cull_visible: depth must be a contiguous float32 [{n},{H},{W}] tensor on the mesh's device")
    out, (ov, oc, of, oh, ocv, ocf) = _out_mesh("mesh_cull_visible", out, dev, cv, cf, c is not None)
    px = out.get("face_pixels")
    if px is None:
        px = out.get("_pixels_buffer")  # (an earlier call's, kept while a call without want_pixels set the public key to None)
    if px is None:
        px = out["_pixels_buffer"] = torch.empty((cf,), dtype=torch.int32, device=dev)
    if px.dtype != torch.int32 or px.numel() < cf or not px.is_contiguous() or px.device != dev:
        raise RuntimeError("dqo_eval.mesh_cull_visible: out['face_pixels'] is a contiguous int32 [cap_faces] tensor on the mesh's device")
    out["_pixels_buffer"] = px
    r = mesh_render_depth_clip(mesh, w2c, K, W, H, view_keep=view_keep, near=near, want_face_index=True,
                               out=_own_render_out("cull_visible", dev, n, H, W))
    ws = _mesh_ws("cull", None, dev, cv, cf)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_mesh_cull_faces(v.data_ptr(), N.ptr(c), f.data_ptr(), N.ptr(h), cv, cf, n, N.ptr(view_keep), W, H,
                                            r["face_index"].data_ptr(), r["depth"].data_ptr(), N.ptr(depth), float(eps), float(depth_trunc),
                                            int(min_pixels), ov.data_ptr(), N.ptr(oc) if c is not None else None, of.data_ptr(), ocv, ocf,
                                            px.data_ptr(), oh.data_ptr(), ws.data_ptr(), ws.numel(), N.current_stream()))
    out["header_names"] = MESH_CULL_FACES_HEADER  # (what mesh_counts calls the words)
    out["face_pixels"] = px if want_pixels else None
    out["render"] = r
    return out


def depth_l1(depth_gt, depth_rec, view_keep=None, depth_trunc=float("inf"), out=None):
    """Depth L1 of two depth stacks, on the device (include/dqo_raster.h, dqo_eval_depth_l1): depth_gt (the truth) and depth_rec,
    float32 [n,H,W] device tensors, 0 = no hit — mesh_render_depth's, a stack of the map's renders, the sensor's.  A pixel is valid iff
    0 < depth_gt <= depth_trunc and depth_rec > 0.  Returns the float32 [n + 1, 8] table (DEPTH_L1_ROW; `out`, or a new tensor): row k
    of a used view = l1_valid (the mean of |gt - rec| over the valid pixels), l1_image (the mean over all pixels, a side without a hit
    taken as 0: the NICE-SLAM form), rmse_valid, the counts both / only_a / only_b / neither, max_abs; NaN in the three means of a view
    without a valid pixel, a row of NaN for an unused view (view_keep: uint8 / bool [n], 0 = unused); row n = the means of the used
    views' three values where defined, the counts summed, the largest maximum.  Double sums added in a fixed order: the table is
    bitwise reproducible.  Two launches, nothing read back; depth_l1_dict reads the table."""
    N.require_gpu_op((depth_gt, depth_rec), view_keep, out)
    dev = depth_gt.device
    if depth_gt.dim() != 3 or depth_gt.dtype != torch.float32 or not depth_gt.is_contiguous():
        raise RuntimeError("dqo_eval.depth_l1: depth_gt must be a contiguous float32 [n,H,W] device tensor")
    n, H, W = (int(x) for x in depth_gt.shape)
    if tuple(depth_rec.shape) != (n, H, W) or depth_rec.dtype != torch.float32 or not depth_rec.is_contiguous() or depth_rec.device != dev:
        raise RuntimeError(f"dqo_eval.depth_l1: depth_rec must be a contiguous float32 [{n},{H},{W}] tensor on depth_gt's device")
    if view_keep is not None:
        if view_keep.dtype == torch.bool:
            view_keep = view_keep.view(torch.uint8)
        if view_keep.dtype != torch.uint8 or view_keep.numel() != n or not view_keep.is_contiguous() or view_keep.device != dev:
            raise RuntimeError(f"dqo_eval.depth_l1: view_keep must be a contiguous uint8 / bool [{n}] tensor on depth_gt's device")
    nbytes = N.lib().dqo_eval_depth_l1_workspace_bytes(n, W, H)
    if nbytes == 0:
        raise RuntimeError(f"dqo_eval.depth_l1: bad sizes: {n} views of {W} x {H}: 1 to 65535 views, W * H below 2^24")
    if out is None:
        out = torch.empty((n + 1, 8), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (n + 1, 8) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"dqo_eval.depth_l1: out must be a contiguous float32 [{n + 1},8] tensor on depth_gt's device")
    ws = _ws(None, dev, nbytes, "depth_l1", n, W, H)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_eval_depth_l1(n, W, H, depth_gt.data_ptr(), depth_rec.data_ptr(), N.ptr(view_keep), float(depth_trunc), out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), N.current_stream()))
    return out


def depth_l1_dict(table):
    """depth_l1's table as {"views": [a dict per view, None for an unused one], "mean": the last row's dict}, names DEPTH_L1_ROW, the
    counts as ints: the ONE host read."""
    rows = table.cpu().tolist()

    def named(r):
        if all(x != x for x in r):
            return None
        return {k: (x if i < 3 or i == 7 else int(x)) for i, (k, x) in enumerate(zip(DEPTH_L1_ROW, r))}

    return dict(views=[named(r) for r in rows[:-1]], mean=named(rows[-1]))


def eval_mesh_depth(rec_mesh, gt_mesh, views, out=None):
    """Depth L1 of a reconstructed mesh against the ground-truth mesh, in one call on the device: both meshes rendered to depth from the
    same views (mesh_render_depth), the two stacks compared (depth_l1, the ground truth as the truth).  rec_mesh, gt_mesh: mesh dicts,
    as for eval_mesh.  views: eval_mesh's dict — w2c, K, W, H and optionally view_keep, near, depth_trunc and clip_near (True: both
    meshes by mesh_render_depth_clip, so a wall that crosses a camera's near plane is depth and not a hole; default False); its other
    keys (depth, eps, min_corners, min_pixels, visibility) belong to the cull and are ignored here.  depth_trunc applies to both renders and to the comparison.  The two depth
    stacks live in buffers of this module's own, one pair per device and sizes.  Returns depth_l1's float32 [n + 1, 8] table (`out`,
    or a new tensor); nothing is read back."""
    if views is None:
        raise RuntimeError("dqo_eval.eval_mesh_depth: views is a dict with w2c, K, W and H: a depth needs cameras")
    kw = {k: x for k, x in dict(views).items() if k not in ("depth", "eps", "min_corners", "min_pixels", "visibility")}
    render = mesh_render_depth_clip if kw.pop("clip_near", False) else mesh_render_depth
    for k in ("out", "want_face_index", "workspace_buffer"):
        if k in kw:
            raise RuntimeError(f"dqo_eval.eval_mesh_depth: views is a dict of the views' keywords; {k!r} is mesh_render_depth's own")
    stacks = []
    for tag, m in (("depth_gt", gt_mesh), ("depth_rec", rec_mesh)):
        v = m["vertices"]
        N.require_gpu_op((v, kw["w2c"]))
        n, H, W = kw["w2c"].numel() // 16, int(kw["H"]), int(kw["W"])
        stacks.append(render(m, out=_own_render_out(tag, v.device, n, H, W), **kw)["depth"])
    return depth_l1(stacks[0], stacks[1], view_keep=kw.get("view_keep"), depth_trunc=kw.get("depth_trunc", float("inf")), out=out)
