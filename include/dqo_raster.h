/*
 * dqo_raster.h — C ABI of libdqoraster.so: the MI355X (gfx950) drop-in for DQO-MAP's mapping hot path.
 *
 * Every entry point replaces one binding of the reference's three CUDA extensions (paths relative to
 * /root/reference):
 *
 *   dqo_rast_forward_*   <- _C_depth.rasterize_gaussians           submodules/diff-gaussian-rasterizer-depth/ext.cpp:16,
 *                                                                  rasterize_points.cu:37-155, cuda_rasterizer/rasterizer.h:35-73
 *   dqo_rast_backward    <- _C_depth.rasterize_gaussians_backward  ext.cpp:17, rasterize_points.cu:157-249, rasterizer.h:75-105
 *   dqo_mark_visible     <- _C_depth.mark_visible                  ext.cpp:18, rasterize_points.cu:251-270, rasterizer.h:27-33
 *   dqo_knn3             <- simple_knn._C.distCUDA2                submodules/simple-knn/ext.cpp:15-17, spatial.cu:15-28
 *   dqo_quadric_*        <- Ellipsoid_tensor.forward + bboxes_iou + the Adam loop of Object_Optimize_only
 *                                                                  SLAM/multiprocess/quadrics.py:285-290, 2018-2091, 2144-2220, 2234-2298
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (tensor.data_ptr()), sizes, no torch / C++ types; all memory is caller-owned.
 *   - every launch goes to the caller's stream (`hipStream_t` passed as void*); no hipMalloc/hipFree, no host
 *     synchronisation inside any entry point except dqo_rast_read_header (explicitly a D2H read).
 *   - return value: 0 on success, negative DqoStatus on error; dqo_last_error() gives the message (thread-local).
 *     The reference throws C++ exceptions -> Python RuntimeError (rasterize_points.cu:67-70); the Python shim does the same.
 *   - fp32 everywhere, matrices in the reference's row-vector convention (flat 16 floats, auxiliary.h:59-77).
 */
#ifndef DQO_RASTER_H_
#define DQO_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQO_ABI_VERSION 5

typedef enum DqoStatus {
    DQO_OK = 0,
    DQO_ERR_INVALID_ARG = -1,  /* bad shape / null pointer / unsupported combination */
    DQO_ERR_WORKSPACE = -2,    /* a caller-provided buffer is too small */
    DQO_ERR_LAUNCH = -3,       /* hipLaunch / hipMemsetAsync failed (message holds hipGetErrorString) */
    DQO_ERR_OVERFLOW = -4      /* instance capacity exceeded (reported by dqo_rast_read_header) */
} DqoStatus;

/* Scalar settings: GaussianRasterizationSettings, diff_gaussian_rasterization_depth/__init__.py:288-307. */
typedef struct DqoRastParams {
    int32_t P;              /* number of Gaussians (means3D.size(0)) */
    int32_t D;              /* active SH degree 0..3 */
    int32_t M;              /* SH coefficients per Gaussian (sh.size(1)); 0 when colours are precomputed */
    int32_t W, H;           /* image size */
    int32_t prefiltered;    /* accepted, unused (reference only traps on it) */
    int32_t debug;          /* accepted, unused */
    float tanfovx, tanfovy;
    float cx, cy;           /* principal point in pixels */
    float scale_modifier;
    float color_sigma;      /* radius = ceil(color_sigma * sqrt(lambda_max)) */
    float opaque_threshold; /* alpha of the first Gaussian that fixes the depth */
    float depth_threshold;  /* hit_depth_threshold */
    float normal_threshold; /* hit_normal_threshold = cos(angle) */
    float T_threshold;
} DqoRastParams;

/* Borrowed device inputs.  Exactly one of (shs, colors_precomp) is non-NULL.  scales and rotations are required: the
 * reference's blend kernel dereferences them unconditionally (forward.cu:780), so cov3D_precomp-only calls are rejected
 * with DQO_ERR_INVALID_ARG instead of faulting. */
typedef struct DqoRastInputs {
    const float* bg;             /* [3] */
    const float* means3D;        /* [P,3] */
    const float* shs;            /* [P,M,3] or NULL */
    const float* colors_precomp; /* [P,3] or NULL */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3] */
    const float* rotations;      /* [P,4] (r,x,y,z), already normalised by the caller */
    const float* cov3D_precomp;  /* must be NULL */
    const float* viewmatrix;     /* [16] */
    const float* projmatrix;     /* [16] */
    const float* campos;         /* [3] */
    const int32_t* tile_mask;    /* [ceil(H/16) * ceil(W/16)], non-zero = render; NULL = all ones */
    /* ABI 5.  NULL (the drop-in behaviour: every row is rendered) or one byte per Gaussian; a row with DQO_ROW_HIDDEN set is treated
     * as culled by the per-Gaussian forward (radii 0, no list entry, no gradient) — the reference's two clouds kept in ONE map:
     * Mapping.global_optimization renders the stable cloud alone (SLAM/multiprocess/mapper.py:1199-1204, stable_params), local_optimize
     * renders cat(unstable, stable) (:578, :1810-1840).  Device memory, read when the launch runs: a captured iteration follows a
     * caller that rewrites the bytes in place between two mapping calls.  The same array serves DqoAdamStep.row_flags. */
    const uint8_t* row_flags;
} DqoRastInputs;
#define DQO_ROW_FROZEN 1u /* DqoAdamStep.row_flags: the row is not trained (no gradient row, no Adam, no confidence count) */
#define DQO_ROW_HIDDEN 2u /* DqoRastInputs.row_flags: the row is not rendered */

/* Caller-allocated outputs; the forward writes EVERY element (masked / empty tiles get the reference's initial
 * fills: colour 0, depth 0, ids 0, weights 0, T 1 — rasterize_points.cu:79-89), so torch.empty is enough. */
typedef struct DqoRastOutputs {
    float* out_color;            /* [3,H,W] */
    float* out_depth;            /* [1,H,W] */
    int32_t* out_hit_color;      /* [1,H,W] id of the max-weight colour contributor, -1 if none */
    int32_t* out_hit_depth;      /* [1,H,W] id of the Gaussian that fixed the depth, -1 if none */
    float* out_hit_color_weight; /* [1,H,W] */
    float* out_hit_depth_weight; /* [1,H,W] */
    float* out_T;                /* [1,H,W] */
    int32_t* n_touched;          /* [P] */
    int32_t* radii;              /* [P] */
} DqoRastOutputs;

/* Forward->backward context: the three opaque byte buffers the reference keeps as geomBuffer / binningBuffer /
 * imgBuffer (rasterize_points.cu:93-98).  Layout is private to this library; sizes come from the functions below. */
/* Optional loss tap of the mapping iteration (row f2; SLAM/multiprocess/mapper.py:836-875 with a render mask): the masked
 * 0.8 L1 colour + 1.0 depth L1 loss is evaluated where its inputs are produced and consumed instead of in two passes over the
 * images between forward and backward.  The forward's blend kernel adds up, per 8x8-pixel wave, |colour error| over the mask and
 * |depth error| over the valid depth pixels (fixed point: exact, order-independent, reproducible) and the two pixel counts.  The
 * backward's blend kernel reads the totals, forms each pixel's dL/dcolour and dL/ddepth from the rendered and the ground-truth
 * images as sign(error) x {color_weight / (3 n_colour), depth_weight / n_depth} — bit for bit what dqo_map_loss_fwd_bwd would have
 * written — so its dL_dout_color / dL_dout_depth arguments are not read (may be NULL), and writes loss_out[8] (same layout as
 * dqo_map_loss_fwd_bwd) and grad_scale[2] (the two factors): the loss is available after the BACKWARD call.  All pointers are
 * device pointers and must stay valid from the forward to the backward; out_color / out_depth are the forward's own outputs. */
typedef struct DqoLossTap {
    const float* gt_color;      /* [3,H,W] */
    const float* gt_depth;      /* [1,H,W] */
    const uint8_t* render_mask; /* [H,W] or NULL (= all pixels) */
    const float* out_color;     /* [3,H,W] = DqoRastOutputs.out_color of the forward (read by the backward) */
    const float* out_depth;     /* [1,H,W] = DqoRastOutputs.out_depth */
    float color_weight, depth_weight, add_depth_thres;
    float* loss_out;            /* [8] */
    float* grad_scale;          /* [2] */
    /* ABI 3.  0: ONE masked loss over all mask pixels (the reference's loss_update with a render mask, mapper.py:836-875).
     * non-zero, with DqoRastCtx.object_gate: the loss of the per-object job of SURVEY.md §8(e),  L = sum_k L_k,  L_k = the same masked
     * loss evaluated on object k's pixels alone (pixel_object == k inside the mask), each term normalised by ITS OWN pixel counts — so
     * that the loss (and every gradient) of an object does not depend on which other objects the caller renders with it: shards of one
     * map add up to the unsharded job exactly.  loss_out[0..2] = sum_k of (total, colour, depth); [4..7] the raw sums over all objects;
     * grad_scale is not written (the scales are per object).  Object ids must lie in [0, 64). */
    int32_t per_object;
} DqoLossTap;

/* Optional object gate (ABI 3; not a feature of the reference, whose renders composite every Gaussian of a ray — F3).  With it a list
 * entry acts on a pixel only if gaussian_object[id] == pixel_object[pixel] (a negative pixel id: no entry acts), in the forward and in
 * the backward: every pixel sees the render of its own object alone, whatever other Gaussians the call holds.  This is what makes the
 * per-object job of SURVEY.md §8(e) ONE function for every number of shards: a shard that owns some of the objects computes exactly its
 * objects' pixels of the unsharded render.  List positions (n_contrib, the hit position) count gated entries like skipped ones.  Both
 * arrays are device pointers and must stay valid from the forward to the backward. */
typedef struct DqoObjectGate {
    const int32_t* gaussian_object; /* [P], ids in [0, 64) */
    const int32_t* pixel_object;    /* [H*W] owner of every pixel, < 0 = none */
    /* Optional (NULL = not used): per 16x16 tile the set of owners among its pixels, bit k = some pixel of the tile has owner k
     * ([ceil(H/16) * ceil(W/16)] 64-bit words, derived from pixel_object by the caller — it only changes when pixel_object does).
     * The binning then drops a (Gaussian, tile) instance whose object owns no pixel of the tile: it could act on none. */
    const uint64_t* tile_objects;
} DqoObjectGate;

typedef struct DqoRastCtx {
    void* geom;
    size_t geom_bytes;
    void* binning;
    size_t binning_bytes;
    void* image;
    size_t image_bytes;
    int64_t inst_capacity; /* number of (Gaussian, tile) instances `binning` can hold */
    /* 0 (default): the per-tile lists are packed back to back by a prefix scan — any list length, `binning` sized by
     * dqo_rast_binning_bytes(inst_capacity).  > 0: every tile owns a fixed bucket of this many list entries (`binning` sized by
     * dqo_rast_binning_bytes_bucketed): the binning kernel writes an instance straight to tile * bucket + rank, no scan and no
     * placement pass sit between it and the sort.  A tile that outgrows its bucket raises the same overflow flag as running out
     * of inst_capacity (outputs invalid, nothing written out of bounds) — for callers that can re-run, like the captured mapping
     * iteration.  Same lists, same order, same results as the packed mode.  Capacity in bucket mode: the instance slots are handed
     * out by up to 64 regional allocators, each owning inst_capacity / regions slots, so a frame is also flagged invalid when ONE
     * region of the map outgrows its share although the total fits — size inst_capacity with headroom (the captured iteration
     * uses 3 x the measured N), or use the packed mode when the capacity is tight. */
    int32_t tile_bucket_capacity;
    /* Bucket mode only.  Non-zero: keep the tile launch order (longest list first, XCD bands) that an earlier forward left in
     * `image` instead of recomputing it — the caller guarantees that a forward with this flag at 0 has run on this `image` buffer
     * for the same W x H (the order only decides which workgroup renders which tile, never a result, so an order computed for a
     * slightly different state of the map is as good).  The one-block scan kernel between binning and sort then disappears: list
     * ranges follow from the tile counters, the header from per-line statistics.  For a captured iteration that is replayed. */
    int32_t keep_tile_order;
    /* NULL (default, the drop-in behaviour) or the loss tap described above; read by the forward and by the backward. */
    const DqoLossTap* loss_tap;
    /* NULL (default: the reference's semantics) or the object gate described above; read by the forward and by the backward. */
    const DqoObjectGate* object_gate;
    /* 0 (default): every 8x8-pixel quadrant of a tile blends its list front to back (and walks it back to front) in ONE wave, the
     * reference's order of arithmetic.  n > 0: lists longer than n entries (n < 64 counts as 64) are shared between eight waves — rounds
     * of eight chunks of 64 entries: per chunk the composed map of the per-pixel state (forward: the product of (1 - alpha) and "holds an
     * opaque hit"; backward: the scale of T and the affine map of the colour blended behind), a scan over the round, then the blend /
     * walk of every chunk from its scanned start state — for launches that cannot fill the GPU, a strong-scaling shard of a few hundred
     * tiles, whose time is the time of the one longest list.  Read by the forward AND by the backward call: the forward builds the
     * queue of long lists, the backward (given n > 0 too) walks that queue with eight waves per quadrant (and every shorter list exactly
     * like a backward given 0: same kernel code, same bits); a backward given 0 walks every list in one wave whatever the forward did.  The state is grouped by chunk, so results on those lists differ from the serial order
     * in the last bits (1e-7 relative; a pixel exactly on T_threshold may finish one entry earlier or later); shorter lists are treated
     * as with 0. */
    int32_t list_split;
    /* ABI 4.  Non-zero: the caller guarantees that the per-frame scalars of ctx.geom (slot allocator, queue counters, statistics lines,
     * loss-tap counters) are zero — as dqo_rast_backward_adam leaves them: its per-Gaussian kernel, the LAST consumer of a frame's
     * counters, clears them for the next frame on the way — so the forward does not launch its zero-fill kernel.  For a captured iteration that is
     * replayed back to back (forward, dqo_rast_backward_adam, forward, ...) on one context: one launch less per iteration.  Ignored when
     * P == 0.  The device header (num_rendered ... overflow) is never cleared: every frame rewrites it.
     * Round 5: that kernel also clears the tile histogram and tile flags of ctx.image and leaves a stamp behind; with per-tile buckets
     * (tile_bucket_capacity > 0) a pre-zeroed frame then has no per-Gaussian preprocess launch either — its statements run at the head of
     * the binning kernel (csrc/dqo_k1_early.h) — and, with buckets of at most 1024 entries and keep_tile_order, no long-list sort launch.
     * A frame that finds no stamp (the promise was broken: a forward-only render, dqo_rast_backward or an error return in between) is
     * flagged in header.overflow and trains nothing; the frame after it is valid again.  Between dqo_rast_forward_prepare and
     * dqo_rast_forward_render of such a frame the stage-1 statistics are not available yet (dqo_rast_read_header reports zeros): use
     * dqo_rast_forward / dqo_rast_forward_async.
     * Round 6: dqo_rast_backward reads the field too.  Non-zero there (and list_split == 0): its per-Gaussian kernel — the last
     * consumer of the frame's counters in that call — clears the same words and leaves the same stamp, so the NEXT forward on the
     * context may be given frame_prezeroed: the drop-in operator's pooled contexts (forward, dqo_rast_backward, forward, ...).  A second
     * dqo_rast_backward over the same forward (retain_graph) is fine: nothing it reads is cleared.  0 (default): nothing is cleared. */
    int32_t frame_prezeroed;
} DqoRastCtx;

/* Gradients (all caller-allocated, fully written by the backward; rasterize_points.cu:198-206).  dL_dcolors, dL_dcov3D and
 * dL_dmeans2D may be NULL when the caller has no use for them (the fused mapping step: no precomputed colours or covariances,
 * no densification statistics) — three scattered partial-line stores per visible Gaussian less. */
typedef struct DqoRastGrads {
    float* dL_dmeans3D;   /* [P,3] */
    float* dL_dsh;        /* [P,M,3] (NULL when M == 0) */
    float* dL_dcolors;    /* [P,3] or NULL */
    float* dL_dopacity;   /* [P,1] */
    float* dL_dscales;    /* [P,3] */
    float* dL_drotations; /* [P,4] */
    float* dL_dcov3D;     /* [P,6] or NULL */
    float* dL_dmeans2D;   /* [P,3] (x,y used; z = 0) or NULL */
    /* 0 (the drop-in behaviour): every row is written, zeros for the Gaussians the forward culled (radii == 0).
     * non-zero: those all-zero rows are left unwritten — for a consumer that looks at radii itself
     * (dqo_map_adam_step with DqoAdamStep.radii) this saves writing and re-reading 236 B per culled Gaussian. */
    int32_t skip_culled_rows;
} DqoRastGrads;

/* Host-visible copy of the device header kept at the start of ctx.geom. */
typedef struct DqoRastHeader {
    uint32_t num_rendered;   /* N: (Gaussian, tile) instances kept in the tile lists (valid after stage 2) */
    uint32_t num_tiles;      /* active (non-empty, unmasked) tiles */
    uint32_t overflow;       /* non-zero: N exceeded inst_capacity, results of this forward are invalid */
    uint32_t max_tile_count; /* longest per-tile list */
    uint32_t num_visible;    /* Gaussians with radius > 0 */
    uint32_t num_candidates; /* (Gaussian, tile) pairs inside the tile rects = the reference's num_rendered
                                (rasterizer_impl.cu:303-309); an upper bound of N, valid after stage 1 */
    uint32_t stage;          /* 1 after stage 1 (only num_visible / num_candidates are meaningful), 2 once stage 2 has written the
                                frame's header; dqo_rast_read_header reports the device header as it is at stage 2 */
    uint32_t reserved;
} DqoRastHeader;

int dqo_abi_version(void);
const char* dqo_last_error(void);
/* sizeof() of the ABI structs as this library was compiled (a binding checks its own struct definitions against it):
 * 0 DqoRastParams, 1 DqoRastInputs, 2 DqoRastOutputs, 3 DqoRastCtx, 4 DqoRastGrads, 5 DqoRastHeader, 6 DqoProfileEntry,
 * 7 DqoAdamStep, 8 DqoLossTap, 9 DqoObjectGate, 10 DqoAdamTensor, 11 DqoRastParamInputs, 12 DqoRastParamGrads, 14 DqoLifecycle, 15 DqoGrowthSample; 0 for
 * any other index (13 stays unused: bindings probe it for the end of the parameter-form structs). */
size_t dqo_abi_sizeof(int32_t which);

/* Optional per-kernel timing (measurement only; the reference has nothing comparable — it times whole frames with
 * time.time(), utils/monitor.py:22-37).  While enabled every kernel launch of this library is bracketed by HIP events
 * recorded on the launch stream; dqo_profile_collect waits for them and returns accumulated milliseconds per kernel. */
typedef struct DqoProfileEntry {
    char name[48];
    double total_ms;
    uint32_t calls;
} DqoProfileEntry;
int dqo_profile_enable(int on);
int dqo_profile_collect(DqoProfileEntry* out, int max_entries, int reset);

size_t dqo_rast_geom_bytes(int32_t P, int32_t W, int32_t H);
size_t dqo_rast_image_bytes(int32_t W, int32_t H);
size_t dqo_rast_binning_bytes(int64_t inst_capacity);
size_t dqo_rast_binning_bytes_bucketed(int64_t inst_capacity, int32_t W, int32_t H, int32_t tile_bucket_capacity);
size_t dqo_rast_backward_workspace_bytes(int64_t inst_capacity);

/* Stage 1 (per-Gaussian preprocess).  Needs ctx.geom and ctx.image; leaves num_candidates (>= N) in the device
 * header: the capacity a caller that wants a guaranteed fit allocates.  rasterizer_impl.cu:272-307 (K1, K2). */
int dqo_rast_forward_prepare(const DqoRastParams*, const DqoRastInputs*, DqoRastOutputs*, DqoRastCtx*, void* hipStream);
/* D2H read of the header (the ONLY synchronising call; replaces the reference's cudaMemcpy at rasterizer_impl.cu:307).  After
 * stage 1 (header.stage == 1): num_visible and num_candidates, everything else 0.  After stage 2 (stage == 2): the device header as
 * the frame's sort kernels wrote it — still valid after dqo_rast_backward / dqo_rast_backward_adam, which clear the counters the
 * header was formed from but not the header. */
int dqo_rast_read_header(const DqoRastCtx*, DqoRastHeader* host_out, void* hipStream);
/* Stage 2 (footprint test + tile binning, per-tile sort, blend).  Needs ctx.binning with inst_capacity >= N, otherwise
 * the device header's overflow flag is raised, nothing is written out of bounds and the outputs are invalid.
 * Stage 2 reads the inputs again (means3D, scales, rotations, shs / colors_precomp: the colour / surfel-normal part of the
 * per-Gaussian forward rides in the sort launches): a two-stage caller passes the SAME, unmodified, still-alive input arrays to
 * both stages.  With ctx.frame_prezeroed the caller promises that the previous frame on this ctx ended in dqo_rast_backward_adam
 * (the only call that restores the zeroed per-frame scalars); any other sequence must leave the flag at 0.
 * rasterizer_impl.cu:309-440 (K3-K6). */
int dqo_rast_forward_render(const DqoRastParams*, const DqoRastInputs*, DqoRastOutputs*, DqoRastCtx*, void* hipStream);
/* Both stages back to back, no host synchronisation (caller guarantees / later checks capacity). */
int dqo_rast_forward(const DqoRastParams*, const DqoRastInputs*, DqoRastOutputs*, DqoRastCtx*, void* hipStream);
/* As dqo_rast_forward, in the training form: for an iteration whose render nobody reads — its backward, loss tap and per-Gaussian tail
 * are its only consumers (the inner iterations of a graph that holds several: FusedMapper.capture(unroll=k)).  Writes out_color,
 * out_depth and radii and the whole forward->backward context; leaves out_hit_color, out_hit_depth, out_hit_color_weight,
 * out_hit_depth_weight, out_T and n_touched UNTOUCHED (not even zeroed), and skips the work that only they need.  The struct is checked
 * like dqo_rast_forward's (no NULL member).  Needs ctx.loss_tap (without it the loss kernels read out_hit_depth) and list_split == 0. */
int dqo_rast_forward_train(const DqoRastParams*, const DqoRastInputs*, DqoRastOutputs*, DqoRastCtx*, void* hipStream);

/* Both stages in ONE call for a caller that carries its instance capacity over from earlier frames and checks it afterwards (ABI 4; the
 * drop-in op's 'lazy' / 'deferred' modes): as dqo_rast_forward, plus — where the frame's header is final, behind the sort kernels and
 * BEFORE the blend kernel — an asynchronous copy of the 32-byte device header to `header_host` (pinned host memory; NULL: no copy) and
 * hipEventRecord(header_event) on the launch stream (a hipEvent_t; NULL: none).  When the event has completed, header_host->overflow says
 * whether ctx.inst_capacity held the frame (num_rendered, num_tiles, max_tile_count, num_visible and num_candidates are final
 * too) — about one blend kernel earlier than a copy issued behind the call would.  Replaces the reference's blocking
 * cudaMemcpy of rasterizer_impl.cu:307 like dqo_rast_read_header does, without the host wait. */
int dqo_rast_forward_async(const DqoRastParams*, const DqoRastInputs*, DqoRastOutputs*, DqoRastCtx*, DqoRastHeader* header_host,
                           void* header_event, void* hipStream);

/* rasterizer_impl.cu:445-564 (K7-K9).  `hit_image` is out_hit_depth of the forward ([H*W]); workspace holds the
 * per-instance gradient records. */
int dqo_rast_backward(const DqoRastParams*, const DqoRastInputs*, const DqoRastCtx*, const float* dL_dout_color,
                      const float* dL_dout_depth, const int32_t* hit_image, DqoRastGrads*, void* workspace,
                      size_t workspace_bytes, void* hipStream);

int dqo_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* hipStream);

/* The parameter form (symbols-only addition to ABI 5): the same operator fed with the map's RAW parameters, as DQO-MAP stores them
 * (SLAM/gaussian_pointcloud.py: _features_dc, _features_rest, _opacity, _scaling, _rotation), with the activations of
 * :732-733, 746-747, 815-822 (sigmoid, exp, F.normalize) and the SH concatenation done inside the per-Gaussian kernels — no extra
 * launch, the same bits as dqo_map_activate followed by the activated form.  The DqoRastInputs given with it must have shs, opacities,
 * scales and rotations NULL (they come from here) and colors_precomp NULL (not supported in this form); params->M must be 1 + rest. */
typedef struct DqoRastParamInputs {
    const float* features_dc;   /* [P,1,3]  SH coefficient 0 */
    const float* features_rest; /* [P,rest,3] coefficients 1 .. rest (NULL when rest == 0) */
    int32_t rest;               /* coefficients in features_rest: 1 + rest >= (D+1)^2 */
    const float* opacity_raw;   /* [P,1] logit:         opacity = sigmoid(x) */
    const float* scaling_raw;   /* [P,3] log scale:     scale = exp(x) */
    const float* rotation_raw;  /* [P,4] (r,x,y,z), not normalised: rotation = x / max(|x|, 1e-12) */
} DqoRastParamInputs;

/* Gradients w.r.t. the raw parameters (the activation Jacobians applied in registers).  Given with a DqoRastGrads whose dL_dsh,
 * dL_dopacity, dL_dscales and dL_drotations are NULL (dL_dmeans3D stays there, dL_dcolors must be NULL). */
typedef struct DqoRastParamGrads {
    float* dL_dfeatures_dc;   /* [P,1,3] */
    float* dL_dfeatures_rest; /* [P,rest,3] (NULL when rest == 0); coefficients above the active degree get zeros */
    float* dL_dopacity_raw;   /* [P,1] */
    float* dL_dscaling_raw;   /* [P,3] */
    float* dL_drotation_raw;  /* [P,4] */
} DqoRastParamGrads;

int dqo_rast_forward_prepare_params(const DqoRastParams*, const DqoRastInputs*, const DqoRastParamInputs*, DqoRastOutputs*, DqoRastCtx*,
                                    void* hipStream);
int dqo_rast_forward_render_params(const DqoRastParams*, const DqoRastInputs*, const DqoRastParamInputs*, DqoRastOutputs*, DqoRastCtx*,
                                   void* hipStream);
int dqo_rast_forward_async_params(const DqoRastParams*, const DqoRastInputs*, const DqoRastParamInputs*, DqoRastOutputs*, DqoRastCtx*,
                                  DqoRastHeader* header_host, void* header_event, void* hipStream);
int dqo_rast_backward_params(const DqoRastParams*, const DqoRastInputs*, const DqoRastParamInputs*, const DqoRastCtx*,
                             const float* dL_dout_color, const float* dL_dout_depth, const int32_t* hit_image, DqoRastGrads*,
                             DqoRastParamGrads*, void* workspace, size_t workspace_bytes, void* hipStream);

/* Exact 3-NN: mean of the 3 smallest squared distances and the 3 neighbour indices (ascending distance, ties by
 * Morton order, INT_MAX / FLT_MAX when fewer than 3 other points exist). */
size_t dqo_knn3_workspace_bytes(int32_t P);
int dqo_knn3(int32_t P, const float* xyz, float* mean_d2, int32_t* idx3, void* workspace, size_t workspace_bytes,
             void* hipStream);

/* Row f3: exact K = 3 nearest REFERENCE points of every QUERY point (Mapping.temp_points_filter, SLAM/multiprocess/mapper.py:
 * 1351-1380 -> pytorch3d.ops.knn_points(K=3, norm=2)): dist2[Q,3] squared L2 distances ascending, idx3[Q,3] indices into the
 * reference set (FLT_MAX / -1 when it has fewer than 3 points).  Ties between equally distant references are resolved
 * arbitrarily. */
size_t dqo_knn3_query_workspace_bytes(int32_t Q, int32_t R);
int dqo_knn3_query(int32_t Q, const float* query_xyz, int32_t R, const float* ref_xyz, float* dist2, int32_t* idx3, void* workspace,
                   size_t workspace_bytes, void* hipStream);
/* ABI 4: the same search restricted to references closer than max_dist (> 0): a slot no such reference fills comes back as FLT_MAX / -1.
 * For callers whose decision saturates beyond a distance (the growth step's per-object decisions, dqo_mapgrowth: a neighbour further than
 * 0.087 m + 3 x its radius clips the scale like a missing one): the search starts from that bound instead of an open one, so a query with
 * no reference nearby prunes the whole map at once.  Same workspace as dqo_knn3_query. */
int dqo_knn3_query_within(int32_t Q, const float* query_xyz, int32_t R, const float* ref_xyz, float max_dist, float* dist2, int32_t* idx3,
                          void* workspace, size_t workspace_bytes, void* hipStream);
/* Row f3, the per-object job (not a reference feature): the same search where a reference point only counts for a
 * query of the SAME GROUP (int32 ids in [0, 64) — the Gaussians' object ids; any other value: the point belongs to no group and is
 * neither found nor finds anything) and, when `group_box` is given ([64][6] floats: lo xyz, hi xyz per group), only if it lies strictly
 * inside its group's box (SLAM/utils.py:801-808 bbox_filter, per object).  One search over the map as it is stored: no shifted copies,
 * no gathered subsets.  At most 2^25 - 1 reference points.  Same workspace as dqo_knn3_query. */
int dqo_knn3_query_grouped(int32_t Q, const float* query_xyz, const int32_t* query_group, int32_t R, const float* ref_xyz,
                           const int32_t* ref_group, const float* group_box, float max_dist, float* dist2, int32_t* idx3, void* workspace,
                           size_t workspace_bytes, void* hipStream);

/* Row f, the per-object job's temp_points_attach (SLAM/multiprocess/mapper.py:1384-1430; not a reference binding: the reference runs the
 * decision as a chain of torch ops) in two launches around the gated render of the stable cloud.
 *   dqo_attach_pixels: candidate n -> lin[n] = its pixel v * W + u (get_uv, scene/cameras.py:207-214: trunc(K (R x + t) / z); -1 = outside
 *     the image), and the sparse object gate of that render, both fully written: sparse_pixel_object [H*W] = pixel_object where a candidate
 *     projects, -1 elsewhere; tile_objects [ceil(H/16) * ceil(W/16)] = per tile the 64-bit set of the owners among those pixels
 *     (DqoObjectGate.pixel_object / .tile_objects).  viewmatrix: the 16 floats DqoRastInputs.viewmatrix takes; fx, fy, cx, cy: pixels.
 *   dqo_attach_decide: out[n] = 1 iff opacity[n] > opacity_low, the candidate is inside the image, hit_index at its pixel names a
 *     Gaussian s >= 0 (index 0 with hit_weight 0 = the op's zero fill: no hit) of the candidate's object, and
 *     |(xyz[s] - temp_xyz[n]) . normal(s)| < plane_thr (normal: SLAM/gaussian_pointcloud.py:780-791 from the raw quaternion and raw
 *     scales).  hit_index / hit_weight: DqoRastOutputs.out_hit_color / out_hit_color_weight of the gated render. */
int dqo_attach_pixels(int32_t n, const float* temp_xyz, const float* viewmatrix, float fx, float fy, float cx, float cy, int32_t W, int32_t H,
                      const int32_t* pixel_object, int32_t* lin, int32_t* sparse_pixel_object, uint64_t* tile_objects, void* hipStream);
int dqo_attach_decide(int32_t n, const float* temp_xyz, const float* temp_opacity, const int32_t* temp_object, const int32_t* lin,
                      const int32_t* hit_index, const float* hit_weight, const float* xyz, const float* scaling_raw,
                      const float* rotation_raw, const int32_t* gaussian_object, float plane_thr, float opacity_low, uint8_t* out,
                      void* hipStream);

/* Row f, small per-point kernels of the growth step (each replaces a chain of element-wise torch ops of the reference's callers; the
 * step is bound by the host's op issue rate):
 *   dqo_growth_scales: GaussianPointCloud.update_geometry's scale initialisation (SLAM/gaussian_pointcloud.py:519-556) behind its two
 *     searches, per-object job: for new point i the candidates are i_new[i][0..2] (indices among the n new points from dqo_knn3 on
 *     object-shifted coordinates; >= n: none; a neighbour counts if it has i's object id and lies within sqrt(reach2) — the distance is
 *     recomputed from xyz) and (d2_old, i_old)[i][0..2] (dqo_knn3_query_grouped against the existing map; i_old < 0: none); the three
 *     nearest give gaps g = dist - 3 * radius (radius / extra_radius of the neighbour); invalid = any g < 0; scale =
 *     clip(sqrt(mean g^2), min_radius, max_radius).  i_new or i_old may be NULL (no such search).
 *   dqo_growth_inside: Mapping.temp_points_filter's decision (SLAM/multiprocess/mapper.py:1372-1380): inside[i] = some idx[i][k] >= 0
 *     with sqrt(d2[i][k]) < 0.6 * radius[idx[i][k]].
 *   dqo_error_maps: the per-pixel error images of mapper.py:1016-1033 for dqo_accumulate_gaussian_error: depth_err = max(gt_depth -
 *     depth, 0), color_err = sum over channels |gt_color - render|; both 0 where gt_depth == 0 or mask == 0 (mask NULL = all), depth_err
 *     also where depth_index == -1.  Images are [C, H*W] planes. */
int dqo_growth_scales(int32_t n, const float* xyz, const int32_t* object, const float* radius, const int32_t* i_new, const float* d2_old,
                      const int32_t* i_old, const float* extra_radius, float reach2, float min_radius, float max_radius, float* scales,
                      uint8_t* invalid, void* hipStream);
int dqo_growth_inside(int32_t n, const float* d2, const int32_t* idx, const float* radius, uint8_t* inside, void* hipStream);
int dqo_error_maps(int32_t H, int32_t W, const float* gt_color, const float* gt_depth, const float* render, const float* depth,
                   const int32_t* depth_index, const uint8_t* mask, float* color_err, float* depth_err, void* hipStream);

/* Map maintenance: the three statements that close every frame of the reference mapper (SLAM/multiprocess/mapper.py:217-219, and :214 on
 * optimise frames) on ONE map whose rows carry a `stable` flag instead of living in two clouds, rewritten in place, nothing read back:
 *     gaussians_fix()            :657-676    unstable -> stable once confidence > stable_confidence_thres (strict; confidence clipped to it)
 *     error_gaussians_remove()   :989-1102   per-Gaussian error of a render of the whole map -> strike counters -> delete / release (:679-689)
 *     gaussians_delete()         :692-730    oversized (radius > 10 x the cloud's mean radius) or too-long-unstable rows leave the map
 *
 * dqo_map_lifecycle_vote (one launch, one thread per pixel; images are [C, H*W] planes, index maps the op's hit_color / hit_depth):
 *   de = gt_depth - depth where that is > 0, else 0, and 0 where gt_depth == 0 or depth_index == -1; ce = (|dr| + |dg|) + |db|, 0 where
 *   gt_depth == 0 (:1015-1026).  The reference scatters a per-Gaussian maximum and tests `max > 2 x thres` (:1029-1068), which holds exactly
 *   when some pixel exceeds it: a pixel with de > 2 x add_depth_thres sets bit 0 of vote[depth_index], one with ce > 2 x add_color_thres
 *   bit 1 of vote[color_index] (integer atomic OR; indices outside [0, P) are ignored).  No error image, no float accumulator.  The
 *   normal error is identically zero in the reference (:1020) and is not formed.
 * dqo_map_lifecycle_rows (two launches, three with stable_oversized; one thread per row; rows with alive == 0 take part in nothing):
 *   0. stable_oversized (gaussians_delete(unstable=False), :214): stable rows with radius > 10 x the stable cloud's mean radius are deleted;
 *   1. gaussians_fix: an unstable row with confidence > stable_confidence_thres becomes stable, its confidence the threshold;
 *   2. use_votes (error_gaussians_remove): on the rows that are stable now, vote bit 0 / 1 adds one to depth_error_counter /
 *      color_error_counter; depth_error_counter >= delete_thresh deletes the row, otherwise color_error_counter >= delete_thresh releases
 *      it (stable = 0, confidence = 0, add_tick = tick).  A released row keeps both counters, as the reference's remove() / cat() carry
 *      them (gaussian_pointcloud.py:235-293, 415-432).  Every vote word is cleared as it is read;
 *   3. gaussians_delete(unstable=True): unstable rows (released ones included) with radius > 10 x the unstable cloud's mean radius or
 *      tick - add_tick > unstable_time_window are deleted.
 *   radius = (sum exp(scaling_raw) - min exp(scaling_raw)) / 2 (get_radius, gaussian_pointcloud.py:739-743).  Each mean is over the
 *   membership the earlier statements left (an empty cloud deletes nothing, :697): per block a double partial sum and a count, added in
 *   index order by the block that takes the last integer ticket, rounded to float once, x 10 in float — no float atomics, the same bits on
 *   every run.  Deleting a row writes what a spare row holds and nothing else: xyz = park, opacity_raw = scaling_raw = -10, alive = 0,
 *   row_flags = DQO_ROW_HIDDEN | DQO_ROW_FROZEN, confidence = 0, and 0 into stable / add_tick / both counters.
 *   stats[8] (the frame's counts, overwritten): promoted, released, deleted by depth, deleted oversized-unstable, deleted by time (and
 *   not oversized), deleted oversized-stable, unstable rows left, stable rows left.
 * workspace: dqo_map_lifecycle_workspace_bytes(P) bytes, ZERO when first used and then left to these calls (they hand it back ready for
 * the next frame); vote [P] likewise. */
typedef struct DqoLifecycle {
    int32_t P, W, H;
    int32_t tick;                  /* the mapper's `time` */
    int32_t unstable_time_window, delete_thresh;
    int32_t stable_oversized;      /* non-zero: statement 0 */
    int32_t use_votes;             /* non-zero: statement 2 (0: the reference's early return, no stable Gaussian / no processed frame) */
    float stable_confidence_thres, add_color_thres, add_depth_thres;
    float* xyz;                    /* [P,3] */
    float* opacity_raw;            /* [P] */
    float* scaling_raw;            /* [P,3] */
    float* confidence;             /* [P] */
    uint8_t* alive;                /* [P] */
    uint8_t* row_flags;            /* [P] */
    uint8_t* stable;               /* [P] */
    int32_t* add_tick;             /* [P] */
    int32_t* depth_error_counter;  /* [P] */
    int32_t* color_error_counter;  /* [P] */
    const float* park;             /* [3] where deleted rows are parked (device memory) */
    uint32_t* vote;                /* [P] */
    void* workspace;
    size_t workspace_bytes;
    int32_t* stats;                /* [8] */
    const DqoRastHeader* render_header; /* dqo_map_lifecycle_vote: the device header of the forward that rendered the images (the start of its
                                      geometry buffer), or NULL.  A frame that overflowed its capacity (header.overflow != 0: invalid
                                      outputs) casts no vote. */
} DqoLifecycle;
size_t dqo_map_lifecycle_workspace_bytes(int32_t P);
int dqo_map_lifecycle_vote(const DqoLifecycle* step, const float* gt_color, const float* gt_depth, const float* render_color,
                           const float* render_depth, const int32_t* depth_index, const int32_t* color_index, void* hipStream);
int dqo_map_lifecycle_rows(const DqoLifecycle* step, void* hipStream);

/* Map growth, the first statement: Mapping.temp_points_init (SLAM/multiprocess/mapper.py:1231-1347) with sample_pixels (SLAM/utils.py:145-212)
 * and GaussianPointCloud.add_empty_points (SLAM/gaussian_pointcloud.py:445-517) — from one RGB-D frame (and a render of the map) to the
 * candidate rows FusedMapper.grow(new=...) takes.  Seven small launches, nothing read back, every k formed on the device.
 *
 * Masks (one thread per pixel; strip(p) = the normal's components sum to non-zero, and with an instance image its components too —
 * what sample_pixels writes INTO its select_mask argument, utils.py:169-174):
 *   first_frame:  draw 0 over depth > 0 (mapper.py:1235), k = uniform_sample_num.
 *   otherwise:    draw 1 over trans = (T > add_transmission_thres) & (depth > 0) (:1251-1253),
 *                   k = trunc((transmission_sample_ratio * (float(sum trans) / float(H * W))) * float(uniform_sample_num)), float32, the sum
 *                   taken BEFORE the strip (:1254-1262);
 *                 draw 2 over ((|depth - render_depth| > add_depth_thres & depth > 0 & depth_index > -1) | (mean3 |color - render_color| >
 *                   add_color_thres & depth > 0 & T < add_transmission_thres)) & ~trans (:1292-1326), with trans AFTER the strip the
 *                   redundant first sample_pixels call (:1269) left in it — unless draw 1's k is 0, when that call returns before it
 *                   touches the mask (utils.py:155-156); k = trunc(float(sum mask) * error_sample_ratio) before the strip (:1327).
 *   mean3 = ((a + b) + c) / 3; every k is clamped to its mask's count after the strip (utils.py:176-177).
 * Selection (replaces the CPU torch.randperm of utils.py:185, same distribution): every pixel of a draw's stripped mask gets
 *   key = hash32(seed, draw, pixel) & (2^key_bits - 1) (csrc/dqo_sample_hash.h); chosen are the k smallest (key, pixel) pairs; rows come out
 *   in ascending pixel index, draw 1's before draw 2's (:1288, 1345).  A radix select over three digits of the key — never a sort.
 * Rows (add_empty_points): normal / (|normal| + 1e-8) with |n| = sqrt(fma(z, z, fma(y, y, x * x))); a row whose normalised components sum
 *   ((x + y) + z) to exactly 0 is dropped (:457); shs[row][0] = (color - 0.5) / C0, the other M - 1 coefficients 0; scales 1e-6; opacity
 *   init_opacity; rotation (1, 0, 0, 0) with identity_rotation, else compute_rot((0, 0, 1), normal) (utils.py:246-251,
 *   utils/general_utils.py:185-191, both + 1e-8 normalisations); obj_id = int(instance[0] * 255) (:497); pixel = y * W + x.
 * Images are the reference's [H, W, C] layouts except render_color, which is the renderer's [3, H * W] planes.
 * header (8 x int32, overwritten): 0 / 2 pixels of draw A / B's mask before the strip, 1 / 3 after it, 4 / 5 the clamped k of A / B,
 *   6 rows written, 7 overflow (non-zero: more than `capacity` rows — rows beyond the capacity are not written).  A = draw 0 or 1, B = draw 2.
 * workspace: dqo_growth_sample_workspace_bytes(W, H) bytes, any contents. */
typedef struct DqoGrowthSample {
    int32_t W, H;
    int32_t first_frame;
    int32_t uniform_sample_num;
    int32_t capacity;            /* rows the output buffers hold */
    int32_t key_bits;            /* 1..32 */
    int32_t M;                   /* SH coefficients per row of shs */
    int32_t identity_rotation;   /* non-zero: xyz_factor == (1, 1, 1) */
    uint64_t seed;
    float add_transmission_thres, add_depth_thres, add_color_thres;
    float transmission_sample_ratio, error_sample_ratio, init_opacity;
    const float* vertex;         /* [H*W,3] frame_map["vertex_map_w"] */
    const float* normal;         /* [H*W,3] frame_map["normal_map_w"] */
    const float* color;          /* [H*W,3] frame_map["color_map"] */
    const float* depth;          /* [H*W]   frame_map["depth_map"] */
    const float* instance;       /* [H*W,3] frame_map["instance_img"], or NULL */
    const float* T;              /* [H*W]   model_map["render_transmission"]      (the four below: unused with first_frame) */
    const float* render_depth;   /* [H*W] */
    const float* render_color;   /* [3,H*W] */
    const int32_t* depth_index;  /* [H*W] */
    float* xyz;                  /* [capacity,3] */
    float* scales;               /* [capacity,3] */
    float* rotations;            /* [capacity,4] */
    float* opacity;              /* [capacity] */
    float* shs;                  /* [capacity,M,3] */
    int32_t* obj_id;             /* [capacity], or NULL (written only with an instance image) */
    float* out_normal;           /* [capacity,3] */
    int32_t* pixel;              /* [capacity] */
    int32_t* header;             /* [8] */
    void* workspace;
    size_t workspace_bytes;
} DqoGrowthSample;
size_t dqo_growth_sample_workspace_bytes(int32_t W, int32_t H);
int dqo_growth_sample(const DqoGrowthSample* args, void* hipStream);

/* Keyframe evaluation: the metrics eval_picture reports for one rendered frame (SLAM/eval.py:38-188; called per frame from slam.py:155,
 * 184 and from metric.py) in one launch, nothing read back.  Replaces, statement by statement:
 *     psnr(gt_image, image).mean()                 eval.py:63   (utils/loss_utils.py:23-25: 20 log10(1 / sqrt(mse_c)) per channel)
 *     l1_loss(gt_image, image)                     eval.py:70   (utils/loss_utils.py:27-29)
 *     valid_range_mask, gt_depth[~mask] = 0        eval.py:116-117
 *     invalid_depth_mask, valid_depth_mask         eval.py:120-123   valid = depth_index != -1 && min_depth < gt_depth < max_depth
 *     valid_pixel_ratio                            eval.py:124-125   float32(valid count) / float32(H * W)
 *     l1_loss(depth[valid], gt_depth[valid])       eval.py:126       NaN when no pixel is valid
 * render, gt_color: [3, H*W] planes; depth, gt_depth (metres), depth_index: [H*W].  Every difference is formed in double from the float
 * inputs and every sum is a double: lanes by a fixed butterfly, one partial per block, the partials added in block-index order by the block
 * that takes the launch's last integer ticket.  No float atomic: the row is bitwise reproducible and independent of block scheduling.
 * out + 8 * row receives eight floats: 0 psnr (+inf for identical images), 1 color_loss, 2 depth_loss, 3 valid_pixel_ratio,
 *   4 NOT WRITTEN (the caller's SSIM: dqo_map_ssim_fwd_bwd in value-only mode), 5..7 the mean squared error of r, g, b.
 * render_header (may be NULL): the device header of the forward that rendered the images (the start of its geometry buffer).  A frame
 *   that overflowed its capacity (header.overflow != 0: invalid images) gets NaN in all eight slots, slot 4 included.
 * workspace: dqo_eval_picture_workspace_bytes(W, H) bytes (0 for a bad size), ZERO when first used and then left to this call, which hands it
 *   back ready for the next one — no zero fill per call, so the entry can be captured in a hipGraph.  Calls that share a workspace must be
 *   ordered (one stream). */
size_t dqo_eval_picture_workspace_bytes(int32_t W, int32_t H);
int dqo_eval_picture(int32_t W, int32_t H, const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                     const int32_t* depth_index, float min_depth, float max_depth, const DqoRastHeader* render_header, float* out, int32_t row,
                     void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_eval_ms_ssim (ABI 5, symbols-only addition) — the "ssim" number of eval_picture (SLAM/eval.py:19-25, :64):
 * pytorch_msssim.ms_ssim(image[None], gt[None], data_range=1.0, size_average=True), nothing read back.  render, gt_color: [3, H*W] planes,
 * used as they are (no clamp).  Five levels; a level filters both images, their squares and their product with the separable 11-tap window
 * of utils/loss_utils.py:41-58 as a VALID correlation ([h,w] -> [h-10,w-10]) and takes per channel the means of
 *     cs = (2 s12 + C2) / (s1 + s2 + C2),   ss = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) * cs,     C1 = 0.01^2, C2 = 0.03^2;
 * between levels both images become avg_pool2d(kernel_size = 2, padding = (h % 2, w % 2)) (an odd side shifts the 2 x 2 grid by one and
 * averages a zero into the first row / column; the divisor is always 4).  Factors: F[l][c] = max(mean cs of channel c at level l, 0) for
 * l = 0..3, F[4][c] = max(mean ss at level 4, 0); ms_c = prod_l F[l][c] ** w[l], w = float32 (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).
 * cs and ss are float32 per pixel, as the reference's library; their sums are doubles added in a fixed order (see dqo_eval_picture) and
 * everything from the means on is double, rounded once per slot: a row is bitwise reproducible.
 * out + 20 * row receives twenty floats: 0 ms_ssim = (ms_r + ms_g + ms_b) / 3, 1..3 ms_r, ms_g, ms_b, 4 + 3 l + c the factor F[l][c]
 *   (after the clamp), 19 NaN (unused).
 * render_header (may be NULL): as dqo_eval_picture's — a frame that overflowed its capacity gets NaN in all twenty slots.
 * Both sides must be > 160 (the library's assertion: smaller_side > (11 - 1) * 2^4) and W * H within dqo_eval_picture's limit;
 * dqo_eval_ms_ssim_workspace_bytes returns 0 otherwise, the call DQO_ERR_INVALID_ARG — as for a NULL image or out, or a negative row — and
 * DQO_ERR_WORKSPACE for a workspace that is too small, all before anything is launched.
 * workspace: ZERO when first used and then left to this call, which hands it back ready for the next one — no zero fill, no allocation,
 *   nine launches, capturable in a hipGraph.  It holds the pooled levels 1..4 (about 2 H W floats).  Calls that share a workspace must be
 *   ordered (one stream). */
size_t dqo_eval_ms_ssim_workspace_bytes(int32_t W, int32_t H);
int dqo_eval_ms_ssim(int32_t W, int32_t H, const float* render, const float* gt_color, const DqoRastHeader* render_header, float* out,
                     int32_t row, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_eval_lpips (ABI 5, symbols-only addition) — the "lpips" number of eval_picture (SLAM/eval.py:28-30, :65-68):
 * LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True) of clamp(gt, 0, 1) and clamp(image, 0, 1), a batch of one, on
 * weights the CALLER brings; nothing read back.  Written from the published sources of `lpips` and `torchmetrics` (neither exists on this
 * platform: no value was recorded from them; tests/lpips_oracle.py restates the steps).  image, gt: [3, H*W] planes.
 *   1. per element, float, one rounding per statement: x = clamp(x, 0, 1) (a NaN stays NaN), x = 2 x - 1, s = (x - shift_c) / scale_c,
 *      shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450).  Padding is zero in s-space.
 *   2. five maps f_l = relu(conv2d(in_l) + bias_l): (Cin -> Cout, kernel, stride, pad) = (3 -> 64, 11, 4, 2) on s, (64 -> 192, 5, 1, 2) on
 *      maxpool3/2(f_0), (192 -> 384, 3, 1, 1) on maxpool3/2(f_1), (384 -> 256, 3, 1, 1) on f_2, (256 -> 256, 3, 1, 1) on f_3; the pools
 *      floor mode, unpadded.  Sides: h0 = (H - 7) / 4 + 1, h1 = (h0 - 3) / 2 + 1, h2 = h3 = h4 = (h1 - 3) / 2 + 1 (integer division), so
 *      H, W >= 31.  An output element is ONE float accumulator: 0, then fmaf(x_k, w_k, acc) for k = 0 .. K - 1 in the packed order below
 *      (the f32 MFMA is that chain bit for bit), then + bias, then the ReLU (a NaN stays NaN).
 *   3. per layer and pixel, double, channels in ascending order: na = a / sqrt(1e-8 + sum a^2) (DQO_LPIPS_NORM_TORCHMETRICS, what the
 *      reference calls) or na = a / (sqrt(sum a^2) + 1e-10) (DQO_LPIPS_NORM_LPIPS, the `lpips` package); v = sum_c lin_l[c] (na_c - nb_c)^2.
 *   4. d_l = the mean of v over the layer's pixels: a double sum added in a fixed order (see dqo_eval_picture); lpips = d_0 + .. + d_4 in
 *      double; each slot rounded once to float.
 * out + 8 * row receives eight floats: 0 lpips, 1..5 d_0..d_4, 6 and 7 NaN.  Bitwise reproducible, and symmetric in (image, gt).
 * weights: ONE packed device buffer of dqo_eval_lpips_weight_floats(-1) = 2 470 848 floats (2 468 544 convolution weights, 1 152 biases,
 *   1 152 lin weights), 16-byte aligned.  Per layer, in order: W[k][co] with k = (kh * KW + kw) * Cin + ci (K = Cin * KH * KW rows of Cout
 *   floats), then bias[Cout], then lin[Cout].  Float offsets of (W, bias, lin):
 *     layer 0 (K  363, Cout  64):       0,   23232,   23296        layer 3 (K 3456, Cout 256):  995264, 1880000, 1880256
 *     layer 1 (K 1600, Cout 192):   23360,  330560,  330752        layer 4 (K 2304, Cout 256): 1880512, 2470336, 2470592
 *     layer 2 (K 1728, Cout 384):  330944,  994496,  994880
 *   The k order IS the accumulation order of step 2.
 * render_header (may be NULL): as dqo_eval_picture's — a frame that overflowed its capacity gets NaN in all eight slots.
 * dqo_eval_lpips_workspace_bytes returns 0 for a side below 31 or W * H beyond dqo_eval_picture's limit; the call then returns
 *   DQO_ERR_INVALID_ARG — as for a NULL image, gt, weights or out, weights that are not 16-byte aligned, a negative row or an unknown
 *   norm_mode — and DQO_ERR_WORKSPACE for a workspace that is too small, all before anything is launched.
 * workspace: the ticket words ZERO when first used and handed back at zero; nothing else needs initialising.  No allocation, no
 *   synchronisation, no float atomics; twelve launches (five convolutions, two pools, five heads) on the one stream, capturable in a
 *   hipGraph.  From byte DQO_LPIPS_FEATURES_OFFSET on it holds f_0 .. f_4 of the last call, pixel-major float [2][h_l][w_l][Cout_l]
 *   (0: image, 1: gt), each map's bytes rounded up to a multiple of 256; behind them the pooled maps and the reduction's partials.
 *   Calls that share a workspace must be ordered (one stream). */
#define DQO_LPIPS_NORM_TORCHMETRICS 0
#define DQO_LPIPS_NORM_LPIPS 1
#define DQO_LPIPS_FEATURES_OFFSET 4608
size_t dqo_eval_lpips_weight_floats(int32_t layer); /* layer 0..4: the floats of that layer's W, bias and lin; any other value: all */
size_t dqo_eval_lpips_workspace_bytes(int32_t W, int32_t H);
int dqo_eval_lpips(int32_t W, int32_t H, const float* image, const float* gt, const float* weights, int32_t norm_mode,
                   const DqoRastHeader* render_header, float* out, int32_t row, void* workspace, size_t workspace_bytes, void* hipStream);

/* Dense exact 1-NN between two large sets (scipy's KDTree(ref).query(query) of SLAM/eval.py:190-226, one million points against one
 * million): dist2[i] = the smallest squared distance from query i to any kept reference, idx[i] (may be NULL) a reference attaining it,
 * in the caller's numbering; which one of several equally distant references is arbitrary.  A pair's distance is dx*dx + dy*dy + dz*dz in
 * float, left to right, never contracted: dist2 is a pure function of the inputs — bit for bit the minimum of that expression over all
 * kept references.  dqo_knn3_query gives every query a wave (few scattered queries against a large map); here the queries are sorted
 * along the reference's Morton grid and a wave's 64 lanes hold 64 neighbouring queries that share every box they open.
 * query_keep / ref_keep: NULL = every row; else one byte per row, 0 = the row is neither found nor searched for (a dropped query gets
 *   FLT_MAX / -1) — the mapper's row buffers go in as stored, spare and deleted rows included.  No kept reference (or R = 0): every
 *   query gets FLT_MAX / -1.
 * query_xform / ref_xform: NULL = identity; else 12 floats, a row-major 3x4 transform applied to a row as it is loaded, per output row
 *   ((m0 * x + m1 * y) + m2 * z) + m3 in float, never contracted.
 * At most 2^25 - 1 rows per set (dqo_nn1_workspace_bytes: 0 beyond).  No allocation, no synchronisation, nothing read back; the
 * workspace needs no initialisation. */
size_t dqo_nn1_workspace_bytes(int32_t Q, int32_t R);
int dqo_nn1(int32_t Q, const float* query_xyz, const uint8_t* query_keep, int32_t R, const float* ref_xyz, const uint8_t* ref_keep,
            const float* query_xform, const float* ref_xform, float* dist2, int32_t* idx, void* workspace, size_t workspace_bytes,
            void* hipStream);

/* dqo_nn1_grouped (ABI 5, symbols-only addition) — dqo_nn1 for every object at once: the searches behind metric_obj.py:169-236, which
 * loads each object's cloud and evaluates it against that object's own mesh (one KDTree build and query per object, direction and
 * statement).  A group id is an int32 per row: an id in [0, 64) is the row's object, any other value (-1, 64, ...) means "no object" and
 * the row takes no part on either side — the limit of the object gate's 64 ids and of the 64-bit group sets of the pruning records.
 * dist2[i] = the minimum of dqo_nn1's float expression over the references whose group equals query i's, idx[i] (may be NULL) a reference
 * of that group attaining it; FLT_MAX / -1 for a query without a group or whose group has no reference (or R = 0).  A pure function of
 * the inputs: bit for bit what dqo_nn1 returns with query_keep = (query_group == g) and ref_keep = (ref_group == g), for every g.
 * It is dqo_nn1's search with another source for a row's group: there a keep byte makes the kept rows one object (and without a mask the
 * group tests are compiled out), here an id column names up to 64.  One build of the reference set (points and records carry their
 * groups), one sort of the queries (by group, then by Morton code on the reference's grid) and one scan launch serve every object; a
 * record is opened only for lanes of a group it holds.
 * query_xform / ref_xform, the row limit (dqo_nn1_grouped_workspace_bytes: 0 beyond 2^25 - 1 rows; the bytes are dqo_nn1_workspace_bytes')
 * and the contract — no allocation, no synchronisation, nothing read back, capturable, the workspace needs no initialisation — are
 * dqo_nn1's. */
size_t dqo_nn1_grouped_workspace_bytes(int32_t Q, int32_t R);
int dqo_nn1_grouped(int32_t Q, const float* query_xyz, const int32_t* query_group, int32_t R, const float* ref_xyz, const int32_t* ref_group,
                    const float* query_xform, const float* ref_xform, float* dist2, int32_t* idx, void* workspace, size_t workspace_bytes,
                    void* hipStream);

/* Geometry evaluation: the metrics eval_pcd reports for a reconstruction against a ground-truth point set (SLAM/eval.py:190-282), nothing
 * read back.  Two dqo_nn1 searches (rec -> gt under rec_xform, gt -> rec) and one reduction launch replace the 4 + 2 T KDTree builds and
 * queries of the reference:
 *     accuracy(), completion()                     eval.py:204-215, 273-274   100 * mean distance, in cm
 *     chamfer_distance()                           eval.py:218-226            the two means added, in metres
 *     accuracy_ratio(), completion_ratio(), F1     eval.py:190-201, 264-269   100 * share of rows with distance < th; 2 P R / (P + R)
 * Per kept row d = sqrt((double)dist2), and the threshold test is (double)dist2 < (double)th * (double)th (exact on both sides: the
 * reference's strict '<').  Means and shares are formed in double over the KEPT rows (gt_keep / rec_keep as in dqo_nn1) and rounded once to
 * float; the sums are added in a fixed order (see dqo_eval_picture): a row is bitwise reproducible.
 * out_table + 32 * row receives 32 floats: 0 accuracy, 1 completion, 2 chamfer, 3 n_thres, then for threshold t: 4 + 3 t precision P,
 *   5 + 3 t recall R, 6 + 3 t F1 (NaN when P + R = 0, as numpy's division); every other slot NaN.  An empty kept set on either side: 32 NaN.
 * thres_host: n_thres <= 8 floats in HOST memory, read before the call returns.  Both sets arrive as points: the ground-truth sampling of eval.py:247 is
 *   dqo_mesh_sample, the random subsampling of :244 is part of dqo_surfel_densify.
 * workspace: dqo_eval_pcd_workspace_bytes(n_gt, n_rec) bytes (0 for a bad size), ZERO when first used and then left to this call, which
 *   hands it back ready for the next one (capturable in a hipGraph).  Calls that share a workspace must be ordered (one stream). */
size_t dqo_eval_pcd_workspace_bytes(int32_t n_gt, int32_t n_rec);
int dqo_eval_pcd(int32_t n_gt, const float* gt_xyz, const uint8_t* gt_keep, int32_t n_rec, const float* rec_xyz, const uint8_t* rec_keep,
                 const float* rec_xform, int32_t n_thres, const float* thres_host, float* out_table, int32_t row, void* workspace,
                 size_t workspace_bytes, void* hipStream);

/* dqo_eval_pcd_grouped (ABI 5, symbols-only addition) — the per-object geometry numbers of metric_obj.py:169-236: for every object id its
 * stable cloud is evaluated against that object's own ground truth with eval_pcd(..., dist_threshs=[0.01], sample_nums=1000000).  Two
 * dqo_nn1_grouped searches (rec -> gt under rec_xform, gt -> rec) and one reduction launch write a [64,32] table: row first_row + g of
 * out_table is dqo_eval_pcd's row for object g — the same arithmetic per row (sqrt((double)dist2), (double)dist2 < (double)th * (double)th,
 * means and shares in double over the object's rows, rounded once; slot 3 = n_thres, unused slots NaN, P + R = 0 gives NaN).  An object
 * without a row on either side gets 32 NaN.  All 64 rows are written by every call, no row outside [first_row, first_row + 64) is
 * touched (table_rows: the rows out_table holds).  gt_group / rec_group: dqo_nn1_grouped's ids, any value outside [0, 64) = no object.
 * Bitwise reproducible: no float or double atomic; every double sum is added in an order fixed by the search's sorted order of the rows
 * (csrc/map_eval.hip states it).  thres_host and the workspace contract are dqo_eval_pcd's: ZERO when first used, handed back ready. */
size_t dqo_eval_pcd_grouped_workspace_bytes(int32_t n_gt, int32_t n_rec);
int dqo_eval_pcd_grouped(int32_t n_gt, const float* gt_xyz, const int32_t* gt_group, int32_t n_rec, const float* rec_xyz,
                         const int32_t* rec_group, const float* rec_xform, int32_t n_thres, const float* thres_host, float* out_table,
                         int64_t table_rows, int64_t first_row, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_nearest (ABI 5, symbols-only addition) — the nearest FACE of a mesh for every query point and the exact point-to-triangle
 * distance to it: what dqo_nn1 is for two point sets, for a point set against a surface.  This text is the specification;
 * tests/mesh_dist_oracle.py restates it one rounding at a time.
 * ARITHMETIC.  All of the rule is in float32.  Every operation is rounded once, evaluated left to right and never contracted; division
 *   is correctly rounded.  A dot product u.v is (ux*vx + uy*vy) + uz*vz.  A cross product has one rounding per product and per
 *   difference: (u x v).x = uy*vz - uz*vy, .y = uz*vx - ux*vz, .z = ux*vy - uy*vx.
 * VALID FACE.  A face is valid when (1) its row lies below the face count — counts[1] clamped to [0, cap_faces]; counts == NULL: the
 *   capacity is the count —, (2) its three indices lie in [0, vertex count) (counts[0], clamped alike) and (3) with ab = b - a,
 *   ac = c - a and n = ab x ac, the dot product n.n is finite and > 0.  A face below the count that fails (2) is counted in
 *   faces_bad_index, any other invalid face below the count in faces_degenerate (a zero-area face holds no surface; dqo_mesh_sample
 *   never draws from one either; a NaN or infinite corner fails (3)).  Invalid faces are never found.
 * E(p, f): the squared distance from p to the closest point x of triangle (a, b, c), by the seven-region walk of Ericson, Real-Time
 *   Collision Detection, 5.1.5, in this order and with these expressions:
 *     ap = p - a, d1 = ab.ap, d2 = ac.ap;  if d1 <= 0 && d2 <= 0:  x = a                                        (region 0)
 *     bp = p - b, d3 = ab.bp, d4 = ac.bp;  if d3 >= 0 && d4 <= d3: x = b                                        (region 1)
 *     vc = d1*d4 - d3*d2;  if vc <= 0 && d1 >= 0 && d3 <= 0:  v = d1 / (d1 - d3), x = a + v*ab                  (region 2)
 *     cp = p - c, d5 = ab.cp, d6 = ac.cp;  if d6 >= 0 && d5 <= d6: x = c                                        (region 3)
 *     vb = d5*d2 - d1*d6;  if vb <= 0 && d2 >= 0 && d6 <= 0:  w = d2 / (d2 - d6), x = a + w*ac                  (region 4)
 *     va = d3*d6 - d5*d4, e = d4 - d3, g = d5 - d6;  if va <= 0 && e >= 0 && g >= 0:  w = e / (e + g), x = b + w*(c - b)   (region 5)
 *     otherwise  den = 1 / ((va + vb) + vc), v = vb*den, w = vc*den, x = (a + ab*v) + ac*w                      (region 6)
 *     E = (p - x).(p - x);  if E is not finite (a 0 / 0 in a sliver's edge branch): E = ap.ap and x = a — the face stands for its corner a.
 * D(p, f) = fmaxf(E(p, f), B(p, aabb(f))): aabb(f) is the min / max of the three corners per axis, and B the squared box distance:
 *     per axis t: dt = 0 if lo_t <= p_t <= hi_t, else fminf(fabsf(p_t - lo_t), fabsf(p_t - hi_t));  B = (dx*dx + dy*dy) + dz*dz.
 *   In real arithmetic B <= the squared distance, so the clamp only ever raises E by E's own rounding error (whose size relative to d^2
 *   is unbounded as d -> 0); it is what makes the search's box pruning exact in float (csrc/knn.hip gives the argument).
 * RESULT.  dist2[i] = the minimum of D(p_i, f) over the valid faces f, bit for bit: a pure function of the inputs, whatever the order
 *   the search visits the faces in.  face[i] (may be NULL) is a valid face attaining it — which one of several is arbitrary, a point
 *   over a shared edge has two.  closest (may be NULL; float [Q,3]) receives E's x for that face, recomputed once after the search.
 *   A query whose keep byte is 0, and every query when the mesh has no valid face, gets FLT_MAX / -1 and its closest row is NOT written.
 * query_xyz [Q,3], query_keep (NULL: every row) and query_xform / mesh_xform (NULL: identity) are dqo_nn1's: 12 floats, a row-major 3x4
 *   transform, per output row ((m0 * x + m1 * y) + m2 * z) + m3; mesh_xform is applied to each vertex as it is loaded.
 * The mesh is the mesh operand of dqo_mesh_components: vertices [cap_vertices,3], faces int32 [cap_faces,3], counts a DEVICE pointer to
 *   two int32 (vertices, faces) or NULL; rows behind the counts are never read, so the header of dqo_tsdf_extract, dqo_mesh_components,
 *   dqo_mesh_simplify or dqo_mesh_cull goes in as counts.
 * header: int32 [8] on the device, cleared by the first launch (it must not be `counts`): 0 faces below the count, 1 valid faces,
 *   2 faces_bad_index, 3 faces_degenerate, 4 live queries (keep byte not 0), 5..7 zero.
 * Sizes: Q and cap_faces in [1, 2^25 - 1] (the index bits of a sorted row), cap_vertices in [1, 2^28); the size query returns 0 outside.
 * DQO_ERR_INVALID_ARG / DQO_ERR_WORKSPACE come back before anything is launched.  No allocation, no synchronisation, nothing read
 * back, no float atomic; the workspace needs no initialisation; capturable in a hipGraph. */
size_t dqo_mesh_nearest_workspace_bytes(int32_t Q, int32_t cap_vertices, int32_t cap_faces);
int dqo_mesh_nearest(int32_t Q, const float* query_xyz, const uint8_t* query_keep, const float* query_xform, const float* vertices,
                     const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces, const float* mesh_xform,
                     float* dist2, int32_t* face, float* closest, int32_t* header, void* workspace, size_t workspace_bytes,
                     void* hipStream);

/* dqo_eval_pcd_surface (ABI 5, symbols-only addition) — dqo_eval_pcd's [32] row (the same slots, the same reduction launch, the same
 * arithmetic per row) with the distances taken to the other side's SURFACE wherever that side has a mesh:
 *   with a ground-truth mesh, a reconstructed point's dist2 is dqo_mesh_nearest's from that point (under rec_xform) to the gt mesh
 *     (accuracy, precision); with a rec mesh, a ground-truth point's dist2 is dqo_mesh_nearest's to the rec mesh with its vertices under
 *     rec_xform (completion, recall).  A side without a mesh — capacities 0, 0 and NULL buffers — keeps its dqo_nn1 search against the
 *     other side's points, so a point-cloud reconstruction against a ground-truth mesh is exact in the one direction a surface exists.
 *   The points of both sides are always given (a mesh's own samples: dqo_mesh_sample_counted); a mesh operand is dqo_mesh_nearest's.
 *   A side whose mesh has no valid face makes the other side's column FLT_MAX: the row then holds 100 * sqrt(FLT_MAX) (about 1.8447e21)
 *     as that accuracy / completion, sqrt(FLT_MAX) in the chamfer sum, 0 as that P / R and with it 0 as F1 (NaN when the other share
 *     is 0 too) — not a row of NaN, which stays the mark of a side without a kept POINT.
 * Row limits, thres_host, out_table / row and the workspace contract are dqo_eval_pcd's: dqo_eval_pcd_surface_workspace_bytes (0 for a
 * bad size or capacity) bytes, ZERO when first used and then left to this call, which hands it back ready (capturable in a hipGraph). */
size_t dqo_eval_pcd_surface_workspace_bytes(int32_t n_gt, int32_t gt_cap_vertices, int32_t gt_cap_faces, int32_t n_rec,
                                            int32_t rec_cap_vertices, int32_t rec_cap_faces);
int dqo_eval_pcd_surface(int32_t n_gt, const float* gt_xyz, const uint8_t* gt_keep, const float* gt_vertices, const int32_t* gt_faces,
                         const int32_t* gt_counts, int32_t gt_cap_vertices, int32_t gt_cap_faces, int32_t n_rec, const float* rec_xyz,
                         const uint8_t* rec_keep, const float* rec_vertices, const int32_t* rec_faces, const int32_t* rec_counts,
                         int32_t rec_cap_vertices, int32_t rec_cap_faces, const float* rec_xform, int32_t n_thres, const float* thres_host,
                         float* out_table, int32_t row, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_surfel_densify (ABI 5, symbols-only addition) — the point set the reference evaluates its geometry on where a config sets
 * pcd_densify: GaussianPointCloud.densify(sigma, circle_num, levels) (SLAM/gaussian_pointcloud.py:67-130; slam.py:202-206 calls
 * densify(1, 30, 5)) followed by eval_pcd's subsample (SLAM/eval.py:244), in one step that never holds the densified cloud.
 * Row i (xyz [P,3], scaling_raw [P,3] log scales, rotation_raw [P,4] as r, x, y, z) becomes M = circle_num * levels * sigma virtual
 * points v = i * M + c, c = (b * levels + l) * circle_num + k (block b < sigma, level l < levels, angle k < circle_num):
 *     order        the three axes in ascending order of the RAW scales (exp is monotone); equal scales: the lower axis index first
 *                  (torch.argmin / argsort leave ties unspecified)
 *     n, p0, p1    columns order[0], order[1], order[2] of build_rotation(q / |q|) (utils/general_utils.py:108-131), each divided by
 *                  (its norm + 1e-8);  axis0 = exp(scaling_raw[order[1]]), axis1 = exp(scaling_raw[order[2]])
 *     a            (axis0 * sigma) * float((l + 0.5) / levels), plus axis0 * b in blocks b >= 1;  b_ the same with axis1
 *     x, z         a * cos(theta_k),  b_ * sin(theta_k)          circle_cs: 2 * circle_num floats on the device, the cosines then the sines
 *     frame 0      DQO_DENSIFY_FRAME_REFERENCE: out = mean + (p0.x x + p0.z z,  n.x x + n.z z,  p1.x x + p1.z z) — what the reference
 *                  writes to pcd_densify.ply: its matmul has p0, n, p1 as the ROWS of the matrix (:107-121)
 *     frame 1      DQO_DENSIFY_FRAME_SURFEL: out = mean + x p0 + z p1, points in the surfel's plane (the evident intent)
 *     normal       n, for every point of the row (:122)
 * every float statement rounded once, none contracted (csrc/map_densify.hip lists them in order).
 * row_keep: NULL = every row; else one byte per row, 0 = the row gives no point.  N = M * (kept rows).
 * Subsample (replaces the host's np.random.choice, same distribution): virtual point v of a kept row gets
 *   key = hash32(seed, draw 3, v) (csrc/dqo_sample_hash.h, all 32 bits; draws 0-2 are dqo_growth_sample's); the n = min(N, cap) smallest
 *   keys are chosen — keys of different v never tie — and the chosen points come out in ascending v.  A radix select, never a sort.
 * points [cap,3], normals [cap,3] (may be NULL), index [cap] int64 (may be NULL): v of each emitted point (its surfel: v / M); rows at
 *   and behind n are NOT written.  keep [cap] uint8, written for ALL cap rows: 1 for the first n, 0 behind — dqo_nn1 / dqo_eval_pcd take
 *   it as rec_keep, so no count is ever read back.
 * header (8 x int32, overwritten): 0 kept rows, 1 / 2 N's low / high word, 3 n, 4 M, 5 the threshold key (the n-th smallest key; -1, all
 *   bits set, when n == N: nothing was rejected), 6 frame, 7 zero.
 * DQO_ERR_INVALID_ARG before anything is launched: a NULL required pointer, P < 1, circle_num, levels or sigma < 1, circle_num > 1024,
 *   M > 65535, P * M >= 2^32, cap < 1, an unknown frame.  DQO_ERR_WORKSPACE: the workspace is too small.
 * workspace: dqo_surfel_densify_workspace_bytes(P, circle_num, levels, sigma) bytes (0 for a bad size), ANY contents: its head is zeroed
 *   by the call's first launch (dqo_growth_sample's contract).  No allocation, no synchronisation, nothing read back, integer atomics
 *   only: the output is a pure function of the arguments.  Calls that share a workspace must be ordered (one stream). */
#define DQO_DENSIFY_FRAME_REFERENCE 0
#define DQO_DENSIFY_FRAME_SURFEL 1
size_t dqo_surfel_densify_workspace_bytes(int32_t P, int32_t circle_num, int32_t levels, int32_t sigma);
int dqo_surfel_densify(int32_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const uint8_t* row_keep,
                       int32_t circle_num, int32_t levels, int32_t sigma, const float* circle_cs, int32_t frame, uint64_t seed, int64_t cap,
                       float* points, float* normals, int64_t* index, uint8_t* keep, int32_t* header, void* workspace,
                       size_t workspace_bytes, void* hipStream);

/* dqo_mesh_sample (ABI 5, symbols-only addition) — the ground truth's point set of eval_pcd: trimesh.sample.sample_surface(mesh_gt,
 * sample_nums) (SLAM/eval.py:247) from the mesh's vertices [V,3] float32 and triangles [F,3] int32, nothing read back.  trimesh's four
 * steps (face areas, their cumulative sum, one uniform draw located in it, two uniform draws folded back into the triangle), with two
 * departures that make the result a pure function of the arguments: the draws are the key rule of csrc/dqo_sample_hash.h (draws 4-7)
 * instead of numpy's stream, and the cumulative table counts integer quanta of area, so no float sum's order can reach it.
 * One rounding per statement, none contracted (tests/mesh_oracle.py restates them):
 *     area     a face with an index outside [0, V) has A = 0; its vertices are never loaded.  Otherwise, in double: e1 = b - a, e2 = c - a,
 *              c = e1 x e2 with each component as p * q - r * s, A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz); a non-finite A becomes 0
 *     quanta   amax = max A;  frexp(amax) = (m, x) (x = 0 when amax = 0);  e = 61 - bit_length(F) - x;
 *              q_f = (uint64) floor(ldexp(A_f, e)) < 2^(61 - bit_length(F)), so the total is below 2^61; the largest face has >= 2^35 quanta
 *     table    cum[f] = q_0 + ... + q_f in uint64, total = cum[F - 1]
 *     draw     sample i: k_d = dqo_sample_key(seed_word, dqo_sample_draw_word(seed_word, 4 + d), i, 0xffffffff), d = 0..3;
 *              t = floor(total * (k0 * 2^32 + k1) / 2^64); the face is the first f with cum[f] > t (a face without quanta is never picked);
 *              u = k2 * 2^-32, v = k3 * 2^-32 in double; if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
 *              p = a + ((b - a) * u + (c - a) * v) per component in double, rounded once to float
 * points [count,3]; face_index [count] int32 (may be NULL); keep [count] uint8, written for ALL rows: 1, or all 0 when the mesh has no area
 *   (then no point is written) — dqo_nn1 / dqo_eval_pcd take it as gt_keep, so no count is ever read back.
 * header (8 x int32, overwritten): 0 n written (count, or 0 when the mesh has no area), 1 F, 2 faces with an index outside [0, V), 3 faces
 *   of zero or non-finite area among those whose indices are in range, 4 the quantum exponent e, 5 / 6 the total's low / high word, 7 zero.
 * DQO_ERR_INVALID_ARG before anything is launched: a NULL required pointer, V < 1, F or count outside [1, 2^25 - 1] (dqo_nn1's row limit).
 *   DQO_ERR_WORKSPACE: the workspace is NULL or too small.
 * workspace: dqo_mesh_sample_workspace_bytes(F, count) bytes (0 for a bad size), ZERO when first used and then left to this call, which
 *   hands it back ready for the next one (capturable in a hipGraph): ticket words, the blocks' partials (a block owns
 *   DQO_MESH_SCAN_BLOCK faces) and, last, cum.  Four launches; no allocation, no synchronisation, integer atomics only.  Calls that share
 *   a workspace must be ordered (one stream). */
#define DQO_MESH_SCAN_BLOCK 1024
size_t dqo_mesh_sample_workspace_bytes(int32_t F, int32_t count);
int dqo_mesh_sample(int32_t V, const float* vertices, int32_t F, const int32_t* faces, int32_t count, uint64_t seed, float* points,
                    int32_t* face_index, uint8_t* keep, int32_t* header, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_sample_counted (ABI 5, symbols-only addition) — dqo_mesh_sample on a mesh operand (dqo_mesh_components', below): vertices
 * float32 [cap_vertices,3], faces int32 [cap_faces,3] and counts, a device pointer to two int32 (V, F; each clamped to [0, capacity];
 * NULL: the capacities are the counts) — the header of dqo_tsdf_extract, dqo_mesh_components, dqo_mesh_simplify or dqo_mesh_cull fits
 * directly, so the mesh this library makes is sampled without its counts leaving the device.  The same statements (area, quanta, table,
 * draw) in the same four launches; bit_length(F) and the exponent e are formed on the device from the count; the workspace,
 * dqo_mesh_sample_counted_workspace_bytes(cap_faces, count), and the grids are sized from cap_faces and count.
 * For every counts, every output byte — points, face_index, keep, header words 0-6 — equals dqo_mesh_sample of the sliced mesh
 * (vertices[:V], faces[:F]).  F == 0, or no area: keep all 0, no point written, header[0] = 0 (the table is never searched).  Rows behind
 * the counts are never read.  DQO_ERR_INVALID_ARG before anything is launched: a NULL required pointer, cap_vertices outside [1, 2^28),
 * cap_faces or count outside [1, 2^25 - 1], a header that is the counts; then DQO_ERR_WORKSPACE. */
size_t dqo_mesh_sample_counted_workspace_bytes(int32_t cap_faces, int32_t count);
int dqo_mesh_sample_counted(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                            int32_t count, uint64_t seed, float* points, int32_t* face_index, uint8_t* keep, int32_t* header, void* workspace,
                            size_t workspace_bytes, void* hipStream);

/* Batched dual-quadric residual over B independent (object, view) pairs: loss = 1 - IoU(obs, bbox(ellipsoid, P34)),
 * with gradients.  valid[b] = 0 when loss == 1 (the reference skips that Adam step). */
int dqo_quadric_iou_fwd_bwd(int32_t B, const float* axes, const float* R, const float* center, const float* P34,
                            const float* obs_bbox, float* bbox, float* loss, int32_t* valid, float* g_axes, float* g_R,
                            float* g_center, void* hipStream);
/* Object_Optimize_only inner loops for n_obj objects in ONE launch: n_iters Adam steps each (lr .01/.001/.01,
 * betas .9/.999, eps 1e-15), view picked by view_schedule[obj][it] (negative = from the end).  Parameters are updated
 * in place; loss_hist [n_obj, n_iters] may be NULL.  Views of object o are P34_views / obs_views rows
 * [view_offset[o], view_offset[o+1]). */
int dqo_quadric_adam(int32_t n_obj, int32_t n_iters, const int32_t* view_offset, const float* P34_views,
                     const float* obs_views, const int32_t* view_schedule, float* axes, float* R, float* center,
                     float* loss_hist, void* hipStream);

/* dqo_objmap_frame / dqo_objmap_optimize / dqo_objmap_mean_iou (ABI 5, symbols-only addition) — the object stage of a mapping frame on a
 * device-resident object table, nothing read back: what SLAM/multiprocess/mapper.py:147-165 runs for a frame with detections
 * (detections_filter quadrics.py:336-386, ObjectsInitialization / Object.__init__ :429-538, Occlusions_Check :926-968, the live MatchObject
 * (Only_IOU) :1013-1217, remove_outlier :2397-2425), Object_Optimize_only as mapper.py:204-205 calls it (quadrics.py:2234-2298) and record_iou
 * (mapper.py:1512-1531).  The reference does this in numpy on the host, with 30 single-pixel reads of the device depth map per detection.
 * tests/object_oracle.py restates every statement; arithmetic is double from the float32 table, the depth statistics float32 in sample order.
 *
 * The table (caller-owned, zero before the first frame; 1 <= cap_obj <= 1024, cap_views >= 2):
 *   obj_axes [cap_obj,3], obj_R [cap_obj,9] (row-major), obj_center [cap_obj,3] float32 — the layout dqo_quadric_adam updates in place;
 *   obj_cat, obj_uid (the reference's Object.id_), obj_nviews [cap_obj] int32;
 *   view_P34 [cap_obj,cap_views,12], view_bbox [cap_obj,cap_views,4] float32: K @ Rt and the detection bbox of each stored observation, in
 *   append order;  state [3] int32: the object count, the next uid, whether the first-frame branch (Map_global is None) has been taken.
 *
 * dqo_objmap_frame: ONE launch of ONE workgroup on the caller's stream, no allocation.  1 <= M <= cap_det <= 64.
 *   in   det_bbox [M,4], det_ellipse [M,5] (centre, full axes, angle: the json's order, quadrics.py:262), det_cat [M] int32, det_score [M];
 *        depth [H,W]; K [9]; Rt [12] (3x4, world to camera); W, H, frame_id, seed.
 *        The 30 depth samples of a detection come from the key rule of csrc/dqo_sample_hash.h (dqo_object_key, draws 8 and 9) instead of
 *        random.randint: a pure function of (seed, frame_id, the detection's index in the input, the sample).
 *   out  det_fate [M] int32: 0 dropped by the filter, 1 invalidated (covered by a stored object of its category), 2 matched, 3 new object,
 *        4 replaced an object (covering replacement), 5 unmatched and too shallow (no object: the mean depth is not in (0.01, 15); the
 *        first frame: (0, 15));  det_row [M] int32: the detection's row AFTER remove_outlier's compaction, -1 without one (also when
 *        its object was removed, or dropped for lack of room);  det_depth [M,2] float32: min(mean, 5) and clamp(max - min, 0.05, 0.2) of
 *        the positive samples, (0, 0) without one;
 *        opt_flag [cap_obj] uint8: rows a validated detection of this frame holds and that store at least two observations — the gate of
 *        quadrics.py:2246-2249;
 *        frame_header [8] int32: accepted, matched, new, replaced, removed (by remove_outlier), has_new_object, overflow_obj, overflow_views.
 *   Two departures from the reference: (1) the table has no orphans: after a covering replacement the frame's visible list keeps the
 *   stale projection and category, as the reference's dictionary does, but a later detection matched through that entry is matched to
 *   the ROW (its observation goes to the row in the reference too); (2) det_row is the row after compaction, where the reference
 *   leaves a stale index in det["node_id"].
 *   Capacity: a full table is never written past — the object (overflow_obj) or observation (overflow_views) is dropped and counted;
 *   an object that is dropped consumes no uid.
 * dqo_objmap_optimize: Object_Optimize_only for every row with opt_flag set, one lane per row, reading the row's observation slots in
 *   place: 20 Adam steps with dqo_quadric_adam's learning rates and constants (bit for bit that launch on the gathered views); the view
 *   of step `it` is dqo_object_key(draw 10, frame_id, uid * 32 + it) modulo the row's count for it <= 5, the last observation afterwards
 *   (quadrics.py:2264-2266).  loss_hist [cap_obj,20] may be NULL.
 * dqo_objmap_mean_iou: mean_iou [cap_obj] float32: each row's mean IoU of its projected bbox with its stored observations over those
 *   with IoU > 0, 0 with none or past the object count.  One lane per row, in double.
 * DQO_ERR_INVALID_ARG before anything is launched: a NULL pointer (loss_hist excepted), capacities out of range, M outside
 *   [1, cap_det], a bad image size. */
int dqo_objmap_frame(int32_t cap_obj, int32_t cap_views, int32_t cap_det, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_cat,
                     int32_t* obj_uid, int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state, int32_t M,
                     const float* det_bbox, const float* det_ellipse, const int32_t* det_cat, const float* det_score, const float* depth,
                     const float* K, const float* Rt, int32_t W, int32_t H, int32_t frame_id, uint64_t seed, int32_t* det_fate,
                     int32_t* det_row, float* det_depth, uint8_t* opt_flag, int32_t* frame_header, void* hipStream);
int dqo_objmap_optimize(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_uid,
                        int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state, const uint8_t* opt_flag, int32_t frame_id,
                        uint64_t seed, float* loss_hist, void* hipStream);
int dqo_objmap_mean_iou(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_nviews,
                        float* view_P34, float* view_bbox, int32_t* state, float* mean_iou, void* hipStream);

/* ---- fused helpers around the rasteriser for one mapping iteration (optional) ------------------
 * They replace eager torch op sequences of the reference's callers, not a CUDA binding:
 *   dqo_map_activate      <- SLAM/gaussian_pointcloud.py:732-733, 746-747 (sigmoid / exp / F.normalize)
 *   dqo_map_loss_fwd_bwd  <- SLAM/multiprocess/mapper.py:836-875 with a render mask (masked L1 colour + masked depth L1; SSIM
 *                            is skipped in that case, B14) and its autograd backward
 *   dqo_map_ssim_fwd_bwd  <- SLAM/multiprocess/mapper.py:839-845 without a render mask: the SSIM term (utils/loss_utils.py:41-100)
 *   dqo_map_adam_step     <- autograd through the activations + torch.optim.Adam(eps=1e-15) over the six parameter groups
 *                            (SLAM/gaussian_pointcloud.py:331-378, mapper.py:548) */
int dqo_map_activate(int32_t P, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, float* opacity,
                     float* scales, float* rotations, void* hipStream);

size_t dqo_map_loss_workspace_bytes(void);
/* color [3,H,W], depth [1,H,W], depth_index int32 [1,H,W] (the op's hit_depth), render_mask uint8 [H,W] or NULL (= all).
 * loss_out[8] = {total, colour, depth, 0, sum |colour error| over the mask, mask pixels, sum |depth error| over the valid depth
 * pixels, valid depth pixels} — the four sums are what object shards of one map add up (one packed all-reduce) to report the loss
 * over all objects; writes dL_dcolor [3,H,W] and dL_ddepth [1,H,W] of `total`. */
int dqo_map_loss_fwd_bwd(int32_t W, int32_t H, const float* color, const float* depth, const int32_t* depth_index,
                         const float* gt_color, const float* gt_depth, const uint8_t* render_mask, float color_weight,
                         float depth_weight, float add_depth_thres, float* loss_out, float* dL_dcolor, float* dL_ddepth,
                         void* workspace, size_t workspace_bytes, void* hipStream);

/* The SSIM term of Mapping.loss_update's unmasked branch (SLAM/multiprocess/mapper.py:839-845: loss += 0.2 * (1 - ssim(image, gt)),
 * ssim = utils/loss_utils.py:41-100: 11 x 11 Gaussian window, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over all
 * channels and pixels) with its gradient, in three launches in place of the five conv2d calls, ~25 elementwise ops and their autograd
 * backward.  image, gt_image [3,H,W]; ssim_out[2] = {ssim, weight * (1 - ssim)}; dL_dimage [3,H,W] (may be NULL: value only) receives
 * d(weight * (1 - ssim)) / d image — written when accumulate == 0, added onto what it holds otherwise (e.g. onto the L1 gradient
 * image dqo_map_loss_fwd_bwd wrote).  loss_out8 (may be NULL) = the loss_out of a dqo_map_loss_fwd_bwd call issued before on the same
 * stream: its total [0] grows by the term and slot [3] receives 1 - ssim, so the eight floats read like Mapping.loss_update's report.
 * The sum over pixels is formed per 16 x 16 tile and then over tiles in a fixed order: reproducible. */
size_t dqo_map_ssim_workspace_bytes(int32_t W, int32_t H);
int dqo_map_ssim_fwd_bwd(int32_t W, int32_t H, const float* image, const float* gt_image, float weight, float* ssim_out,
                         float* dL_dimage, int32_t accumulate, float* loss_out8, void* workspace, size_t workspace_bytes,
                         void* hipStream);

/* The attach loss of Mapping.loss_update (SLAM/multiprocess/mapper.py:812-829) with its gradient, for callers that keep their own
 * optimiser (ABI 3):  loss[0] = 1000 * (mse(scaling[a], scaling0[a]) + mse(xyz[a], xyz0[a]) + mse(rotation[a], rotation0[a])),  a =
 * attach_mask != 0 with |a| = attach_count (0: loss and gradients are zero), on the RAW parameters; g_* ([P,3], [P,3], [P,4]) are fully
 * written (zeros outside a).  Two launches in place of the ~12 eager torch ops of the forward and the ~25 of their autograd backward. */
size_t dqo_map_attach_workspace_bytes(int32_t P);
int dqo_map_attach_loss_fwd_bwd(int32_t P, const float* scaling_raw, const float* xyz, const float* rotation_raw,
                                const float* init_scaling_raw, const float* init_xyz, const float* init_rotation_raw,
                                const uint8_t* attach_mask, int32_t attach_count, float* loss, float* g_scaling_raw, float* g_xyz,
                                float* g_rotation_raw, void* workspace, size_t workspace_bytes, void* hipStream);

/* torch.optim.Adam's step (weight_decay = 0, amsgrad = False, maximize = False) over up to DQO_ADAM_MULTI_MAX dense fp32 tensors in
 * ONE launch, for callers that keep the reference's parameter tensors and autograd (ABI 3): per tensor p, its gradient g (w.r.t. p
 * itself — no activation Jacobian is applied here, unlike dqo_map_adam_step), exp_avg m, exp_avg_sq v, element count n and the
 * group's learning rate; `step` is the 1-based step count of THIS update, common to the tensors of the call (gaussian_pointcloud.py:
 * 331-378 builds ONE Adam over six groups with eps = 1e-15, so they share it).  The element update is the library's adam1 — the
 * statement order of torch's single- / multi-tensor paths; betas and eps arrive as doubles and 1 - beta, beta^t, lr / (1 - beta1^t) are
 * formed in double and rounded once, as torch forms them from python floats.  In place
 * of torch.optim.Adam.step()'s per-group launches (and their host time: six groups = 0.28 ms per iteration on the drop-in path). */
#define DQO_ADAM_MULTI_MAX 16
typedef struct DqoAdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    double lr;  /* the group's learning rate as the python float it is: lr / (1 - beta1^t) is formed in double and rounded once, as torch does */
} DqoAdamTensor;
int dqo_adam_multi(const DqoAdamTensor* tensors, int32_t n_tensors, int32_t step, double beta1, double beta2, double eps, void* hipStream);
/* The same with the step count on the device, for a step that is captured into a hipGraph (a replay must take the count of ITS step,
 * not the capture's): step_dev[0] = steps taken so far; the launch applies step step_dev[0] + 1 — its bias corrections are formed by the
 * kernel with the host path's double-precision expressions (torch's capturable Adam forms them in float) — and, with advance != 0, a
 * one-thread launch behind it stores the new count (advance = 0 on all but the last call when one step takes several calls). */
int dqo_adam_multi_dev(const DqoAdamTensor* tensors, int32_t n_tensors, int32_t* step_dev, int32_t advance, double beta1, double beta2,
                       double eps, void* hipStream);

/* dqo_accumulate_gaussian_error <- cuda_utils._C.accumulate_gaussian_error (submodules/cuda_utils/ext.cpp, cuda_utils.cu:17-62,
 * map_process.cu:33-245; caller SLAM/multiprocess/mapper.py:1034-1047).  Maps are [H*W]; outputs [P] are fully written
 * (zero-initialised inside).  check_max != 0: per-Gaussian maximum of the errors (the mode DQO-MAP uses); 0: mean, which needs
 * `counters` (int32 [2*P] scratch).  rescale_counter counts pixels whose error exceeds the thresholds. */
int dqo_accumulate_gaussian_error(int32_t H, int32_t W, int32_t P, const float* screen_color_error, const float* screen_depth_error,
                                  const float* screen_normal_error, const int32_t* screen_color_index,
                                  const int32_t* screen_depth_index, float color_threshold, float depth_threshold,
                                  float normal_threshold, int32_t check_max, float* gs_color_error, float* gs_depth_error,
                                  float* gs_normal_error, float* gs_rescale_counter, int32_t* counters, void* hipStream);

/* dqo_accumulate_gaussian_confidence <- cuda_utils._C.accumulate_gaussian_confidence (submodules/cuda_utils/ext.cpp:7,
 * cuda_utils.cu:62-83, map_process.cu:247-360; exported by the reference's extension, no Python caller in the reference).  Maps are
 * [H*W]; per Gaussian named by gaussian_index_map (entries outside [0, P) are skipped): maximum, minimum and mean of the confidence
 * over its pixels, 0 / 0 / 0 for a Gaussian no pixel names.  Outputs [P] fully written; `counter` is int32 [P] scratch. */
int dqo_accumulate_gaussian_confidence(int32_t H, int32_t W, int32_t P, const int32_t* gaussian_index_map,
                                       const float* gaussian_confidence_map, float* gs_confidence_max, float* gs_confidence_min,
                                       float* gs_confidence_mean, int32_t* counter, void* hipStream);

/* Row f3 — tile-mask producers of the mapping loop (SLAM/utils.py:720-799, SLAM/multiprocess/mapper.py:930-988), 16x16 tiles
 * with the reference's zero padding (a tile is always divided by 256).  All pointers are device pointers.
 *   dqo_tile_count_mask:   tile_count[t] = number of non-zero pixels of a uint8 pixel mask in tile t
 *                          (pixelmask2tilemask = count > 0; transmission2tilemask = count / 256 > ratio)
 *   dqo_transmission_mask: render_mask = (T_map != 1) (written if non-NULL), tile_count as above, *total = its pixel count
 *                          (evaluate_render_range: render_mask, tile_mask, render_ratio in one pass)
 *   dqo_tile_color_error:  color_error = sum_c |render - gt|, zeroed where the rendered colour sums to 0 (written if
 *                          non-NULL); tile_sum[t] = its sum over tile t (meanpool / colorerror2tilemask = tile_sum / 256) */
int dqo_tile_count_mask(int32_t W, int32_t H, const uint8_t* pixel_mask, int32_t* tile_count, void* hipStream);
int dqo_transmission_mask(int32_t W, int32_t H, const float* T_map, uint8_t* render_mask, int32_t* tile_count, int32_t* total,
                          void* hipStream);
int dqo_tile_color_error(int32_t W, int32_t H, const float* render, const float* gt, float* color_error, float* tile_sum,
                         void* hipStream);

/* dqo_window_masks (ABI 5, symbols-only addition) — Mapping.evaluate_render_range (SLAM/multiprocess/mapper.py:930-988) for one frame
 * of a mapping call's window, written in place.  T_map: [H*W]; render, gt: [3, H*W] planes; gy = ceil(H/16), gx = ceil(W/16).
 *   mode 0 (local, :983-985)  render_mask = T_map != 1;  tile_mask = float(count) / 256.f > tile_mask_ratio, count over the tile's in-image
 *                             pixels (transmission2tilemask, SLAM/utils.py:752-762)
 *   mode 1 (error, :947-978)  tile_mask = 1 on the k tiles with the largest colour error sum (dqo_tile_color_error's expression and
 *                             order; k = int(gy * gx * sample_ratio), SLAM/utils.py:787);  render_mask = the tile mask over its 16 x 16
 *                             pixels, cropped.  T_map is not read.
 *   mode 2 (final, :980-982)  render_mask = T_map != 1;  tile_mask = 1 everywhere (the reference's None)
 * render_mask uint8 [H*W], tile_mask int32 [gy*gx], ratio_out[0] = float32(pixels of render_mask) / float32(H * W) (:987).
 * Mode 1's selection: the k largest by (sum descending, tile index ascending); a sum is compared by its float32 bit pattern as an unsigned
 *   integer (the sums are non-negative; a NaN lies above every number).  k = 0: all zero; k = gy * gx: all one.  Any tile count.
 * One launch (mode 1: two), no float atomic, no zero fill: the same bytes for the same inputs, and capturable in a hipGraph.
 * render_header (may be NULL): the device header of the forward that rendered the images.  header.overflow != 0 (invalid images):
 *   render_mask and tile_mask keep their bytes and ratio_out[0] = NaN.
 * workspace: dqo_window_masks_workspace_bytes(W, H) bytes (0 for a bad size), ZERO when first used and then left to this call, which hands
 *   it back ready for the next one.  After a mode 1 call its float32 words from byte DQO_WINDOW_MASKS_SUMS_OFFSET on are the gy * gx tile
 *   sums the selection ran on.  Calls that share a workspace must be ordered (one stream).
 * DQO_ERR_INVALID_ARG before anything is launched: a NULL output, a bad size or mode, modes 0 / 2 without T_map, mode 1 without render /
 *   gt or with k outside [0, gy * gx], a workspace that is NULL or too small. */
#define DQO_WINDOW_MASKS_SUMS_OFFSET 4352
size_t dqo_window_masks_workspace_bytes(int32_t W, int32_t H);
int dqo_window_masks(int32_t W, int32_t H, int32_t mode, const float* T_map, const float* render, const float* gt, float tile_mask_ratio,
                     int32_t k, uint8_t* render_mask, int32_t* tile_mask, float* ratio_out, const DqoRastHeader* render_header,
                     void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_map_pack_rows / dqo_map_unpack_rows (ABI 5, symbols-only addition) — the vertex table of a map checkpoint, built and taken apart on
 * the device.  They replace the host work of gaussian_map.save_model (SLAM/multiprocess/mapper.py:1571-1608: save_model_ply,
 * SLAM/gaussian_pointcloud.py:641-684, for each cloud, and merge_ply, SLAM/utils.py:414-423) and of pointcloud.load
 * (gaussian_pointcloud.py:132-207): boolean indexing of every buffer, seven device-to-host copies, the SH transpose, np.concatenate.
 * The map: P rows of xyz [P,3], shs [P,M,3] (coefficient 0 = f_dc), opacity_raw [P], scaling_raw [P,3], rotation_raw [P,4],
 *   confidence [P] (NULL = zeros), alive uint8 [P] (NULL = every row is a Gaussian), stable uint8 [P] (NULL = every row is unstable).
 * A table row, all float32, C = 6 + 3 M + 8 + (confidence ? 1 : 0) columns in the order of construct_list_of_attributes (:557-588):
 *   x y z | three zeros (the normals, :645) | f_dc_0..2 | f_rest channel-major, shs[:, 1:, :] as [3, M - 1] | opacity | scale_0..2 |
 *   rot_0..3 | confidence.  Values are copied as 32-bit words: NaN payloads, -0 and denormals keep their bits.
 * dqo_map_pack_rows: the alive rows with stable == 0 in ascending row index, then the alive rows with stable != 0 in ascending row
 *   index — the row order of the reference's merged file.  header (2 x int32, device, overwritten) = {U, S}: the first U table rows are the
 *   vertex data of path.ply, the last S those of path_stable.ply, all U + S those of path_merge.ply.  table must hold table_rows >= P rows
 *   (an overflow is impossible without a host read); rows at and behind U + S are NOT written.  Two launches, nothing read back, no float
 *   atomics, integer atomics only for the last-block ticket: the table is a pure function of the inputs.
 *   workspace: dqo_map_pack_workspace_bytes(P) bytes (0 for P < 1), ZERO when first used and then left to this call, which hands it back
 *   ready for the next one (capturable in a hipGraph).  Calls that share a workspace must be ordered (one stream).
 * dqo_map_unpack_rows: table rows [0, n) (has_confidence: with the column) into rows [first_row, first_row + n) of a map of P rows;
 *   a table without the column writes confidence as zero; confidence NULL: not written.  One launch.  n = 0: nothing is done.
 * Size limit: a table of P rows has at most 2^31 - 1 floats (P * C <= 2^31 - 1; the kernels index with 64 bits all the same), and
 *   1 <= M <= 64.
 * DQO_ERR_INVALID_ARG before anything is launched: P < 1, M outside [1, 64], P * C > 2^31 - 1, a NULL required pointer, table_rows < P,
 *   n < 0, first_row < 0, first_row + n > P.  DQO_ERR_WORKSPACE: the workspace is NULL or too small. */
size_t dqo_map_pack_workspace_bytes(int32_t P);
int dqo_map_pack_rows(int32_t P, int32_t M, int32_t include_confidence, const float* xyz, const float* shs, const float* opacity_raw,
                      const float* scaling_raw, const float* rotation_raw, const float* confidence, const uint8_t* alive,
                      const uint8_t* stable, float* table, int64_t table_rows, int32_t* header, void* workspace, size_t workspace_bytes,
                      void* hipStream);
int dqo_map_unpack_rows(int32_t P, int32_t M, int32_t n, int32_t first_row, int32_t has_confidence, const float* table, float* xyz,
                        float* shs, float* opacity_raw, float* scaling_raw, float* rotation_raw, float* confidence, void* hipStream);

/* dqo_map_pack_rows_by_object (ABI 5, symbols-only addition) — the vertex data of every file GaussianPointCloud.save_model_ply_obj writes
 * (SLAM/gaussian_pointcloud.py:589-637, called for both clouds from mapper.py:1586-1588; metric_obj.py loads the `_stable_obj{id}.ply`
 * ones), in ONE table.  It replaces, per cloud and per object, the boolean indexing of every buffer, seven device-to-host copies, the SH
 * transpose and np.concatenate of :606-634, and the np.unique of :592-593.
 * The map arguments, the row layout and the word-for-word copies are dqo_map_pack_rows'.  gaussian_object int32 [P]: an id in [0, 64) is
 *   the row's object, any other value means none.  The table's rows are the alive rows that have an object, ordered by (stable != 0,
 *   object id, row index), all ascending; header (int32 [2][64], device, overwritten): header[c][g] = the rows of cloud c (0 unstable, 1
 *   stable), object g.  The slice of (cloud 0, object g) is the vertex data of path + "_obj{g}.ply", that of (cloud 1, object g) of
 *   path + "_stable_obj{g}.ply"; an object without rows in a cloud has no file (:590-593).  table_rows >= P; rows at and behind the
 *   total are NOT written.  Three launches, nothing read back, no atomics: the table is a pure function of the inputs.
 *   workspace: dqo_map_pack_workspace_bytes(P) bytes, the same query — those bytes suffice: this call's order list lives in word 0 of the
 *   table rows it is about to fill, and the workspace is handed back as it came (the contract of dqo_map_pack_rows holds trivially).
 * DQO_ERR_INVALID_ARG / DQO_ERR_WORKSPACE as dqo_map_pack_rows, and for a NULL gaussian_object. */
int dqo_map_pack_rows_by_object(int32_t P, int32_t M, int32_t include_confidence, const float* xyz, const float* shs,
                                const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, const float* confidence,
                                const uint8_t* alive, const uint8_t* stable, const int32_t* gaussian_object, float* table, int64_t table_rows,
                                int32_t* header, void* workspace, size_t workspace_bytes, void* hipStream);

/* Row f4 — normal equations of one Gauss-Newton iteration of the point-to-plane ICP tracker (SLAM/icp.py:51-123:
 * compute_residuals_jacobian + compute_jtj + compute_jtr).  vertex / normal maps are [H, W, 3] fp32, pose10 a row-major 4x4
 * (maps frame-0 points into frame 1), normal_threshold the cosine.  Out: JtJ [6,6] (rotation block first), JtR [6],
 * valid_count [1] = pixels that passed every test.  The 6x6 solve / se(3) update stay with the caller. */
size_t dqo_icp_workspace_bytes(void);
int dqo_icp_normal_equations(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1,
                             const float* pose10, float fx, float fy, float cx, float cy, float distance_threshold,
                             float normal_threshold, float* JtJ, float* JtR, int32_t* valid_count, void* workspace,
                             size_t workspace_bytes, void* hipStream);

/* Row f4 — one Gauss-Newton iteration of ICP.icp on the device (SLAM/icp.py:33-47, 248-337): dqo_icp_normal_equations' pass, then
 * one block that folds its partials in the same order, forms lev_mar_H = JtJ + damping * trace(JtJ) * I in fp32, solves
 * xi = -H^-1 JtR in double (Cholesky; a cyclic-Jacobi pseudo-inverse with numpy.linalg.pinv's cutoff when H is not positive
 * definite, so H == 0 gives xi = 0) and updates pose10 <- exp_se3(xi) @ pose10 IN PLACE (exp in double, the product in fp32).
 * valid_count [1] gets the iteration's valid pixel count.  Two launches, no host copy: an ICP level of n iterations is n calls.
 * K: the intrinsics as a row-major 3x3 fp32 matrix in DEVICE memory, used as K * k_scale (fp32, icp.py:437-439), so a per-frame
 * GPU intrinsic needs no host read.  workspace: dqo_icp_workspace_bytes(). */
int dqo_icp_gauss_newton(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1,
                         float* pose10, const float* K, float k_scale, float distance_threshold, float normal_threshold, float damping,
                         int32_t* valid_count, void* workspace, size_t workspace_bytes, void* hipStream);

/* Tracker frame geometry (Tracker.map_preprocess, SLAM/multiprocess/tracker.py:135-156) of a metric depth map [H, W]:
 * optional bilateralFilter_torch(depth, 5, 2, 2) (depth_filter != 0), range mask min_depth < d < max_depth, compute_vertex_map,
 * compute_normal_map (Sobel, cross(dy, dx), zero where z <= min z or z >= max z over the whole map), compute_confidence_map,
 * invalid = (normal == 0).all() | confidence < invalid_confidence_thresh, and depth / vertex / normal / confidence zeroed there.
 * Out: depth_out [H, W], vertex_out / normal_out [H, W, 3], confidence_out [H, W], invalid_out [H, W] (0 / 1).  depth_out may
 * be `depth` itself (in place).  K: row-major 3x3 fp32 intrinsics in device memory, as for dqo_icp_gauss_newton.  Two launches. */
size_t dqo_track_preprocess_workspace_bytes(int32_t H, int32_t W);
int dqo_track_preprocess(int32_t H, int32_t W, const float* depth, const float* K, float min_depth, float max_depth,
                         float invalid_confidence_thresh, int32_t depth_filter, float* depth_out, float* vertex_out, float* normal_out,
                         float* confidence_out, uint8_t* invalid_out, void* workspace, size_t workspace_bytes, void* hipStream);

/* Vertex / normal pyramids of a depth map [H, W] (ImagePyramids("max") + build_vertex_pyramid + build_normal_pyramid, SLAM/icp.py:340-358,
 * SLAM/utils.py:542-558).  `levels` in [1, 4]; level i (coarsest first) max-pools by 2^(levels-1-i) with floor sizes
 * (H >> (levels-1-i), W >> ...), takes K * 2^-(levels-1-i) (K[2,2] = 1) for its vertex map and the normal rule of
 * dqo_track_preprocess per level.  vertex / normal hold the levels packed in that order: dqo_track_pyramid_pixels(H, W, levels)
 * rows of 3 floats each.  K: device intrinsics as for dqo_icp_gauss_newton.  Two launches. */
int64_t dqo_track_pyramid_pixels(int32_t H, int32_t W, int32_t levels);
size_t dqo_track_pyramid_workspace_bytes(void);
int dqo_track_pyramid(int32_t H, int32_t W, int32_t levels, const float* depth, const float* K, float* vertex, float* normal,
                      void* workspace, size_t workspace_bytes, void* hipStream);

/* IcpTracker.update_last_status (SLAM/icp.py:403-421), in place on render_depth [H, W]: where frame_depth > 0 and
 * (|render - frame| > sample_distance_threshold or render == 0 or 1 - cos(render_normal, frame_normal) > sample_normal_threshold),
 * render_depth takes frame_depth.  Normals [H, W, 3].  One launch. */
int dqo_track_fill_model_depth(int32_t H, int32_t W, float* render_depth, const float* frame_depth, const float* render_normal,
                               const float* frame_normal, float sample_distance_threshold, float sample_normal_threshold, void* hipStream);

/* predict_pose's failure test (SLAM/icp.py:7-14, 450-457): loss [1] = mean over all H * W pixels of ((R v1 + t - v0) . n0)^2 with
 * pose10's R, t — pixel-aligned, no data association; success [1] = !(loss > fail_threshold).  valid_count non-NULL: valid_ratio [1]
 * = valid_count / H / W in fp32 (the last ICP level's ratio when that level is this H x W).  Two launches. */
size_t dqo_track_p2p_workspace_bytes(void);
int dqo_track_p2p_loss(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* pose10,
                       float fail_threshold, const int32_t* valid_count, float* loss, int32_t* success, float* valid_ratio, void* workspace,
                       size_t workspace_bytes, void* hipStream);

/* dqo_traj_append / dqo_track_world_maps / dqo_eval_ate (ABI 5, symbols-only addition) — the trajectory on the device: the stretch of
 * Tracker.tracking between the tracker's answer and the mapper's input (SLAM/multiprocess/tracker.py:307-339), the mapper's keyframe
 * test and the tracking metric, nothing read back.  csrc/map_traj.hip lists every statement in order; tests/traj_oracle.py restates them.
 *
 * dqo_traj_append — one launch per frame.  The trajectory is caller-owned device memory of capacity cap rows:
 *     pose [cap,16] double   world poses c2w, row-major          pose_gt [cap,16] double   may be NULL when gt is never given
 *     flags [cap] int32      DQO_TRAJ_* bits                      kf_metric [cap,2] double  (theta in degrees, l2) of a tested row, else 0
 *     header [DQO_TRAJ_HEADER_WORDS] int32: the row count, the row of the last keyframe (-1: none yet), the overflow word; the caller
 *       sets (0, -1, 0, 0) once.  The launch reads the row index i from the header and advances it itself, so a captured graph appends
 *       correctly.  A full store (i >= cap) writes nothing but overflow = 1.
 *   World pose (tracker.py:312-327): exactly one of rel (float32 [4,4], the tracker's pose_t1_t0: pose[i] = pose[i-1] @ double(rel) in
 *     double, :324; row 0 takes init_pose, identity when NULL, :318) and abs_pose (double [4,4]: pose[i] = abs_pose — use_gt_pose :313, an
 *     ORB-refined pose :322).  gt (double [4,4], may be NULL) is copied to pose_gt[i] (:308).
 *   The frame's camera — Camera.updatePose / update (scene/cameras.py:165-183) — into float32 device buffers, NULL skips one:
 *     c2w [16] = pose[i] rounded once; viewmatrix [16] = the double inverse of the affine pose (by the cofactors of its 3x3 block, as
 *     np.linalg.inv :166, never the transpose) transposed and rounded once (world_view_transform :174-178); projmatrix [16] = the double
 *     w2c transposed @ double(projection), rounded once (full_proj_transform :179-183, which forms it in float32 from the rounded
 *     viewmatrix and lands up to 1.25 ulp from this; projection: device float32 [4,4], transposed as the reference keeps it);
 *     campos [3] = pose[i]'s translation (Camera.update never refreshes camera_center: the reference keeps the constructor's).
 *   Keyframe test — check_keyframe (SLAM/multiprocess/mapper.py:734-773; rot_compare / trans_compare SLAM/utils.py:42-54) on the rows
 *     i == 0 || (i + 1) % gaussian_update_frame == 0 (0: never): the first tested row enters the keyframe list and reports "not a
 *     keyframe" (:736-748); any other is a keyframe iff theta > theta_thres || l2 > trans_thres against the last keyframe row (cos not
 *     clamped: NaN compares false, as in numpy) and then becomes the last keyframe.
 * DQO_ERR_INVALID_ARG before the launch: cap < 1, a NULL store, both or neither of rel / abs_pose, gt without pose_gt, projmatrix without
 *   projection, gaussian_update_frame < 0. */
enum { DQO_TRAJ_HEADER_COUNT = 0, DQO_TRAJ_HEADER_LAST_KEYFRAME = 1, DQO_TRAJ_HEADER_OVERFLOW = 2, DQO_TRAJ_HEADER_WORDS = 4 };
enum {
    DQO_TRAJ_TESTED = 1,   /* check_keyframe ran for the row */
    DQO_TRAJ_KEYFRAME = 2, /* its return value */
    DQO_TRAJ_LISTED = 4    /* the row is in the keyframe list (row 0 is, and reports "not a keyframe") */
};
int dqo_traj_append(int32_t cap, double* pose, double* pose_gt, int32_t* flags, double* kf_metric, int32_t* header, const float* rel,
                    const double* abs_pose, const double* init_pose, const double* gt, const float* projection, float* c2w,
                    float* viewmatrix, float* projmatrix, float* campos, int32_t gaussian_update_frame, double theta_thres,
                    double trans_thres, void* hipStream);

/* transform_map of the frame's two maps (tracker.py:332-337, SLAM/utils.py:56-63) in one pixel launch: vertex_w = ((r0 x + r1 y) + r2 z) + t
 * per component with c2w's rows (device float32 [16]), normal_w the same with the rotation only (get_rot, utils.py:30-33); float32, one
 * rounding per operation.  Maps [H,W,3]; a zero vertex maps to t, as the reference's does.  normal_c / normal_w may both be NULL.  An
 * output may be its input.  Each map is read and written once, 16 bytes per lane when all four addresses are 16-byte aligned.
 * DQO_ERR_INVALID_ARG before the launch: H * W < 1 or too large, a NULL vertex map or c2w, one normal pointer without the other. */
int dqo_track_world_maps(int32_t H, int32_t W, const float* vertex_c, const float* normal_c, const float* c2w, float* vertex_w,
                         float* normal_w, void* hipStream);

/* The ATE curve of Tracker.eval_total_ate (tracker.py:341-346, 426-430; eval_ate / align SLAM/utils.py:486-532) in one launch:
 * ate[i-1] = eval_ate over the first i points, in centimetres, for i = 1..N.  Argument order as Tracker.eval_ate calls it (:429):
 * model = ground truth, data = estimate.  A stream is (pointer, doubles between points, doubles between a point's components):
 * (p, 3, 1) for a packed [N,3], (poses + 3, 16, 4) for the translation column of a [N,4,4] pose stack.
 * One block per prefix, three passes in double — the means; the 3x3 sum of outer products of the zero-centred points (:502-507); the sum
 * of squared lengths of R (m - mean m) - (d - mean d), then sqrt(sum / i) * 100 (:515-531) — with R from Horn's quaternion form (the
 * eigenvector of the largest eigenvalue of the symmetric 4x4, cyclic Jacobi): always a proper rotation, which is what the SVD with
 * S[2,2] = -1 of :508-512 yields.  Sums are added in a fixed order: a curve is bitwise reproducible.
 * fit [12] double, may be NULL: rot (row-major) and trans of the full trajectory's alignment (:512-513).
 * workspace: dqo_eval_ate_workspace_bytes(N) bytes (0 for a bad N), ANY contents; on return it holds the alignment of every prefix,
 *   [N,12] double.  DQO_ERR_INVALID_ARG before the launch: N outside [1, DQO_ATE_MAX_POINTS], a NULL stream of positions or ate, a
 *   negative stride.  DQO_ERR_WORKSPACE: the workspace is NULL or too small. */
#define DQO_ATE_MAX_POINTS (1 << 24)
size_t dqo_eval_ate_workspace_bytes(int32_t N);
int dqo_eval_ate(int32_t N, const double* model, int64_t model_stride, int64_t model_cstride, const double* data, int64_t data_stride,
                 int64_t data_cstride, double* ate, double* fit, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_prune_cameras / dqo_prune_touch / dqo_prune_rows (ABI 5, symbols-only addition) — floater pruning: Mapping.to_purne with
 * create_virtual_cameras (SLAM/multiprocess/mapper.py:424-529) on one map whose rows carry `stable` and `frame_id`
 * (GaussianPointCloud._frame_ids, SLAM/gaussian_pointcloud.py:52, 230-231, 277-279, 435), nothing read back, every row rewritten in place.
 * csrc/map_prune.hip lists every statement in order; tests/prune_oracle.py restates them.
 *
 * dqo_prune_cameras — replaces :471-481 and create_virtual_cameras (:424-466) with frame.update (scene/cameras.py:169-183) of :497.  One
 *   launch, one lane, double, one rounding per statement, none contracted.  viewmatrix: the keyframe's float32 [4,4] as in the raster
 *   settings (the transposed w2c); projection: float32 [4,4], transposed as the reference keeps it (dqo_traj_append's argument); depth:
 *   the frame's depth map, float32 [H*W]; pixel: the index read from it; cos_t, sin_t: cos / sin of the angle, formed by the HOST in double.
 *     W2V[a][b] = viewmatrix[b][a]; Rw = W2V[:3,:3]; T = W2V[:3,3]; d0 = depth[pixel]; d = d0 == 0 ? -1 : -d0;
 *     focal = T + d * Rw[:,2]; offset = T - focal; for A_k = Ry(+t), Ry(-t), Rx(+t), Rx(-t) (rotation_matrix's signs, :431-443):
 *     R_k = A_k @ Rw, T_k = A_k @ offset + focal, every entry (a0 b0 + a1 b1) + a2 b2.
 *   out_viewmatrix [4,4,4]: [k][:3,:3] = float(R_k) as it stands, [k][3,:3] = float(T_k), last column (0,0,0,1) — update() takes R_k for
 *   the camera's R.  out_projmatrix [4,4,4]: float(viewmatrix_k in double @ double(projection)), entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
 *   rounded once (the departure dqo_traj_append documents).  out_focal [3]: float(focal), for inspection.  campos is not formed:
 *   Camera.update never refreshes camera_center, the reference renders the virtual views with the real camera's centre.
 *   The reference's quirks are kept: `cx, cy = int(frame.cy), int(frame.cx)` then depth_map[cy, cx] reads row int(frame.cx), column
 *   int(frame.cy) (the caller forms `pixel`); camera_T is the w2c translation used as a position; update() is handed a w2c rotation
 *   where it expects the transposed one.  The frame is not mutated, so the restore of :529 has no counterpart.
 *   DQO_ERR_INVALID_ARG before the launch: H * W < 1 or too large, a NULL pointer, pixel outside [0, H * W).
 * dqo_prune_touch — replaces `n_touched += render_output["n_touched"]` (:506-508); one launch per virtual camera directly behind its
 *   render, one thread per row: touched[i] = 1 where n_touched[i] != 0.  render_header: the device header of that render (the start of
 *   its geometry buffer), or NULL.  A render that overflowed its capacity (overflow != 0) left n_touched at zero for every row: the launch
 *   then marks nothing and counts an invalid render.  DQO_ERR_INVALID_ARG: P < 0, NULL n_touched; DQO_ERR_WORKSPACE.
 * dqo_prune_rows — replaces :509-527 (the mask, its .item(), GaussianPointCloud.delete of both clouds); one launch, one thread per row.
 *   A row with alive != 0 && lo < frame_id <= hi is in the window ((keyframe_list[-2].uid, keyframe_list[-1].uid], or (uid - 1, uid]
 *   with one keyframe, :510-515).  If no render since the last call was invalid, a window row with touched == 0 is deleted: xyz = park,
 *   opacity_raw = scaling_raw = -10, alive = 0, row_flags = DQO_ROW_HIDDEN | DQO_ROW_FROZEN, confidence = 0, and 0 into stable / add_tick
 *   / both counters / frame_id (what dqo_map_lifecycle_rows writes into a freed row, plus frame_id).  Every touched word and both render
 *   counts are cleared as they are read.  stats[8] (overwritten): rows in the window, deleted unstable, deleted stable, valid renders,
 *   skipped (1: some render was invalid, nothing was deleted), rows alive afterwards, 0, 0.  With P == 0 stats is all zero.
 *   A row dqo_map_lifecycle_rows frees keeps a stale frame_id; nothing reads it while alive == 0.
 *   DQO_ERR_INVALID_ARG before the launch: P < 0, lo > hi, NULL stats, a NULL per-Gaussian buffer or park; DQO_ERR_WORKSPACE.
 * workspace: dqo_prune_workspace_bytes(P) bytes, ZERO when first used and then left to these calls (dqo_prune_rows hands it back zero). */
size_t dqo_prune_workspace_bytes(int32_t P);
int dqo_prune_cameras(int32_t H, int32_t W, const float* viewmatrix, const float* projection, const float* depth, int64_t pixel, double cos_t,
                      double sin_t, float* out_viewmatrix, float* out_projmatrix, float* out_focal, void* hipStream);
int dqo_prune_touch(int32_t P, const int32_t* n_touched, const DqoRastHeader* render_header, void* workspace, size_t workspace_bytes,
                    void* hipStream);
int dqo_prune_rows(int32_t P, float* xyz, float* opacity_raw, float* scaling_raw, float* confidence, uint8_t* alive, uint8_t* row_flags,
                   uint8_t* stable, int32_t* add_tick, int32_t* depth_error_counter, int32_t* color_error_counter, int32_t* frame_id,
                   const float* park, int32_t lo, int32_t hi, void* workspace, size_t workspace_bytes, int32_t* stats, void* hipStream);

/* dqo_tsdf_clear / dqo_tsdf_integrate / dqo_tsdf_extract (ABI 5, symbols-only addition) — the map as a triangle mesh: what make_mesh.py
 * and eval_frame(..., volume=..., scale=...) (SLAM/eval.py:299, 316-343: every frame's render becomes an RGB-D image, then
 * volume.integrate(rgbd, intrinsics, w2c) on an open3d TSDF volume) are there to produce.  The shipped make_mesh.py breaks off inside its
 * loop and open3d does not exist on this platform, so THIS text defines the rule (it follows open3d's UniformTSDFVolume integrate as
 * published) and tests/tsdf_oracle.py restates it in numpy; nothing is pinned against the library.  csrc/map_tsdf.hip lists every
 * statement in order.  Plain arguments, no struct.
 *
 * The volume: a DENSE uniform grid over the caller's box (not open3d's hashed blocks) of nx x ny x nz voxels, x fastest, lattice point
 *   (x, y, z) at origin + (index + 0.5) * voxel_length.  The caller owns the device tensors, a structure of arrays: tsdf float32
 *   [nz,ny,nx], weight float32 [nz,ny,nx], color float32 [3,nz,ny,nx], header int32 [8].  Every entry refuses, before any launch
 *   (DQO_ERR_INVALID_ARG), a side below 2 and nx * ny * nz >= 2^28.
 * dqo_tsdf_clear — one launch (no memset): tsdf = 1, weight = 0, color = 0, header = 0.
 * dqo_tsdf_integrate — one frame, one launch, one thread per voxel, float32, one rounding per operation, left to right, none contracted,
 *   division and square root correctly rounded.  depth float32 [H,W] in metres, image float32 [3,H,W], fx fy cx cy the pinhole
 *   intrinsics, w2c 16 floats in DEVICE memory, row major (world to camera), m below:
 *       pw_a = origin_a + ((float)i_a + 0.5f) * L                                  a = x, y, z
 *       pc_r = ((m[r][0] * pw_x + m[r][1] * pw_y) + m[r][2] * pw_z) + m[r][3]
 *       skip unless pc_z > 0
 *       u_f = ((pc_x * fx) / pc_z + cx) + 0.5f;  v_f likewise with fy, cy
 *       skip unless u_f >= 0.0001f && u_f < (float)W - 0.0001f                     (the same for v_f and H)
 *       u = (int)u_f;  v = (int)v_f;  d = depth[v][u]
 *       skip unless d > 0 && d <= depth_trunc
 *       mult = sqrtf((1.0f + ((u - cx) / fx) * ((u - cx) / fx)) + ((v - cy) / fy) * ((v - cy) / fy))
 *       sdf = (d - pc_z) * mult;  skip unless sdf > -sdf_trunc
 *       t = fminf(1.0f, sdf / sdf_trunc);  w = weight
 *       tsdf = (tsdf * w + t) / (w + 1.0f);  color_c = (color_c * w + image[c][v][u]) / (w + 1.0f);  weight = w + 1.0f
 *   Every skip comes before the thread's first access to the volume; a touched voxel reads 20 bytes and writes 20, plus one gathered
 *   pixel.  render_header (may be NULL): the device header of the forward that rendered the frame; a render that outgrew its context
 *   (overflow != 0, as dqo_eval_picture tests it) integrates nothing and adds 1 to header[5]; every other frame adds 1 to header[4].
 *   DQO_ERR_INVALID_ARG before the launch: bad dims, voxel_length or sdf_trunc not above 0, a bad image size, a NULL pointer.
 * dqo_tsdf_extract — the volume as a welded, indexed, coloured triangle mesh in caller-owned device buffers: vertices float32
 *   [cap_vertices,3], vertex_color float32 [cap_vertices,3], faces int32 [cap_faces,3].  Marching tetrahedra on the Kuhn decomposition
 *   (no marching-cubes table; watertight by construction); four launches, no host read, no float atomics, the same bits on every run.
 *     - a cube is the lattice points o + {0,1}^3, named by o, valid iff all eight weights are > 0; the corner o + (dx,dy,dz) has code
 *       dx + 2 dy + 4 dz.  Tetrahedron k belongs to the k-th permutation p of (0,1,2) in lexicographic order, path corners c0 = o,
 *       c1 = c0 + e[p0], c2 = c1 + e[p1], c3 = o + (1,1,1).
 *     - the edges are of seven translation-invariant types, offsets (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = types 0..6;
 *       an edge is owned by its lower lattice point.  A corner is negative iff tsdf < 0.  An edge carries a vertex iff its ends differ in
 *       sign and at least one valid cube contains it: no vertex is unreferenced.
 *     - with a the negative end, s = f_a / (f_a - f_b); position and colour are p_a + s * (p_b - p_a) per component (float32, one
 *       rounding each).  Vertices are numbered in ascending (lattice linear index, edge type).
 *     - triangles per tetrahedron case (bit i: path corner i is negative): one negative corner a — the edges (a,b) for the positive b
 *       ascending; three — the edges (a,b) for the negative a ascending; two, a0 < a1 and b0 < b1 — the quad (a0b0, a0b1, a1b1, a1b0) cut
 *       into (q0,q1,q2), (q0,q2,q3).  The last two indices are swapped iff FLIP[case] XOR parity(p), FLIP = cases 0010 0101 1000 1010
 *       1011 1110 (bit 3 first): the right-hand normal points to the positive side, free space.  Faces are numbered in ascending (cube
 *       linear index, tetrahedron, triangle).
 *     - capacities: the vertex list is cut at cap_vertices; the faces that name a cut vertex leave the list; what is left is cut at
 *       cap_faces.  Nothing is written behind either.  header[0..3] = vertices written, faces written, vertices dropped, faces dropped.
 *   DQO_ERR_INVALID_ARG before any launch: bad dims, a NULL volume buffer or header, a capacity below 0, a NULL mesh buffer with a
 *   capacity above 0; DQO_ERR_WORKSPACE.
 * workspace: dqo_tsdf_workspace_bytes(nx, ny, nz) bytes (0 for bad dims; 5 bytes per voxel and 12 per 2048 voxels behind the ticket words),
 *   ZERO when first used and then left to dqo_tsdf_extract, which hands it back ready for the next call.
 * Laplacian smoothing (the mesh_smooth_iter / mesh_smooth_lambda keys of configs/Cube_Diorama_base.yaml:45-46, read by nothing in the
 *   reference tree) is dqo_mesh_smooth below.  Simplification is dqo_mesh_simplify below.  Not built: hashed or sparse volumes, merging the volumes of shards. */
size_t dqo_tsdf_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int dqo_tsdf_clear(int32_t nx, int32_t ny, int32_t nz, float* tsdf, float* weight, float* color, int32_t* header, void* hipStream);
int dqo_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_length,
                       float sdf_trunc, float* tsdf, float* weight, float* color, int32_t* header, int32_t W, int32_t H, const float* depth,
                       const float* image, float fx, float fy, float cx, float cy, const float* w2c, float depth_trunc,
                       const DqoRastHeader* render_header, void* hipStream);
int dqo_tsdf_extract(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_length,
                     const float* tsdf, const float* weight, const float* color, float* vertices, float* vertex_color, int32_t* faces,
                     int32_t cap_vertices, int32_t cap_faces, int32_t* header, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_components / dqo_mesh_smooth / dqo_mesh_normals (ABI 5, symbols-only addition) — the clean-up of the mesh dqo_tsdf_extract
 * leaves, on the device: what a SLAM mesh pipeline does with open3d before it reports or shows a mesh.  open3d does not exist on this
 * platform, so THIS text defines the rules (they follow open3d's published algorithms; every departure is marked) and
 * tests/mesh_ops_oracle.py restates them in numpy; nothing is pinned against the library.  csrc/map_meshops.hip lists the launches.
 *
 * The operand: an indexed mesh in caller-owned device buffers, laid out as dqo_tsdf_extract's output — vertices float32 [cap_vertices,3],
 *   colors float32 [cap_vertices,3] (may be NULL), faces int32 [cap_faces,3] — and counts, a device pointer to two int32 (vertices, faces;
 *   words 0 and 1 of a TSDF header or of dqo_mesh_components' header fit directly; NULL: the capacities are the counts; a count is clamped
 *   to [0, capacity]).  V and F below are the counts.  Rows behind the counts are never read and never written.  Grids are sized from the
 *   capacities: the launch count is a fixed function of the arguments, never of the data; no host read, no synchronise, no memset, no float
 *   atomics — every entry can be captured in a hipGraph.  A face is VALID iff its three indices lie in [0, V).
 *   Every entry refuses, before any launch (DQO_ERR_INVALID_ARG), a capacity outside 1 <= cap_vertices, cap_faces < 2^28 and a NULL
 *   vertices / faces pointer; then a short workspace (DQO_ERR_WORKSPACE).
 *
 * dqo_mesh_components — open3d's cluster_connected_triangles + remove_triangles_by_mask + remove_unreferenced_vertices.  Eleven launches.
 *     - two faces are connected iff they share a vertex INDEX.  (Departure: open3d clusters by shared edges; the two differ only at
 *       non-manifold pinch vertices, where two sheets touch in one vertex.)
 *     - a face that is not valid belongs to no component: it is dropped and counted.  A face with a repeated index is a face like any other.
 *     - a component's label is the smallest vertex id in it, its size its number of faces.
 *     - threshold = max(min_faces, largest_only ? the size of the largest component : 0); a face is kept iff its component's size >=
 *       threshold (components tied for largest are all kept).
 *     - kept faces keep their order; the vertices they reference keep their order and are renumbered densely; positions and colours are
 *       copied bit for bit.
 *   Outputs: the out mesh in separate buffers (out_vertices, out_colors — ignored when colors is NULL — and out_faces must not be the
 *   input's; their capacities must not be below the input's, so nothing can be cut); labels (may be NULL) int32 [cap_faces]: a face's
 *   label, -1 for a dropped bad face; header int32 [8]: [0] vertices written, [1] faces written (so the header is the next operator's
 *   counts), [2] components, [3] components kept, [4] faces with a bad index, [5] the largest component's faces, [6] vertices removed,
 *   [7] faces removed by the threshold.
 *   A lock-free union-find over the vertices (the larger root goes under the smaller by a returning compare-and-swap, with path halving:
 *   the final root is the component's minimum whatever order the hardware ran in), sizes by integer atomics aggregated per wave and root,
 *   compaction by block counts and a last-block scan.  The same bits on every run.
 *   DQO_ERR_INVALID_ARG also for min_faces < 0, a NULL header or out buffer, an out buffer that is the input's, a header that is the
 *   input's counts (the first launch clears the header before any launch reads the counts), an out capacity below the
 *   input's.
 *
 * dqo_mesh_smooth — open3d's filter_smooth_laplacian (configs/Cube_Diorama_base.yaml:45-46: mesh_smooth_iter = iterations,
 *   mesh_smooth_lambda = lambda) and, with mu != 0, filter_smooth_taubin (open3d's defaults: lambda 0.5, mu -0.53), in place.
 *   Adjacency, the same for every iteration of a call: N(i) = the vertices that share a valid face with i, i itself excluded, each once,
 *   in ascending id order.  One step with factor L, for every vertex with N(i) non-empty, in DOUBLE from the float32 values of the step
 *   before, every operation rounded once, none contracted, sums left to right from 0 over ascending neighbour id, sqrt and division
 *   correctly rounded:
 *       d_n = p_i - p_n;  dist = sqrt((d_x * d_x + d_y * d_y) + d_z * d_z);  w_n = 1 / (dist + 1e-12)
 *       S = sum w_n * p_n;  T = sum w_n;  p_i' = (float)(p_i + L * (S / T - p_i))
 *   Colours, when the scope includes them, use the same w_n — taken from the positions BEFORE the step — in place of p in the last line.
 *   A vertex without neighbours is copied unchanged (departure: open3d divides by zero there); rounding to float32 between steps is a
 *   departure too (open3d keeps doubles).  mu == 0: an iteration is one step with lambda; otherwise a step with lambda, then one with mu.
 *   scope: DQO_MESH_SMOOTH_POSITIONS, _COLOURS (positions give the weights and stay), _BOTH.  iterations == 0: nothing is launched.
 *   Five launches build the adjacency as a CSR (count by integer atomics, scan, fill through an atomic cursor, then every vertex's segment
 *   is sorted and made unique — by its thread up to 32 raw entries, by its block beyond: nothing depends on the fill's order), then one
 *   launch per step, one thread per vertex, and a copy after an odd number of steps (the workspace holds the other half of the ping-pong).
 *   DQO_ERR_INVALID_ARG also for iterations < 0, a lambda or mu that is not finite, a bad scope, NULL colors with a scope that needs them.
 *
 * dqo_mesh_normals — open3d's compute_vertex_normals: normals float32 [cap_vertices,3].  Face normal n_f = cross(p1 - p0, p2 - p0) in
 *   double, un-normalised (the sum is area-weighted), each component a * b - c * d with one rounding per operation.  A vertex's normal is
 *   the sum, from 0, of the normals of its incident valid faces in ascending face index — a face that names the vertex twice counts once
 *   per corner, as open3d's loop does — divided by its length sqrt((x * x + y * y) + z * z) and rounded once to float32.  A zero or
 *   non-finite length gives (0, 0, 1): an unreferenced vertex, a vertex with only degenerate faces.  The CSR build of dqo_mesh_smooth with
 *   a corner's face in place of its two neighbours (five launches), then one thread per vertex.
 *
 * workspaces: dqo_mesh_components_workspace_bytes / dqo_mesh_smooth_workspace_bytes / dqo_mesh_normals_workspace_bytes (cap_vertices,
 *   cap_faces): 0 for bad capacities; ZERO when first used and then left to the entry, which hands it back ready for the next call.
 * Not built: edge-based clustering, hole filling, smoothing of normals; simplification is dqo_mesh_simplify below. */
#define DQO_MESH_SMOOTH_POSITIONS 0
#define DQO_MESH_SMOOTH_COLOURS 1
#define DQO_MESH_SMOOTH_BOTH 2
size_t dqo_mesh_components_workspace_bytes(int32_t cap_vertices, int32_t cap_faces);
size_t dqo_mesh_smooth_workspace_bytes(int32_t cap_vertices, int32_t cap_faces);
size_t dqo_mesh_normals_workspace_bytes(int32_t cap_vertices, int32_t cap_faces);
int dqo_mesh_components(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                        int32_t cap_faces, int32_t min_faces, int32_t largest_only, float* out_vertices, float* out_colors,
                        int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* labels, int32_t* header,
                        void* workspace, size_t workspace_bytes, void* hipStream);
int dqo_mesh_smooth(float* vertices, float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                    int32_t iterations, double lambda, double mu, int32_t scope, void* workspace, size_t workspace_bytes, void* hipStream);
int dqo_mesh_normals(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                     float* normals, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_simplify (ABI 5, symbols-only addition) — the mesh with fewer triangles, by vertex clustering on the device: open3d's
 * simplify_vertex_clustering(voxel_size, SimplificationContraction::Average).  Marching tetrahedra leave about twice the triangles of
 * marching cubes, at lattice resolution on flat walls too; a pipeline that reports or shows a mesh decimates it first.  open3d does not
 * exist on this platform, so THIS text defines the rule (every departure is marked) and tests/mesh_simplify_oracle.py restates it in
 * numpy; nothing is pinned against the library.  The operand, the counts and the common refusals are those of the three operators above;
 * csrc/map_meshops.hip lists the launches.  Twelve launches, whatever the data.
 *     - cells: for vertex v < V and axis a, t_a = ((double)p_a - origin_a) / voxel_size in double, one rounding per operation, none
 *       contracted; i_a = floor(t_a).  The vertex is IN THE GRID iff the three t_a are finite and 0 <= i_a < 2^21; its cell is
 *       (i_x, i_y, i_z).  (Departure: open3d puts the grid at the bounding box's minimum minus half a voxel; here the caller gives the
 *       origin, which costs no reduction and no host read — the caller of a TSDF mesh has the volume's origin.)
 *     - clusters: a cluster is the set of in-grid vertices of one cell; its representative is its smallest vertex id.
 *     - faces, classified in this order: not valid — dropped, counted in [4]; names a vertex outside the grid — dropped, [5]; two corners
 *       share a cluster — collapsed, [6]; otherwise LIVE.  A live face's triple of clusters is rotated so that the smallest comes first
 *       (the orientation stays, as in open3d).  Among the live faces with the same rotated triple the one with the lowest face index is
 *       kept, the others are duplicates, [7].  Kept faces keep their input order.
 *     - output vertices: a cluster is written iff a live face names it; written clusters are numbered densely in ascending representative
 *       id.  (Departure: open3d keeps a cluster none of whose triangles survive as an unreferenced vertex; here it goes, which is what
 *       remove_unreferenced_vertices would do next.)
 *     - position and colour of a written cluster of n members, in double: S = 0; S = S + (double)p_m over the members m in ASCENDING
 *       vertex id; the result is (float)(S / (double)n) per component; colours the same way.  A cluster of one member is copied bit for
 *       bit (for every value but -0 and a NaN's payload that is what the formula gives).
 *   voxel_size, origin_x, origin_y, origin_z: doubles.  Outputs: the out mesh in separate buffers, under dqo_mesh_components' conditions
 *   (not the input's buffers, capacities not below the input's: nothing can be cut; out_colors is ignored when colors is NULL); header
 *   int32 [8]: [0] vertices written, [1] faces written (so the header is the next operator's counts), [2] clusters formed, before the
 *   unreferenced ones go, [3] vertices outside the grid, [4] faces with a bad index, [5] faces with a vertex outside the grid, [6] faces
 *   collapsed, [7] duplicate faces removed.  valid faces = [1] + [5] + [6] + [7]; [0] <= [2] <= V - [3].
 *   No device-wide sort: two open-addressed tables (vertex ids keyed by the cell, face indices keyed by the rotated triple; a power of two
 *   of slots, at least twice the entries; linear probing, every probe loop bounded by the slot count; a compare-and-swap claims an empty
 *   slot, an occupant with the same key makes it an integer atomic minimum, and a slot's key never changes — so a slot ends at the
 *   smallest id of its key whatever order the hardware ran in), member lists by the count, scan and fill of dqo_mesh_smooth's CSR build
 *   with the cluster as the segment's owner, put in ascending order by counting (a member's place is the number of ids below its own;
 *   lists above 2048 members: a bitonic network), compaction by span counts and a last-block scan.  Integer atomics only: the same bits
 *   on every run.
 *   DQO_ERR_INVALID_ARG before any launch also for a NULL header or out buffer, an out buffer that is the input's, a header that is the
 *   input's counts, an out capacity below the input's, a voxel_size that is not finite or not above 0, an origin that is not finite;
 *   then DQO_ERR_WORKSPACE.
 * workspace: dqo_mesh_simplify_workspace_bytes(cap_vertices, cap_faces): 0 for bad capacities; ZERO when first used and then left to the
 *   entry, which hands it back ready for the next call.
 * Not built: quadric-error placement of a cluster's vertex, normals carried through (dqo_mesh_normals recomputes them), edge-collapse
 *   decimation. */
size_t dqo_mesh_simplify_workspace_bytes(int32_t cap_vertices, int32_t cap_faces);
int dqo_mesh_simplify(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                      int32_t cap_faces, double voxel_size, double origin_x, double origin_y, double origin_z, float* out_vertices,
                      float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* header,
                      void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_cull (ABI 5, symbols-only addition) — a mesh restricted to what K views see: the frustum test and the occlusion test against
 * the frames' depth that the mesh-evaluation protocols of dense SLAM (the NICE-SLAM lineage) apply to the reconstructed AND the
 * ground-truth mesh before they sample them, so that neither is charged for surface no camera looked at.  Neither a reference
 * implementation nor open3d exists on this platform, so THIS text defines the rule and tests/mesh_cull_oracle.py restates it in numpy;
 * nothing is pinned against a library.  The operand, the counts and the common refusals are those of dqo_mesh_components;
 * csrc/map_meshcull.hip lists the launches.  Six launches, whatever the data.  Plain arguments, no struct.
 *   Views: n_views in [1, 65535]; w2c float32 [n_views,16] in DEVICE memory, row major, world to camera (dqo_tsdf_integrate's
 *   convention), m below; view_keep uint8 [n_views] (may be NULL: every view is USED; otherwise the views with a byte != 0 are); W, H,
 *   fx, fy, cx, cy: the pinhole camera all views share; depth float32 [n_views,H,W] in metres, device (may be NULL: frustum test
 *   only); near (finite, >= 0), eps (finite, >= 0), depth_trunc (> 0, may be +inf): host floats.
 *   Per vertex v < V at (x, y, z) and used view k — float32, one rounding per operation, left to right, none contracted, division
 *   correctly rounded; the projection is dqo_tsdf_integrate's own statements, so a mesh is culled by exactly the pixels that made it:
 *       pc_r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3]                r = 0, 1, 2
 *       not seen unless pc_z > near
 *       u_f = ((pc_x * fx) / pc_z + cx) + 0.5f;  v_f likewise with fy, cy
 *       not seen unless u_f >= 0.0001f && u_f < (float)W - 0.0001f                  (the same for v_f and H)
 *       depth == NULL: seen
 *       else u = (int)u_f;  v = (int)v_f;  d = depth[k][v][u];
 *            seen iff d > 0 && d <= depth_trunc && pc_z <= d + eps                   (d + eps: one float32 add)
 *   views(v) = the number of used views that see v.
 *     - a face is KEPT iff it is valid and at least min_corners (1, 2 or 3) of its corners have views > 0; a repeated index counts once
 *       per corner.
 *     - kept faces keep their order; the vertices they reference keep their order and are renumbered densely; positions and colours are
 *       copied bit for bit (dqo_mesh_components' compaction rules).  A seen vertex that no kept face names is dropped.
 *   Outputs: the out mesh in separate buffers, under dqo_mesh_components' conditions (not the input's buffers, capacities not below the
 *   input's: nothing can be cut; out_colors is ignored when colors is NULL); vertex_views (may be NULL) int32 [cap_vertices]: views(v)
 *   for v < V, rows behind V untouched; header int32 [8]: [0] vertices written, [1] faces written (so the header is the next operator's
 *   counts), [2] vertices with views > 0, [3] views used, [4] faces with a bad index, [5] faces removed by the rule, [6] vertices
 *   removed, [7] 0.  F = [1] + [4] + [5] and V = [0] + [6].
 *   The hot path is V x n_views: a grid over (256 vertices, 32 views); a view's matrix and its used bit are wave-uniform scalar loads,
 *   the vertex stays in registers, the one per-pair memory access is the gathered depth pixel, and a vertex's count is merged by one
 *   integer atomic add per chunk of views that saw it (without vertex_views a wave leaves its chunk once all its lanes are seen: no
 *   output can tell).  Compaction by span counts and a last-block scan.  Integer atomics only: the same bits on every run and under
 *   any schedule; no memset, no host read, no synchronise — the entry can be captured in a hipGraph.
 *   DQO_ERR_INVALID_ARG before any launch also for n_views outside [1, 65535], a NULL w2c, W or H below 1 or n_views * H * W not below
 *   2^40 (the kernel indexes the depth with size_t), a near or eps that is not finite or below 0, a depth_trunc that is not above 0,
 *   min_corners outside 1..3, a NULL header or out buffer, an out buffer that is the input's, a header that is the input's counts, an
 *   out capacity below the input's; then DQO_ERR_WORKSPACE.
 * workspace: dqo_mesh_cull_workspace_bytes(cap_vertices, cap_faces): 0 for bad capacities; ZERO when first used and then left to the
 *   entry, which hands it back ready for the next call.
 * Rendering the mesh to depth — for the Depth L1 number, or as this entry's `depth` where no sensor depth exists — is
 *   dqo_mesh_render_depth below.  Not built: per-view intrinsics or image sizes, triangle-frustum intersection (a large face whose
 *   corners all fall outside the image is dropped), exact point-to-triangle distances.  (That is this entry's rule and stays it;
 *   dqo_mesh_cull_faces below decides per FACE, by the pixels a face wins in a render, and keeps such a face.) */
size_t dqo_mesh_cull_workspace_bytes(int32_t cap_vertices, int32_t cap_faces);
int dqo_mesh_cull(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                  int32_t cap_faces, int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy,
                  float cx, float cy, const float* depth, float near, float eps, float depth_trunc, int32_t min_corners, float* out_vertices,
                  float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* vertex_views,
                  int32_t* header, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_cull_faces (ABI 5, symbols-only addition) — a mesh restricted to the faces that WIN PIXELS in a render of it: visibility per
 * face, where dqo_mesh_cull's is per vertex and drops a wall of two triangles whose corners all lie outside the image although it fills
 * it.  The operand, the counts, n_views, view_keep, W, H, the out mesh and the common refusals are dqo_mesh_cull's; tests/mesh_clip_oracle.py
 * restates the rule in numpy.  Six launches, whatever the data.  Plain arguments, no struct.
 *   face_index int32 [n_views,H,W] and rdepth float32 [n_views,H,W], device: a render of THIS mesh from the views —
 *   dqo_mesh_render_depth_clip's (or dqo_mesh_render_depth's) face_index and depth; depth float32 [n_views,H,W] (may be NULL): the
 *   frames' depth; eps (finite, >= 0), depth_trunc (> 0, may be +inf), min_pixels (>= 1).
 *   Pixel (k, Y, X) of a used view k, with f = face_index[k][Y][X], COUNTS for f iff
 *       0 <= f < F — anything else, -1 included, is ignored and never used as an index —, f is a valid face, and
 *       depth == NULL, or s = depth[k][Y][X] has s > 0 && s <= depth_trunc && rdepth[k][Y][X] <= s + eps       (one float32 add)
 *   — dqo_mesh_cull's occlusion statement with the render's depth in the place of the vertex's.  pixels(f) = the pixels that count
 *   for f.  A face is KEPT iff it is valid and pixels(f) >= min_pixels.  Compaction, renumbering and the bit-for-bit copies are
 *   dqo_mesh_cull's.
 *   Outputs: the out mesh; face_pixels int32 [cap_faces] (required, a buffer of its own): pixels(f) for f < F (0 for a face with a bad
 *   index), rows behind F untouched; header int32 [8]: [0] vertices written, [1] faces written, [2] faces with a pixel, [3] views
 *   used, [4] faces with a bad index, [5] faces removed by the rule, [6] vertices removed, [7] pixels counted, summed over the faces (its
 *   low 32 bits).  F = [1] + [4] + [5] and V = [0] + [6].
 *   The hot path is n_views x H x W pixels.  A wall wins most of a view, so one add per pixel would queue on one address: a wave walks
 *   consecutive pixels, a lane shift and a ballot find the heads of the runs of one face id across its 64 lanes, a run is ONE integer
 *   add, and a run that goes on through whole rounds of 64 rides in a scalar until it ends.  Integer adds only: the same bits on every
 *   run and under any schedule; no memset, no host read, no synchronise — the entry can be captured in a hipGraph.
 *   DQO_ERR_INVALID_ARG before any launch for dqo_mesh_cull's refusals of the operand, n_views, the image size, eps, depth_trunc and
 *   the out mesh, and also for a NULL face_index, rdepth or face_pixels, min_pixels below 1, a face_pixels that is the faces, the out
 *   faces, the header or the counts; then DQO_ERR_WORKSPACE.
 * workspace: dqo_mesh_cull_workspace_bytes(cap_vertices, cap_faces) is this entry's query too (mark, keep, the span pairs, the view
 *   bits; the per-face counts are the caller's face_pixels): ZERO when first used and then left to the entry. */
int dqo_mesh_cull_faces(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                        int32_t cap_faces, int32_t n_views, const uint8_t* view_keep, int32_t W, int32_t H, const int32_t* face_index,
                        const float* rdepth, const float* depth, float eps, float depth_trunc, int32_t min_pixels, float* out_vertices,
                        float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* face_pixels,
                        int32_t* header, void* workspace, size_t workspace_bytes, void* hipStream);

/* dqo_mesh_render_depth (ABI 5, symbols-only addition) — a triangle mesh rasterised to depth in K views: what the Depth L1 number of the
 * dense-SLAM evaluation protocols (the NICE-SLAM lineage) compares pixel by pixel for the reconstructed and the ground-truth mesh, and a
 * depth for dqo_mesh_cull's occlusion test where no sensor depth exists.  No rasterising library exists on this platform, so THIS text
 * defines the rule and tests/mesh_render_oracle.py restates it in numpy; nothing is pinned against a library.  The operand (vertices,
 * faces, counts, the capacities), the views (n_views, w2c, view_keep) and the camera (W, H, fx, fy, cx, cy, near, depth_trunc) are
 * dqo_mesh_cull's; csrc/map_meshrender.hip lists the launches.  Three launches, whatever the data.  Plain arguments, no struct.
 *   Per valid face f < F with corners i = 0, 1, 2 at vertex ids v_i, and used view k.
 *   float32, one rounding per operation, left to right, none contracted, division correctly rounded — dqo_mesh_cull's statements:
 *       pc_i,r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3]              r = 0, 1, 2; m = w2c[k]
 *       a corner is in front iff pc_i,z > near.  No corner in front: the pair is skipped silently.  Some but not all: the pair CROSSES
 *       THE NEAR PLANE and is dropped and counted — there is no clipping (a documented departure from a clipping rasteriser).
 *       x_i = (pc_i,x * fx) / pc_i,z + cx;  y_i likewise with fy, cy — dqo_mesh_cull's u_f without the + 0.5f: pixel centres sit at
 *       integer coordinates, and a mesh is rendered by the very projection that integrated and culled it.
 *       box: [ceil(min x_i), floor(max x_i)] x [ceil(min y_i), floor(max y_i)], a lower end below 0 set to 0 and an upper end above
 *       W - 1 (H - 1) set to that, in float32, before the conversion to int; unless lo <= hi on both axes the pair is skipped.
 *   double, from the widened floats, one rounding per operation, none contracted:
 *       for the edge between corners i and j let (p, q) be the two ordered by VERTEX ID, lower first;
 *       E = (x_q - x_p) * (Y - y_p) - (y_q - y_p) * (X - x_p);  e_ij = E if p is i, else -E.  Two faces that share an edge compute
 *       bitwise opposite values there: no pixel centre falls between them and none is lost on the edge.
 *       A = e_01 at (x_2, y_2).  A repeated vertex id or A == 0: the pair is DEGENERATE, counted and skipped.
 *       pixel (X, Y) of the box is covered iff A > 0 and e_01, e_12, e_20 are all >= 0, or A < 0 and they are all <= 0: inclusive,
 *       and both sides of a face are rendered (no back-face culling).
 *       depth by ray-plane intersection in camera space: n = (P_1 - P_0) x (P_2 - P_0) with P_i = pc_i;  r_x = (X - cx) / fx,
 *       r_y = (Y - cy) / fy;  nr = (n_x * r_x + n_y * r_y) + n_z;  nr == 0: no hit;
 *       z = ((n_x * P_0,x + n_y * P_0,y) + n_z * P_0,z) / nr, set to min pc_i,z where below it and to max pc_i,z where above it;
 *       d = (float)z;  a hit iff d > near && d <= depth_trunc.
 *   The pixel's key is the uint64 (float bits of d) << 32 | f, and a pixel keeps the MINIMUM key of its hits: the nearest face wins,
 *   equal depth goes to the lower face id, and the result does not depend on the order the faces arrive in — the same bits on every
 *   run and under any schedule.
 *   Outputs: depth float32 [n_views,H,W], 0 = no hit; face_index int32 [n_views,H,W] (may be NULL), -1 = no hit; the images of unused
 *   views are written as no hit.  header int32 [8]: [0] views used, [1] faces with a bad index, [2] pairs rasterised (in front, a box,
 *   not degenerate), [3] pairs dropped at the near plane, [4] degenerate pairs, [5] the pairs of [2] whose clipped box holds more than
 *   SMALL_MAX = 64 pixels (or is wider or taller than 64) — the pairs a whole wave walks, below —, [6] pixels hit, summed over the
 *   views (its low 32 bits), [7] 0.
 *   The hot path is F x n_views: a grid over (256 faces, 32 views); a view's matrix and its used bit are wave-uniform scalar loads,
 *   the face's nine corner floats stay in registers across the chunk.  A pair with a box of at most SMALL_MAX pixels is walked by its
 *   own lane; a larger one by the whole wave — a ballot finds the flagged lanes, the face's floats are broadcast, the 64 lanes stride
 *   the box in 8 x 8 pixel tiles — so no lane walks a wall-sized triangle alone.  Per hit one 64-bit no-return integer min atomic
 *   (a load of the pixel's key in front of it, to skip an atomic that cannot win, was measured slower and is not there:
 *   profiles/mesh_render.txt).  Integer atomics only; no memset, no host read, no synchronise — the entry can be captured in a hipGraph.
 *   DQO_ERR_INVALID_ARG before any launch for dqo_mesh_cull's refusals of the operand, the views and the camera, and also for W or H
 *   above 2^24 (W - 1 must be an exact float32), cap_faces * n_views not below 2^31 (the pair counts are int32: a caller with more
 *   views renders them in chunks), a NULL depth, a header that is the mesh's counts; then DQO_ERR_WORKSPACE.
 * workspace: dqo_mesh_render_depth_workspace_bytes(n_views, W, H): 0 for a bad size; it holds the 8-byte keys, which the first launch
 *   clears; its head is ZERO when first used and then left to the entry, which hands it back ready for the next call.
 * Not built: near-plane clipping, back-face culling, per-view intrinsics or image sizes, colour or normal shading of the mesh.
 * (That is this entry's rule and stays it; dqo_mesh_render_depth_clip below is the entry that clips at the near plane.) */
size_t dqo_mesh_render_depth_workspace_bytes(int32_t n_views, int32_t W, int32_t H);
int dqo_mesh_render_depth(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                          int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy, float cx,
                          float cy, float near, float depth_trunc, float* depth, int32_t* face_index, int32_t* header, void* workspace,
                          size_t workspace_bytes, void* hipStream);

/* dqo_mesh_render_depth_clip (ABI 5, symbols-only addition) — dqo_mesh_render_depth with the near plane CLIPPED: a camera that stands in a
 * room is within one triangle of its floor or of a wall, and a wall of two triangles that crosses the near plane is most of the image.
 * Arguments, refusals, workspace (dqo_mesh_render_depth_workspace_bytes), the three launches, the key and the outputs are
 * dqo_mesh_render_depth's; header[3] counts the pairs that cross the near plane, which are now rasterised, and nothing is dropped.
 * tests/mesh_clip_oracle.py restates the rule in numpy.  The rule is homogeneous rasterisation: no clip polygon is formed.
 *   pc_i and "in front" (pc_i,z > near) as above.  No corner in front: skipped.  All three in front: the pair goes through
 *   dqo_mesh_render_depth's statements UNCHANGED — a mesh that no used view crosses gives that entry's bytes.
 *   1 or 2 corners in front — the pair CROSSES (counted in [3], whatever follows):
 *       x_i, y_i of the corners in front as above (float32).
 *       box, in double from the widened floats, one rounding per operation: the points are (x_i, y_i) of the corners in front and, for
 *       each edge from a corner a in front to a corner b that is not, the edge's crossing of z = near,
 *           t = (near - z_a) / (z_b - z_a);  q_x = x_a + t * (x_b - x_a), q_y likewise (camera space);
 *           u = (q_x * fx) / near + cx;  v = (q_y * fy) / near + cy
 *       — with near == 0 a crossing lies at infinity: u is +inf or -inf by the sign of q_x, so the box opens to the image border on
 *       that side, or a NaN (q_x == 0), which is left out.  [ceil(min u) - 1, floor(max u) + 1] x [ceil(min v) - 1, floor(max v) + 1],
 *       comparisons that a NaN fails, the ends set to 0 and W - 1 (H - 1) where beyond; unless lo <= hi on both axes the pair is
 *       skipped.  (One pixel of margin: the float32 corners of a 2-D edge and the exact lines of the 3-D edges do not meet in one
 *       point.  The visible part of the face is the hull of these points, so the box holds every covered pixel.)
 *       orientation: A = (P_0,x * t_x + P_0,y * t_y) + P_0,z * t_z with t = P_1 x P_2, t_x = P_1,y * P_2,z - P_1,z * P_2,y and so on:
 *       the triple product P_0 . (P_1 x P_2), in double.  A repeated vertex id or A == 0: DEGENERATE, counted and skipped.
 *       edge between corners i and j, (p, q) the two ordered by vertex id: both in front — the 2-D edge function above, on the
 *       projected float32 corners; otherwise c = P_p x P_q (c_x = P_p,y * P_q,z - P_p,z * P_q,y, c_y = P_p,z * P_q,x - P_p,x * P_q,z,
 *       c_z = P_p,x * P_q,y - P_p,y * P_q,x), E = (c_x * r_x + c_y * r_y) + c_z with r the pixel's ray of the depth step; e_ij = E if p
 *       is i, else -E.  E is the 2-D form times z_p * z_q / (fx * fy): the two agree in sign on an edge in front (fx, fy > 0).  Both
 *       faces that share an edge see the same endpoints, pick the same form and compute bitwise opposite values.
 *       covered iff A > 0 and all three >= 0, or A < 0 and all three <= 0; depth, clamp and the test d > near && d <= depth_trunc as
 *       above — that test IS the clip: the part of the face's cone behind the near plane fails it.
 *   header: [2] counts the crossing pairs that have a box and are not degenerate too, [3] pairs that cross the near plane (clipped, not
 *   dropped), [5] by the box above for a crossing pair; the other words as above.
 *   The rasterise launch is the CLIP instantiation of dqo_mesh_render_depth's kernel; a crossing pair takes the same two paths (its own
 *   lane up to SMALL_MAX pixels of box, the whole wave above), and both paths call the one pixel function. */
int dqo_mesh_render_depth_clip(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                               int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy, float cx,
                               float cy, float near, float depth_trunc, float* depth, int32_t* face_index, int32_t* header, void* workspace,
                               size_t workspace_bytes, void* hipStream);

/* dqo_eval_depth_l1 (ABI 5, symbols-only addition) — Depth L1: two depth stacks compared pixel by pixel.  a (the truth) and b, float32
 * [n_views,H,W] in DEVICE memory, 0 = no hit (dqo_mesh_render_depth's, a Gaussian render's, a sensor's); view_keep as dqo_mesh_cull's;
 * depth_trunc > 0 (may be +inf).  A pixel is hit in a iff a > 0 && a <= depth_trunc, in b iff b > 0; VALID iff hit in both.
 * out_table float32 [n_views + 1][8]; row k of a used view:
 *     [0] l1_valid    the mean of |a - b| over the valid pixels
 *     [1] l1_image    the mean over all H * W pixels of |a' - b'|, a side without a hit taken as 0 (the NICE-SLAM form)
 *     [2] rmse_valid  the root of the mean of (a - b)^2 over the valid pixels
 *     [3] both  [4] only_a  [5] only_b  [6] neither     the pixels hit in both, in a alone, in b alone, in neither
 *     [7] max_abs     the largest |a - b| of the valid pixels (0 without one)
 * A view with both == 0 has NaN in the three means; an unused view is a row of NaN.  Row n_views: [0..2] the means of the used views'
 * values where they are defined (NaN without one), [3..6] the counts summed in double and rounded once, [7] the largest maximum.
 * Differences and sums are doubles added in a fixed order (see dqo_eval_picture; tests/depth_l1_oracle.py restates it): a table is
 * bitwise reproducible.  Two launches, no float atomic, no host read, no synchronise.  DQO_ERR_INVALID_ARG for n_views outside
 * [1, 65535], W * H not below 2^24 (a view's counts are exact float32), a NULL pointer, a depth_trunc that is not above 0; then
 * DQO_ERR_WORKSPACE.  workspace: dqo_eval_depth_l1_workspace_bytes(n_views, W, H), 0 for a bad size; ZERO when first used. */
size_t dqo_eval_depth_l1_workspace_bytes(int32_t n_views, int32_t W, int32_t H);
int dqo_eval_depth_l1(int32_t n_views, int32_t W, int32_t H, const float* a, const float* b, const uint8_t* view_keep, float depth_trunc,
                      float* out_table, void* workspace, size_t workspace_bytes, void* hipStream);

#define DQO_TICKET_WORDS (16 + 16 * 64) /* int32 words behind DqoAdamStep.block_ticket */
typedef struct DqoAdamStep {
    int32_t P, M;      /* Gaussians, SH coefficients per Gaussian (f_dc = coefficient 0, f_rest = the others) */
    int32_t step;      /* 1-based Adam step count */
    /* betas travel as floats; 1 - beta and beta^t are formed in double from the decimal the float was written as (rounded to seven
     * decimals: 0.9, 0.999 and every other short decimal come back exactly; a beta that is not a short decimal is used to seven
     * decimals — dqo_adam_multi takes doubles and has no such limit) */
    float beta1, beta2, eps;
    float lr_xyz, lr_f_dc, lr_f_rest, lr_opacity, lr_scaling, lr_rotation;
    float *xyz, *shs, *opacity_raw, *scaling_raw, *rotation_raw;            /* raw parameters, updated in place */
    const float *g_means3D, *g_sh, *g_opacity, *g_scales, *g_rotations;      /* dqo_rast_backward outputs (w.r.t. activated) */
    float *m_xyz, *m_shs, *m_opacity, *m_scaling, *m_rotation;               /* exp_avg, same shapes as the parameters */
    float *v_xyz, *v_shs, *v_opacity, *v_scaling, *v_rotation;               /* exp_avg_sq */
    /* Optional (NULL = skip): the activated values of the UPDATED parameters, exactly what dqo_map_activate would
     * compute from them — saves that launch in the next iteration. */
    float *act_opacity, *act_scales, *act_rotations;
    /* Optional (NULL = every gradient row is read): the forward's radii of this step.  Gradient rows of culled Gaussians
     * (radii == 0) are taken as zero without being read (pair with DqoRastGrads.skip_culled_rows); their parameters and
     * moments are still updated exactly as dense Adam does with a zero gradient. */
    const int32_t* radii;
    /* Optional (NULL = use `step`): device scalar holding the 1-based step count of THIS launch; the launch is followed
     * by a one-thread kernel that increments it.  With it a whole mapping iteration has no host-side per-iteration
     * argument and can be captured once in a hipGraph and replayed. */
    int32_t* step_dev;
    /* Optional (NULL = dense): one byte per Gaussian, 0 = both moment rows of the Gaussian are identically zero (the state of a
     * freshly built optimiser, which the reference builds per mapping call, mapper.py:548).  Such a Gaussian with no gradient
     * (radii == 0) is a fixed point of Adam — m, v stay 0 and p - step * 0 / (0 + eps) = p bit for bit — so its rows are neither
     * read nor written; the first update of the row sets its byte to 1.  Needs `radii`.  Results are identical to the dense update.
     * "No gradient" is radii == 0 and, where the backward's records are at hand (dqo_rast_backward_adam always; dqo_map_adam_step given
     * record_ctx below), also an in-view Gaussian for which the backward marked no partial record valid: the culling, the tile mask or
     * the object gate left it no list entry, or every entry sits behind an early exit, in another object's pixels or below 1/255, or
     * its pixels carry no incoming gradient — its record sums are exact zeros.  In-view members of the attach set are always updated. */
    uint8_t* moment_live;
    /* Optional (NULL = no such term): the attach loss of Mapping.loss_update (SLAM/multiprocess/mapper.py:812-829),
     *   1000 * (mse(_scaling[a], scaling0[a]) + mse(_xyz[a], xyz0[a]) + mse(_rotation[a], rotation0[a])),
     * a = Gaussians whose opacity at the start of the mapping call (init_stat, mapper.py:533-545) was below 0.9.  Its gradient is
     * elementwise on the RAW parameters and is added here, after the activation Jacobians: attach_mask [P] (1 = in a),
     * init_* = the raw parameters at the start of the call, attach_count = |a| (the means divide by 3 |a|, 3 |a|, 4 |a|).
     * attach_partial (optional, [ceil(P / 256)]): per-block sum of 1000 * (d_scaling^2 / (3|a|) + d_xyz^2 / (3|a|) + d_rot^2 /
     * (4|a|)) over the block's Gaussians at the PRE-update parameters — their sum is the reported "scale_loss" of this
     * iteration (fixed order, reproducible).  A Gaussian that has never moved contributes an exact zero, so the exact sparse
     * mode stays exact. */
    const uint8_t* attach_mask;
    const float *init_xyz, *init_scaling_raw, *init_rotation_raw;
    int32_t attach_count;
    float* attach_partial;
    /* Optional (NULL = always step): device header of the forward whose gradients this step consumes (start of ctx.geom).  If
     * its overflow flag is set — the frame was invalid: lists emptied, all gradients zero — the launch is a no-op: parameters,
     * moments, moment_live and the device step count stay as they were, so the caller can re-capture with a larger capacity and
     * continue from a clean optimiser state. */
    const DqoRastHeader* frame_header;
    /* Optional, with step_dev: DQO_TICKET_WORDS int32 (ABI 5; one word until ABI 4), zero before the first launch (they are zero again
     * after every launch).  The block that finishes last advances *step_dev inside the Adam launch itself — tickets are taken on up
     * to 64 lines and then on word 0, so that no single address is hit by every block; NULL = a separate one-thread kernel does it
     * afterwards. */
    int32_t* block_ticket;
    /* Optional, with step_dev and block_ticket (ABI 3): eight floats, zero before the first launch.  The bias corrections of a step
     * (two double-precision pow() calls + six divisions) are then computed ONCE per step — by the block that advances *step_dev, for the
     * step it advances to — instead of once per block of every launch; a launch whose step the table does not hold (the first one,
     * or after the caller rewrote *step_dev) computes them itself.  Same function either way: same bits. */
    float* bias_table;
    /* Optional (ABI 3): two device floats { 2000 / (3 |a|), 2000 / (4 |a|) } (computed in double, rounded to float), read when the
     * launch RUNS instead of deriving them from attach_count when it is issued — for a captured launch (hipGraph) whose attach set
     * changes between replays: the caller rewrites attach_mask, init_* and these two numbers in place at the start of a mapping call
     * and replays the same graph.  With it, the attach term is on whenever attach_mask is given (|a| = 0: write two zeros). */
    const float* attach_gains;
    /* ABI 5 — the reference trains ONE of its two clouds per mapping call while it renders both (local_optimize: pointcloud.parametrize,
     * SLAM/multiprocess/mapper.py:533; global_optimization: stable_pointcloud.parametrize, :1119).  Optional (NULL = every row trains):
     * one byte per Gaussian; a row with DQO_ROW_FROZEN set is no parameter of the optimiser: its gradient row is not formed, its
     * parameters, moments, moment_live byte and confidence stay bit for bit as they are, it is no member of the attach set whatever
     * attach_mask says.  Device memory, read when the launch runs (see DqoRastInputs.row_flags). */
    const uint8_t* row_flags;
    /* Optional (NULL = not counted): float [P], the reference's per-Gaussian confidence (SLAM/gaussian_pointcloud.py:42, :836).  A trained
     * row whose f_dc gradient of this step has a non-zero element gains 1 — Mapping.loss_update's
     *     grad_mask = (pointcloud._features_dc.grad.abs() != 0).any(dim=-1);  pointcloud._confidence[grad_mask] += 1   (mapper.py:908-910)
     * — inside the launch that consumes the gradient (the fused tail never writes the row to HBM).  An invalid frame counts nothing. */
    float* confidence;
    /* Optional (NULL = the six lr_* fields above): six device floats { xyz, f_dc, f_rest, opacity, scaling, rotation }, read when the
     * launch runs — global_optimization rescales the groups' learning rates per call (mapper.py:1120-1131: xyz 0, the others x 0.1 or
     * x their *_lr_coef); a caller that rewrites the table (and zeroes bias_table) between two mapping calls keeps its captured graph. */
    const float* lr_table;
    /* Optional, with moment_live (NULL = radii alone decides): the context of the forward / dqo_rast_backward call whose gradient rows
     * this step consumes, with that call's image size — read on the host when the launch is issued; its buffers must still hold the
     * frame.  dqo_map_adam_step then lists a row exactly as dqo_rast_backward_adam does (see moment_live): same rows touched, same
     * moment_live bytes.  Ignored by dqo_rast_backward_adam (it has its own ctx). */
    const DqoRastCtx* record_ctx;
    int32_t record_W, record_H;
} DqoAdamStep;
int dqo_map_adam_step(const DqoAdamStep*, void* hipStream);

/* Mapping.history_merge (SLAM/multiprocess/mapper.py:607-650), the statement that closes every local_optimize call: the trained cloud is
 * pulled back towards its state at the start of the call (`history_stat`, :535-545), weighted by how much of its confidence is old:
 *     w[i] = max_weight * conf0[i] / (conf[i] + 1e-6)
 *     xyz[i]      = xyz0[i] * w[i] + (1 - w[i]) * xyz[i]
 *     f_dc, f_rest, scaling: the same lerp with w[first_row] FOR EVERY ROW — the reference indexes `history_weight[0]` (:620-637), a [1]
 *                  tensor that broadcasts: the first Gaussian's weight serves the whole cloud (reproduced, not fixed)
 *     rotation[i] = slerp(rot0_unit[i], normalize(rotation[i]), 1 - w[i])     (SLAM/utils.py:650-709: |dot| > 0.9995 or NaN -> torch.lerp,
 *                  otherwise sin-weighted; no shortest-arc flip, no renormalisation) — the result replaces the RAW quaternion.
 * One launch in place of ~40 eager torch ops.  All tensors are updated in place; rot0_unit = the ACTIVATED (normalised) rotation at the
 * start of the call (`history_stat["rotation"]` = get_rotation), shs0 / shs are [P, M, 3] (coefficient 0 = f_dc, the rest f_rest).  rows:
 * optional row_flags (NULL = all rows): rows with DQO_ROW_FROZEN are left untouched (they belong to the cloud the call did not train);
 * first_row = the row whose weight serves the broadcast quirk (row 0 of the reference's trained cloud).  max_weight <= 0: no-op (:608-609). */
int dqo_map_history_merge(int32_t P, int32_t M, float max_weight, int32_t first_row, const uint8_t* row_flags, const float* conf0,
                          const float* conf, const float* xyz0, const float* shs0, const float* scaling0, const float* rot0_unit, float* xyz,
                          float* shs, float* scaling_raw, float* rotation_raw, void* hipStream);

/* Fused mapping iteration, backward half (ABI 3): the blend kernel of dqo_rast_backward followed by ONE kernel that, per block of 256
 * Gaussians, sums the per-instance gradient records, runs the per-Gaussian backward (rasterizer_impl.cu:445-564's K8 + K9,
 * backward.cu:273-548) and applies dqo_map_adam_step's update (SLAM/gaussian_pointcloud.py:331-378, SLAM/multiprocess/mapper.py:548,
 * 812-829) with the gradient rows held in LDS: neither the 59-float gradient rows nor the summed records reach HBM, two launches
 * fewer.  Parameters, moments, activations, moment_live and the device step count come out BIT-IDENTICAL to
 *     dqo_rast_backward(grads with skip_culled_rows = 1)  +  dqo_map_adam_step(step with radii = the forward's radii)
 * (same statements on the same operands).  Only step->attach_partial differs: here it must hold 4 * ceil(P / 256) floats — one
 * partial sum per wave of 64 Gaussians instead of one per block of 256 — whose total agrees with dqo_map_adam_step's to rounding.
 * `step`: the g_* and radii fields are not read (visibility comes from ctx); frame_header is taken from ctx (an overflowed frame is a
 * no-op, as in dqo_map_adam_step).  inputs->shs is required (precomputed colours have no Adam group) with params->M == step->M <= 16
 * and params->P == step->P.  workspace as for dqo_rast_backward.  With a loss tap in ctx, dL_dout_* may be NULL. */
int dqo_rast_backward_adam(const DqoRastParams*, const DqoRastInputs*, const DqoRastCtx*, const float* dL_dout_color,
                           const float* dL_dout_depth, const DqoAdamStep* step, void* workspace, size_t workspace_bytes,
                           void* hipStream);

/* dqo_window_bank_arm / dqo_window_bank_select (ABI 5, symbols-only addition) — the keyframe bank.  The final pass of the reference,
 * global_optimization(is_end=True) (SLAM/slam.py:183, SLAM/multiprocess/mapper.py:1143-1148, 1196-1199), trains over ALL keyframes with a
 * random keyframe per iteration.  A captured iteration reads everything per frame from device buffers (the DESTINATION below); a bank of
 * keyframes and a schedule in device memory plus ONE launch at the head of the iteration, which moves the scheduled keyframe into those
 * buffers, let one captured graph train over any number of keyframes with no host work per iteration.  csrc/map_window_bank.hip lists
 * the statements in order; tests/window_bank_oracle.py restates them.
 *   The bank: K_cap slots, a structure of arrays in caller-owned device memory, every part contiguous per slot.  gy = ceil(H/16),
 *     gx = ceil(W/16).
 *       camera        float32 [K_cap, 40]        bg[3], viewmatrix[16], projmatrix[16], campos[3], two pad floats
 *       gt_color      float32 [K_cap, 3, H, W]     gt_depth     float32 [K_cap, 1, H, W]
 *       render_mask   uint8   [K_cap, H, W]        tile_mask    int32   [K_cap, gy, gx]
 *       pixel_object  int32   [K_cap, H, W]        tile_objects int64   [K_cap, gy * gx]     (both NULL without an object gate)
 *   The destination: dst_bg [3], dst_viewmatrix [16], dst_projmatrix [16], dst_campos [3] (four pointers of their own), dst_gt_color,
 *     dst_gt_depth, dst_render_mask, dst_tile_mask, dst_pixel_object, dst_tile_objects: one slot's worth each.  The gate parts are given
 *     on both sides or on neither.
 *   The schedule: int32 [n][2] in device memory; entry (k, m) = camera, targets and gate of slot k under the render mask and tile mask
 *     of slot m (the pair of global_optimization's second half, mapper.py:1188-1195); a plain keyframe k is (k, k).  `lost`: int32 [n].
 *     `n` of the struct is the ENTRIES both lists hold; the length of the armed schedule is the state's word.
 *   The state: DQO_WINDOW_BANK_STATE_WORDS int32 of device memory: the ticket's DQO_TICKET_WORDS, then the words of the enum below, padded
 *     to a multiple of 256 bytes as every last-block head is.  dqo_window_bank_arm writes ALL of it (no zero fill needed before).
 *   dqo_window_bank_arm(state, n, stream): one small launch: cursor = 0, n, prev_k = prev_m = -1, force = 1, overrun = lost_count = 0, the
 *     ticket words zero.
 *   dqo_window_bank_select(args, stream): ONE launch, the same grid on every call, capturable.  Every block reads c = cursor, n, the
 *     previous pair and force.  Then
 *       c >= n, or c >= args.n             nothing is copied; overrun = 1; the cursor, the previous pair, force and the log stay
 *       (k, m) = schedule[c] with k or m outside [0, K_cap): nothing is copied; overrun = 2; the rest stays likewise
 *       otherwise   camera, gt_color, gt_depth, pixel_object, tile_objects from slot k  iff  force != 0 or k != prev_k;
 *                   render_mask, tile_mask from slot m                                  iff  force != 0 or m != prev_m;
 *                   if c > 0 and render_header (may be NULL; the device header of the context the graph renders on) has its overflow
 *                   word set (!= 0, as dqo_eval_picture and dqo_tsdf_integrate test it), the frame trained at position c - 1 was a no-op
 *                   for the optimiser (DqoAdamStep.frame_header): lost[lost_count] = c - 1, lost_count += 1;
 *                   then prev_k = k, prev_m = m, force = 0, cursor = c + 1.
 *     Copies are exact bytes and nothing outside the destinations' extents is written: 16-byte accesses where source and destination
 *     are both 16-byte aligned, 4-byte ones where both are 4-byte aligned, single bytes otherwise, and single bytes for what is left
 *     of a part whose length is no multiple of the access.  The state changes in the block that takes the launch's last ticket, after
 *     every block has read it.  Integer atomics on the ticket words only; no float arithmetic.
 *   DQO_ERR_INVALID_ARG before the launch: K_cap < 1, a bad image size, a NULL required pointer (everything but render_header and the
 *     gate parts), gate parts on one side only, n < 0; dqo_window_bank_arm: a NULL state, n < 0.  Calls that share a state must be
 *     ordered (one stream). */
enum {
    DQO_WINDOW_BANK_CURSOR = DQO_TICKET_WORDS + 0,     /* schedule position of the NEXT select */
    DQO_WINDOW_BANK_N = DQO_TICKET_WORDS + 1,          /* length of the armed schedule */
    DQO_WINDOW_BANK_PREV_K = DQO_TICKET_WORDS + 2,     /* the slots the destination holds: camera group / mask group (-1: none) */
    DQO_WINDOW_BANK_PREV_M = DQO_TICKET_WORDS + 3,
    DQO_WINDOW_BANK_FORCE = DQO_TICKET_WORDS + 4,      /* non-zero: copy even if unchanged; cleared by the launch that honours it */
    DQO_WINDOW_BANK_OVERRUN = DQO_TICKET_WORDS + 5,    /* 1: a select ran past the schedule; 2: a schedule entry names no slot */
    DQO_WINDOW_BANK_LOST_COUNT = DQO_TICKET_WORDS + 6, /* entries of `lost` */
    DQO_WINDOW_BANK_STATE_WORDS = DQO_TICKET_WORDS + 48
};
typedef struct DqoWindowBank {
    int32_t W, H, K_cap, n;
    const float *camera, *gt_color, *gt_depth;
    const uint8_t* render_mask;
    const int32_t* tile_mask;
    const int32_t* pixel_object;
    const int64_t* tile_objects;
    float *dst_bg, *dst_viewmatrix, *dst_projmatrix, *dst_campos, *dst_gt_color, *dst_gt_depth;
    uint8_t* dst_render_mask;
    int32_t* dst_tile_mask;
    int32_t* dst_pixel_object;
    int64_t* dst_tile_objects;
    const int32_t* schedule;
    int32_t* state;
    int32_t* lost;
    const DqoRastHeader* render_header;
} DqoWindowBank;
int dqo_window_bank_arm(int32_t* state, int32_t n, void* hipStream);
int dqo_window_bank_select(const DqoWindowBank*, void* hipStream);

/* dqo_traj_repose (ABI 5, symbols-only addition) — pose corrections.  Mapping.update_poses (SLAM/multiprocess/mapper.py:256-263; called
 * by slam.py:126-127 before every mapping() and by :181-182 before the final global_optimization) hands Camera.updatePose
 * (scene/cameras.py:165-183) the corrected world pose of every processed frame and keyframe; Tracker.save_traj (tracker.py:399-401)
 * replaces pose_es by the same set; metric.py:181, make_mesh.py:199 and metric_obj.py:212 run updatePose per dataset frame.  ONE launch,
 * capturable: nothing is read back, no memset, no atomics; the same bytes on every run.  csrc/map_repose.hip lists the statements in
 * order; tests/repose_oracle.py restates them.
 *   The store: pose [cap,16] double and header of dqo_traj_append's trajectory.  count = header[DQO_TRAJ_HEADER_COUNT], read on the
 *     device (clipped to [0, cap]).
 *   Pose part: new_pose, double [n_new,16] in device memory, indexed by trajectory row (new_poses[frame.uid] of the reference, the
 *     [N,4,4] stack of pose_es.npy).  pose[r] = new_pose[r] for every r < min(count, n_new, cap), as exact bytes.  Rows at or beyond n_new
 *     keep their pose (the reference would raise IndexError there).  pose_gt, flags, kf_metric and the header are not touched: the
 *     reference never re-tests a keyframe.  new_pose == NULL: poses unchanged, only the cameras are re-formed.
 *   Camera part: `targets`, T entries of DqoReposeTarget in device memory (48 bytes each, 8-byte aligned: an int64 [T,6] table): a
 *     trajectory row and up to five float32 destinations — c2w [16], w2c [16] (row-major: what dqo_mesh_cull / dqo_mesh_render_depth*
 *     take as a view), viewmatrix [16], projmatrix [16], campos [3]; a NULL destination skips that one.  Destinations are only
 *     guaranteed 4-byte aligned (a bank slot's viewmatrix starts at float 3 of a 160-byte camera row): every store is a 4-byte store and
 *     nothing outside the named extents is written.  A target's source pose is new_pose[row] when new_pose is given and row < n_new,
 *     otherwise pose[row]: the camera lanes never read a store row that the same launch is writing.  A target with row < 0 or
 *     row >= count writes nothing and is counted.  One lane per target in blocks of 256, doubles throughout, dqo_traj_append's camera
 *     statements and bits: c2w = the pose rounded once; w2c = the double inverse of the affine pose (by the cofactors of its 3x3 block)
 *     rounded once, viewmatrix its transpose; projmatrix = the double w2c transposed @ double(projection), rounded once (projection:
 *     device float32 [4,4], transposed as the reference keeps it); campos = the pose's translation (it follows the pose, where
 *     Camera.update keeps the constructor's centre).  Two targets may name one row; two targets must not share a destination.
 *   Bank state: bank_state non-NULL (a DqoWindowBank's state words): its DQO_WINDOW_BANK_FORCE word is set to 1 by one thread, so the
 *     next dqo_window_bank_select copies the camera group even when k == prev_k.  Graphs that read their camera tensors in place need
 *     no flag.  Calls that share a state must be ordered (one stream).
 *   stats: int32 [4], overwritten (may be NULL): pose rows rewritten, targets written, targets skipped for their row, 0.
 *   flags: DQO_REPOSE_HAS_PROJMATRIX when any target of the table has a projmatrix destination (the host cannot see a device table).
 * DQO_ERR_INVALID_ARG before the launch: NULL arguments, cap < 1, a NULL store or header, n_new < 0, T < 0, T > 0 with a NULL table,
 *   DQO_REPOSE_HAS_PROJMATRIX without a projection (without the flag and without a projection a projmatrix destination is skipped).
 * Not done: the world-frame maps of stored frames are not re-transformed (the reference's keymap_list keeps its normal_map too). */
enum { DQO_REPOSE_HAS_PROJMATRIX = 1 };
typedef struct DqoReposeTarget {
    int64_t row;
    float *c2w, *w2c, *viewmatrix, *projmatrix, *campos;
} DqoReposeTarget;
typedef struct DqoTrajRepose {
    int32_t cap, n_new, T, flags;
    double* pose;
    const int32_t* header;
    const double* new_pose;
    const DqoReposeTarget* targets;
    const float* projection;
    int32_t* bank_state;
    int32_t* stats;
} DqoTrajRepose;
int dqo_traj_repose(const DqoTrajRepose*, void* hipStream);

#ifdef __cplusplus
}
#endif
#endif /* DQO_RASTER_H_ */
