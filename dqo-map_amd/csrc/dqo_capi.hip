// extern "C" entry points of libdqoraster.so (declared in include/dqo_raster.h): argument validation, buffer-size
// queries and launches.  No allocation, no synchronisation (except dqo_rast_read_header), no exceptions.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "dqo_common.h"

static thread_local char g_err[512] = "";

void dqo_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int dqo_launch_mark_visible(int P, const float* means3D, const float* view, const float* proj, uint8_t* present, hipStream_t s);
int dqo_launch_knn3(int P, const float* xyz, float* mean_d2, int32_t* idx3, void* ws, size_t ws_bytes, hipStream_t s);
size_t dqo_knn3_ws_bytes(int P);
size_t dqo_knn3_query_ws_bytes(int Q, int R);
int dqo_launch_knn3_query(int Q, const float* q_xyz, int R, const float* r_xyz, float* dist2, int32_t* idx3, void* ws, size_t ws_bytes,
                          hipStream_t s, float bound2, const int32_t* q_group = nullptr, const int32_t* r_group = nullptr,
                          const float* group_box = nullptr);
int dqo_launch_quadric_iou(int B, const float* axes, const float* R, const float* center, const float* P34, const float* obs,
                           float* bbox, float* loss, int32_t* valid, float* g_axes, float* g_R, float* g_center, hipStream_t s);
int dqo_launch_objmap_frame(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* cat, int32_t* uid, int32_t* nviews,
                            float* view_P34, float* view_bbox, int32_t* state, int M, const float* det_bbox, const float* det_ellipse,
                            const int32_t* det_cat, const float* det_score, const float* depth, const float* K, const float* Rt, int W, int H,
                            int frame_id, uint64_t seed, int32_t* det_fate, int32_t* det_row, float* det_depth, uint8_t* opt_flag,
                            int32_t* frame_header, hipStream_t s);
int dqo_launch_objmap_optimize(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* uid, int32_t* nviews,
                               float* view_P34, float* view_bbox, int32_t* state, const uint8_t* opt_flag, int frame_id, uint64_t seed,
                               float* loss_hist, hipStream_t s);
int dqo_launch_objmap_mean_iou(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* nviews, float* view_P34,
                               float* view_bbox, int32_t* state, float* mean_iou, hipStream_t s);
int dqo_launch_quadric_adam(int n_obj, int n_iters, const int32_t* view_offset, const float* P34_views, const float* obs_views,
                            const int32_t* view_schedule, float* axes, float* R, float* center, float* loss_hist, hipStream_t s);

int dqo_launch_map_activate(int P, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, float* opacity,
                            float* scales, float* rotations, hipStream_t s);
size_t dqo_map_loss_ws_bytes(void);
int dqo_launch_map_loss(int W, int H, const float* color, const float* depth, const int32_t* depth_index, const float* gt_color,
                        const float* gt_depth, const uint8_t* render_mask, float color_weight, float depth_weight, float add_depth_thres,
                        float* loss_out, float* dL_dcolor, float* dL_ddepth, void* ws, hipStream_t s);
size_t dqo_map_ssim_ws_bytes(int W, int H);
int dqo_launch_map_ssim(int W, int H, const float* img, const float* gt, float weight, float* ssim_out, float* dL_dimg, int accumulate,
                        float* loss8, void* ws, hipStream_t s);
int dqo_launch_map_adam(const DqoAdamStep* st, hipStream_t s);
size_t dqo_map_attach_ws_bytes(int P);
int dqo_launch_adam_multi(const DqoAdamTensor* ts, int n_tensors, int step, double beta1, double beta2, double eps, hipStream_t s,
                          int32_t* step_dev = nullptr, int bump = 0);
int dqo_launch_history_merge(int P, int M, float max_weight, int first_row, const uint8_t* row_flags, const float* conf0, const float* conf,
                             const float* xyz0, const float* shs0, const float* scaling0, const float* rot0_unit, float* xyz, float* shs,
                             float* scaling_raw, float* rotation_raw, hipStream_t s);
int dqo_launch_map_attach(int P, const float* scaling, const float* xyz, const float* rotation, const float* scaling0, const float* xyz0,
                          const float* rotation0, const uint8_t* mask, int attach_count, float* loss, float* g_scaling, float* g_xyz,
                          float* g_rotation, void* ws, hipStream_t s);
int dqo_launch_backward_adam(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor,
                             const float* dL_ddepth, const DqoAdamStep* st, void* ws, hipStream_t s);
size_t dqo_icp_ws_bytes(void);
int dqo_launch_icp(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1, const float* pose10,
                   float fx, float fy, float cx, float cy, float dist_thr, float normal_thr, float* JtJ, float* JtR, int32_t* valid_count,
                   void* ws, hipStream_t s);
int dqo_launch_icp_gauss_newton(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1, float* pose10,
                                const float* K, float k_scale, float dist_thr, float normal_thr, float damping, int32_t* valid_count, void* ws,
                                hipStream_t s);
size_t dqo_track_preprocess_ws_bytes(int H, int W);
int dqo_launch_track_preprocess(int H, int W, const float* depth, const float* K, float min_depth, float max_depth,
                                float conf_thr, int filter, float* depth_out, float* vertex_out, float* normal_out, float* conf_out,
                                uint8_t* invalid_out, void* ws, hipStream_t s);
size_t dqo_track_pyramid_ws_bytes(void);
int64_t dqo_track_pyramid_pixel_count(int H, int W, int levels);
int dqo_launch_track_pyramid(int H, int W, int levels, const float* depth, const float* K, float* vertex, float* normal,
                             void* ws, hipStream_t s);
int dqo_launch_track_fill(int H, int W, float* render_depth, const float* frame_depth, const float* render_normal, const float* frame_normal,
                          float dist_thr, float normal_thr, hipStream_t s);
size_t dqo_track_p2p_ws_bytes(void);
int dqo_launch_track_p2p(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* pose10, float fail_thr,
                         const int32_t* valid_count, float* loss, int32_t* success, float* valid_ratio, void* ws, hipStream_t s);
int dqo_launch_tile_count(int W, int H, int mode, const uint8_t* mask_in, const float* T_map, uint8_t* mask_out, int32_t* tile_count,
                          int32_t* total, hipStream_t s);
int dqo_launch_tile_color_error(int W, int H, const float* render, const float* gt, float* err_px, float* tile_sum, hipStream_t s);
size_t dqo_window_masks_ws_bytes(int W, int H);
int dqo_launch_window_masks(int W, int H, int mode, const float* T_map, const float* render, const float* gt, float tile_mask_ratio, int k,
                            uint8_t* render_mask, int32_t* tile_mask, float* ratio_out, const DqoRastHeader* header, void* ws, hipStream_t s);
int dqo_launch_growth_scales(int n, const float* xyz, const int32_t* obj, const float* radius, const int32_t* i_new, const float* d2_old,
                             const int32_t* i_old, const float* extra_radius, float reach2, float min_radius, float max_radius, float* scales,
                             uint8_t* invalid, hipStream_t s);
int dqo_launch_growth_inside(int n, const float* d2, const int32_t* idx, const float* radius, uint8_t* inside, hipStream_t s);
int dqo_launch_error_maps(int64_t HW, const float* gt_color, const float* gt_depth, const float* render, const float* depth,
                          const int32_t* depth_index, const uint8_t* mask, float* color_err, float* depth_err, hipStream_t s);
size_t dqo_lifecycle_ws_bytes(int64_t P);
int dqo_launch_lifecycle_vote(const DqoLifecycle* a, const float* gt_color, const float* gt_depth, const float* render, const float* depth,
                              const int32_t* depth_index, const int32_t* color_index, hipStream_t s);
int dqo_launch_lifecycle_rows(const DqoLifecycle* a, hipStream_t s);
size_t dqo_sample_ws_bytes(int64_t HW);
int dqo_launch_growth_sample(const DqoGrowthSample* a, hipStream_t s);
size_t dqo_nn1_ws_bytes(int Q, int R);
int dqo_launch_nn1(int Q, const float* q_xyz, const uint8_t* q_keep, int R, const float* r_xyz, const uint8_t* r_keep, const float* q_xform,
                   const float* r_xform, float* dist2, int32_t* idx, void* ws, hipStream_t s);
size_t dqo_eval_pcd_ws_bytes(int n_gt, int n_rec);
int dqo_launch_eval_pcd(int n_gt, const float* gt_xyz, const uint8_t* gt_keep, int n_rec, const float* rec_xyz, const uint8_t* rec_keep,
                        const float* rec_xform, int n_thres, const float* thres, float* out_row, void* ws, hipStream_t s);
size_t dqo_densify_ws_bytes(uint64_t total);
int dqo_launch_surfel_densify(int P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const uint8_t* row_keep,
                              int circle_num, int levels, int sigma, const float* circle_cs, int frame, uint64_t seed, int64_t cap,
                              float* points, float* normals, int64_t* index, uint8_t* keep, int32_t* header, void* ws, hipStream_t s);
size_t dqo_mesh_sample_ws_bytes(int64_t F);
int dqo_launch_mesh_sample(int V, const float* vertices, int F, const int32_t* faces, int count, uint64_t seed, float* points,
                           int32_t* face_index, uint8_t* keep, int32_t* header, void* ws, hipStream_t s);
size_t dqo_eval_ws_bytes(int64_t HW);
size_t dqo_msssim_ws_bytes(int W, int H);
int dqo_launch_msssim(int W, int H, const float* render, const float* gt_color, const DqoRastHeader* header, float* out_row, void* ws,
                      hipStream_t s);
int dqo_launch_eval_picture(int W, int H, const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                            const int32_t* depth_index, float min_depth, float max_depth, const DqoRastHeader* header, float* out_row,
                            void* ws, hipStream_t s);
size_t dqo_map_pack_ws_bytes(int64_t P);
int dqo_launch_map_pack(int P, int M, int with_conf, const float* xyz, const float* shs, const float* opacity_raw, const float* scaling_raw,
                        const float* rotation_raw, const float* confidence, const uint8_t* alive, const uint8_t* stable, float* table,
                        int32_t* header, void* ws, hipStream_t s);
int dqo_launch_map_unpack(int M, int64_t n, int64_t first_row, int has_conf, const float* table, float* xyz, float* shs, float* opacity_raw,
                          float* scaling_raw, float* rotation_raw, float* confidence, hipStream_t s);
int dqo_launch_attach_pixels(int n, const float* xyz, const float* V, float fx, float fy, float cx, float cy, int W, int H,
                             const int32_t* pixel_object, int32_t* lin, int32_t* sparse, unsigned long long* tile_objects, hipStream_t s);
int dqo_launch_attach_decide(int n, const float* xyz, const float* opacity, const int32_t* obj, const int32_t* lin, const int32_t* hit_index,
                             const float* hit_weight, const float* sxyz, const float* scaling_raw, const float* rotation_raw,
                             const int32_t* gobj, float plane_thr, float opacity_low, uint8_t* out, hipStream_t s);
int dqo_launch_tap_report(const DqoGeomLayout& g, const DqoTapDev& tap, hipStream_t s);
int dqo_launch_accumulate_confidence(int H, int W, int P, const int32_t* index, const float* confidence, float* gmax, float* gmin,
                                     float* gmean, int32_t* counter, hipStream_t s);
int dqo_launch_accumulate_error(int H, int W, int P, const float* color_err, const float* depth_err, const float* normal_err,
                                const int32_t* color_index, const int32_t* depth_index, float color_thr, float depth_thr,
                                float normal_thr, int check_max, float* gs_color, float* gs_depth, float* gs_normal, float* rescale,
                                int32_t* counters, hipStream_t s);

// ---- per-kernel timing with HIP events on the launch stream (bench.py's roofline leg) -------------------------------
#include <map>
#include <mutex>
#include <string>
#include <vector>
int g_dqo_profile_on = 0;
namespace {
std::mutex g_profile_mu;  // the timing tables are process-wide: launches may come from several host threads (one per stream)
struct Pending {
    std::string name;
    hipEvent_t start, stop;
};
std::vector<Pending> g_pending;
std::vector<hipEvent_t> g_event_pool;
std::map<std::string, std::pair<double, uint32_t>> g_profile_acc;
hipEvent_t take_event() {
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace
// before / after bracket ONE launch of the calling thread: the index of its pending entry is kept per thread, so brackets of
// different threads may interleave
static thread_local size_t t_pending_idx = 0;
void dqo_profile_before(const char* name, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_profile_mu);
    Pending p{name, take_event(), take_event()};
    (void)hipEventRecord(p.start, s);
    t_pending_idx = g_pending.size();
    g_pending.push_back(p);
}
void dqo_profile_after(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_profile_mu);
    if (t_pending_idx < g_pending.size()) (void)hipEventRecord(g_pending[t_pending_idx].stop, s);
}

extern "C" {

#define DQO_API __attribute__((visibility("default")))

DQO_API int dqo_profile_enable(int on) {
    g_dqo_profile_on = on ? 1 : 0;
    return DQO_OK;
}

// Waits for every bracketed launch recorded so far, accumulates elapsed times per kernel name and copies up to
// max_entries accumulated rows out (returns the number of rows).  reset != 0 clears the accumulators afterwards.
DQO_API int dqo_profile_collect(DqoProfileEntry* out, int max_entries, int reset) {
    std::lock_guard<std::mutex> lk(g_profile_mu);
    for (auto& p : g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.stop) == hipSuccess && hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
            auto& a = g_profile_acc[p.name];
            a.first += ms;
            a.second += 1;
        }
        g_event_pool.push_back(p.start);
        g_event_pool.push_back(p.stop);
    }
    g_pending.clear();
    int n = 0;
    for (auto& kv : g_profile_acc) {
        if (n >= max_entries || out == nullptr) break;
        strncpy(out[n].name, kv.first.c_str(), sizeof(out[n].name) - 1);
        out[n].name[sizeof(out[n].name) - 1] = 0;
        out[n].total_ms = kv.second.first;
        out[n].calls = kv.second.second;
        n++;
    }
    if (reset) g_profile_acc.clear();
    return n;
}

DQO_API int dqo_abi_version(void) { return DQO_ABI_VERSION; }
DQO_API size_t dqo_abi_sizeof(int32_t which) {
    static const size_t sz[] = {sizeof(DqoRastParams), sizeof(DqoRastInputs), sizeof(DqoRastOutputs), sizeof(DqoRastCtx), sizeof(DqoRastGrads),
                                sizeof(DqoRastHeader), sizeof(DqoProfileEntry), sizeof(DqoAdamStep), sizeof(DqoLossTap), sizeof(DqoObjectGate),
                                sizeof(DqoAdamTensor), sizeof(DqoRastParamInputs), sizeof(DqoRastParamGrads), 0 /* 13: unused */,
                                sizeof(DqoLifecycle), sizeof(DqoGrowthSample)};
    return (which >= 0 && which < (int32_t)(sizeof(sz) / sizeof(sz[0]))) ? sz[which] : 0;
}
DQO_API const char* dqo_last_error(void) { return g_err; }

DQO_API size_t dqo_rast_geom_bytes(int32_t P, int32_t W, int32_t H) {
    (void)W;
    (void)H;
    return dqo_geom_layout(nullptr, P < 0 ? 0 : P).total;
}
DQO_API size_t dqo_rast_image_bytes(int32_t W, int32_t H) { return dqo_image_layout(nullptr, W, H).total; }
DQO_API size_t dqo_rast_binning_bytes(int64_t cap) { return dqo_bin_layout(nullptr, cap < 0 ? 0 : cap, cap < 0 ? 0 : cap, 0).total; }
DQO_API size_t dqo_rast_binning_bytes_bucketed(int64_t cap, int32_t W, int32_t H, int32_t bucket) {
    if (cap < 0) cap = 0;
    if (bucket <= 0 || W <= 0 || H <= 0) return dqo_rast_binning_bytes(cap);
    return dqo_bin_layout(nullptr, cap, dqo_list_cap(cap, W, H, bucket), bucket).total;
}
DQO_API size_t dqo_rast_backward_workspace_bytes(int64_t cap) { return dqo_bwd_ws_bytes(cap); }

static int check_common(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx) {
    DQO_CHECK_ARG(p && in && ctx, "null params / inputs / ctx");
    DQO_CHECK_ARG(p->P >= 0 && p->W > 0 && p->H > 0, "bad sizes P=%d W=%d H=%d", p->P, p->W, p->H);
    DQO_CHECK_ARG(p->D >= 0 && p->D <= 3, "sh degree %d out of range 0..3", p->D);
    DQO_CHECK_ARG((p->W + DQO_TILE - 1) / DQO_TILE < 65536 && (p->H + DQO_TILE - 1) / DQO_TILE < 65536, "image too large");
    DQO_CHECK_ARG(in->viewmatrix && in->projmatrix && in->campos && in->bg, "viewmatrix/projmatrix/campos/bg must be given");
    if (p->P > 0) {
        DQO_CHECK_ARG(in->means3D && in->opacities, "means3D / opacities missing");
        DQO_CHECK_ARG((in->shs != nullptr) != (in->colors_precomp != nullptr),
                      "Please provide excatly one of either SHs or precomputed colors!");
        DQO_CHECK_ARG(in->cov3D_precomp == nullptr,
                      "cov3D_precomp is not supported by the depth rasteriser: its blend kernel reads scales/rotations (forward.cu:780)");
        DQO_CHECK_ARG(in->scales && in->rotations, "scales and rotations are required");
        if (in->shs) DQO_CHECK_ARG(p->M >= (p->D + 1) * (p->D + 1), "sh has %d coefficients, degree %d needs %d", p->M, p->D, (p->D + 1) * (p->D + 1));
        if (in->colors_precomp == nullptr && p->M == 0) {
            // rasterizer_impl.cu:267-270 analogue
            dqo_set_error("For non-RGB, provide precomputed Gaussian colors!");
            return DQO_ERR_INVALID_ARG;
        }
    }
    DQO_CHECK_ARG(ctx->geom && ctx->geom_bytes >= dqo_rast_geom_bytes(p->P, p->W, p->H), "geom buffer too small (%zu < %zu)",
                  ctx->geom_bytes, dqo_rast_geom_bytes(p->P, p->W, p->H));
    DQO_CHECK_ARG(ctx->image && ctx->image_bytes >= dqo_rast_image_bytes(p->W, p->H), "image buffer too small (%zu < %zu)",
                  ctx->image_bytes, dqo_rast_image_bytes(p->W, p->H));
    return DQO_OK;
}

static int check_outputs(const DqoRastParams* p, const DqoRastOutputs* o) {
    DQO_CHECK_ARG(o, "null outputs");
    DQO_CHECK_ARG(o->out_color && o->out_depth && o->out_hit_color && o->out_hit_depth && o->out_hit_color_weight &&
                      o->out_hit_depth_weight && o->out_T,
                  "null image output");
    if (p->P > 0) DQO_CHECK_ARG(o->n_touched && o->radii, "null n_touched / radii");
    return DQO_OK;
}

DQO_API int dqo_rast_forward_prepare(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx, void* stream) {
    int rc = check_common(p, in, ctx);
    if (rc) return rc;
    rc = check_outputs(p, out);
    if (rc) return rc;
    rc = dqo_launch_forward_prepare(p, in, out, ctx, (hipStream_t)stream);
    if (rc) return rc;
    return dqo_launch_mark_header_stage0(p, ctx, (hipStream_t)stream);  // (a no-op unless the frame's first stage is fused into its second)
}

DQO_API int dqo_rast_read_header(const DqoRastCtx* ctx, DqoRastHeader* host_out, void* stream) {
    DQO_CHECK_ARG(ctx && ctx->geom && host_out, "null ctx / out");
    static thread_local uint32_t buf[128 + 64 * DQO_SPREAD];  // header | counters | spread statistics counters
    DQO_CHECK_HIP(hipMemcpyAsync(buf, ctx->geom, sizeof(buf), hipMemcpyDeviceToHost, (hipStream_t)stream));
    DQO_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    memcpy(host_out, buf, sizeof(DqoRastHeader));
    // Stage 2 has written the frame's header (tile_scan_kernel / the sort kernel's header_from_spread): report it as it is.  The
    // counters and statistics lines it was formed from are NOT a second source: bucket mode allocates slots per region (counters[0]
    // stays 0) and dqo_rast_backward_adam's tail clears them for the next frame.
    if (host_out->stage == 2u) return host_out->overflow ? DQO_ERR_OVERFLOW : DQO_OK;
    // after `prepare` only the statistics lines are valid: visible Gaussians and the candidate count (>= N) a caller sizes its
    // binning buffer from; everything else is not known yet
    uint32_t nv = 0, nc = 0;
    for (int j = 0; j < DQO_SPREAD; j++) nv += buf[128 + 64 * j], nc += buf[128 + 64 * j + 1];
    memset(host_out, 0, sizeof(*host_out));
    host_out->stage = 1u;
    host_out->num_visible = nv;
    host_out->num_candidates = nc;
    return host_out->overflow ? DQO_ERR_OVERFLOW : DQO_OK;
}

static int check_render(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx) {
    int rc = check_common(p, in, ctx);
    if (rc) return rc;
    rc = check_outputs(p, out);
    if (rc) return rc;
    DQO_CHECK_ARG(ctx->inst_capacity >= 0 && ctx->inst_capacity < (int64_t)0xffffffffll, "bad inst_capacity");
    DQO_CHECK_ARG(ctx->inst_capacity == 0 || ctx->binning, "null binning buffer");
    DQO_CHECK_ARG(ctx->tile_bucket_capacity >= 0, "negative tile_bucket_capacity");
    DQO_CHECK_ARG(ctx->loss_tap == nullptr || (ctx->loss_tap->gt_color && ctx->loss_tap->gt_depth && ctx->loss_tap->loss_out &&
                                               ctx->loss_tap->grad_scale), "loss tap with a null pointer");
    DQO_CHECK_ARG(ctx->object_gate == nullptr || (ctx->object_gate->gaussian_object && ctx->object_gate->pixel_object),
                  "object gate with a null pointer");
    DQO_CHECK_ARG(ctx->loss_tap == nullptr || !ctx->loss_tap->per_object || ctx->object_gate, "a per-object loss tap needs the object gate");
    if (ctx->binning_bytes < dqo_rast_binning_bytes_bucketed(ctx->inst_capacity, p->W, p->H, ctx->tile_bucket_capacity)) {
        dqo_set_error("binning buffer too small (%zu < %zu)", ctx->binning_bytes,
                      dqo_rast_binning_bytes_bucketed(ctx->inst_capacity, p->W, p->H, ctx->tile_bucket_capacity));
        return DQO_ERR_WORKSPACE;
    }
    return DQO_OK;
}

DQO_API int dqo_rast_forward_render(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx, void* stream) {
    const int rc = check_render(p, in, out, ctx);
    if (rc) return rc;
    return dqo_launch_forward_render(p, in, out, ctx, (hipStream_t)stream);
}

DQO_API int dqo_rast_forward(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx, void* stream) {
    int rc = check_render(p, in, out, ctx);  // (covers the checks of the first stage)
    if (rc) return rc;
    rc = dqo_launch_forward_prepare(p, in, out, ctx, (hipStream_t)stream);
    if (rc) return rc;
    return dqo_launch_forward_render(p, in, out, ctx, (hipStream_t)stream);
}

DQO_API int dqo_rast_forward_async(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx,
                                   DqoRastHeader* header_host, void* header_event, void* stream) {
    int rc = check_render(p, in, out, ctx);  // (covers the checks of the first stage)
    if (rc) return rc;
    rc = dqo_launch_forward_prepare(p, in, out, ctx, (hipStream_t)stream);
    if (rc) return rc;
    return dqo_launch_forward_render(p, in, out, ctx, (hipStream_t)stream, header_host, (hipEvent_t)header_event);
}

// dqo_rast_backward and dqo_rast_backward_params (pf: the parameter form's coefficients 1.., dL_drest their gradient rows)
static int rast_backward(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor, const float* dL_ddepth,
                         const int32_t* hit_image, DqoRastGrads* g, void* ws, size_t ws_bytes, hipStream_t stream, const DqoShRest* pf,
                         float* dL_drest) {
    int rc = check_common(p, in, ctx);
    if (rc) return rc;
    DQO_CHECK_ARG(g, "null grads");
    if (p->P == 0) {  // rasterize_points.cu:208 (with a loss tap the loss of the background-only frame is still reported)
        if (ctx->loss_tap == nullptr) return DQO_OK;
        return dqo_launch_tap_report(dqo_geom_layout(ctx->geom, 0), dqo_tap_dev(ctx->loss_tap), (hipStream_t)stream);
    }
    DQO_CHECK_ARG((dL_dcolor && dL_ddepth) || ctx->loss_tap, "null upstream gradients");
    DQO_CHECK_ARG(ctx->loss_tap == nullptr || (ctx->loss_tap->gt_color && ctx->loss_tap->gt_depth && ctx->loss_tap->out_color &&
                                               ctx->loss_tap->out_depth && ctx->loss_tap->loss_out && ctx->loss_tap->grad_scale),
                  "loss tap with a null pointer");
    DQO_CHECK_ARG(g->dL_dmeans3D && g->dL_dopacity && g->dL_dscales && g->dL_drotations, "null gradient output");
    DQO_CHECK_ARG(p->M == 0 || g->dL_dsh, "null dL_dsh");
    DQO_CHECK_ARG(ctx->binning || ctx->inst_capacity == 0, "null binning buffer");
    if (ws_bytes < dqo_rast_backward_workspace_bytes(ctx->inst_capacity) || (ws == nullptr && ctx->inst_capacity > 0)) {
        dqo_set_error("backward workspace too small (%zu < %zu)", ws_bytes, dqo_rast_backward_workspace_bytes(ctx->inst_capacity));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_backward(p, in, ctx, dL_dcolor, dL_ddepth, hit_image, g, ws, ws_bytes, stream, pf, dL_drest);
}

DQO_API int dqo_rast_backward(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor,
                              const float* dL_ddepth, const int32_t* hit_image, DqoRastGrads* g, void* ws, size_t ws_bytes, void* stream) {
    return rast_backward(p, in, ctx, dL_dcolor, dL_ddepth, hit_image, g, ws, ws_bytes, (hipStream_t)stream, nullptr, nullptr);
}

// ---- the parameter form (DqoRastParamInputs / DqoRastParamGrads) ----
// Checks what is particular to the form and builds the DqoRastInputs / DqoRastParams the launchers take: the raw tensors in the
// activated tensors' places (the kernels' PF instantiations read them as such), M = 1 + rest.  The common checks follow on those.
static int pf_inputs(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastParamInputs* pin, DqoRastParams* p2, DqoRastInputs* in2,
                     DqoShRest* rest) {
    DQO_CHECK_ARG(p && in && pin, "null params / inputs / parameter inputs");
    DQO_CHECK_ARG(in->shs == nullptr && in->opacities == nullptr && in->scales == nullptr && in->rotations == nullptr,
                  "parameter form: DqoRastInputs.shs / opacities / scales / rotations must be NULL (they come from DqoRastParamInputs)");
    DQO_CHECK_ARG(in->colors_precomp == nullptr, "parameter form: colors_precomp is not supported");
    DQO_CHECK_ARG(pin->rest >= 0, "parameter form: negative rest coefficient count %d", pin->rest);
    DQO_CHECK_ARG(p->M == 1 + pin->rest, "parameter form: params M = %d, must be 1 + rest = %d", p->M, 1 + pin->rest);
    DQO_CHECK_ARG(p->D < 0 || p->D > 3 || 1 + pin->rest >= (p->D + 1) * (p->D + 1),
                  "parameter form: features_rest has %d coefficients, degree %d needs %d", pin->rest, p->D, (p->D + 1) * (p->D + 1) - 1);
    if (p->P > 0) {
        DQO_CHECK_ARG(pin->features_dc && pin->opacity_raw && pin->scaling_raw && pin->rotation_raw, "parameter form: null raw parameter");
        DQO_CHECK_ARG(pin->rest == 0 || pin->features_rest, "parameter form: null features_rest with rest = %d", pin->rest);
    }
    *p2 = *p;
    *in2 = *in;
    in2->shs = pin->features_dc, in2->opacities = pin->opacity_raw, in2->scales = pin->scaling_raw, in2->rotations = pin->rotation_raw;
    rest->rest = pin->features_rest, rest->m_rest = pin->rest;
    return DQO_OK;
}

DQO_API int dqo_rast_forward_prepare_params(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastParamInputs* pin, DqoRastOutputs* out,
                                            DqoRastCtx* ctx, void* stream) {
    DqoRastParams p2;
    DqoRastInputs in2;
    DqoShRest rest;
    int rc = pf_inputs(p, in, pin, &p2, &in2, &rest);
    if (rc) return rc;
    rc = check_common(&p2, &in2, ctx);
    if (rc) return rc;
    rc = check_outputs(&p2, out);
    if (rc) return rc;
    rc = dqo_launch_forward_prepare(&p2, &in2, out, ctx, (hipStream_t)stream, &rest);
    if (rc) return rc;
    return dqo_launch_mark_header_stage0(&p2, ctx, (hipStream_t)stream);
}

DQO_API int dqo_rast_forward_render_params(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastParamInputs* pin, DqoRastOutputs* out,
                                           DqoRastCtx* ctx, void* stream) {
    DqoRastParams p2;
    DqoRastInputs in2;
    DqoShRest rest;
    int rc = pf_inputs(p, in, pin, &p2, &in2, &rest);
    if (rc) return rc;
    rc = check_render(&p2, &in2, out, ctx);
    if (rc) return rc;
    return dqo_launch_forward_render(&p2, &in2, out, ctx, (hipStream_t)stream, nullptr, nullptr, &rest);
}

DQO_API int dqo_rast_forward_async_params(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastParamInputs* pin, DqoRastOutputs* out,
                                          DqoRastCtx* ctx, DqoRastHeader* header_host, void* header_event, void* stream) {
    DqoRastParams p2;
    DqoRastInputs in2;
    DqoShRest rest;
    int rc = pf_inputs(p, in, pin, &p2, &in2, &rest);
    if (rc) return rc;
    rc = check_render(&p2, &in2, out, ctx);  // (covers the checks of the first stage)
    if (rc) return rc;
    rc = dqo_launch_forward_prepare(&p2, &in2, out, ctx, (hipStream_t)stream, &rest);
    if (rc) return rc;
    return dqo_launch_forward_render(&p2, &in2, out, ctx, (hipStream_t)stream, header_host, (hipEvent_t)header_event, &rest);
}

DQO_API int dqo_rast_backward_params(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastParamInputs* pin, const DqoRastCtx* ctx,
                                     const float* dL_dcolor, const float* dL_ddepth, const int32_t* hit_image, DqoRastGrads* g,
                                     DqoRastParamGrads* pg, void* ws, size_t ws_bytes, void* stream) {
    DqoRastParams p2;
    DqoRastInputs in2;
    DqoShRest rest;
    int rc = pf_inputs(p, in, pin, &p2, &in2, &rest);
    if (rc) return rc;
    DQO_CHECK_ARG(g && pg, "null grads / parameter grads");
    DQO_CHECK_ARG(g->dL_dsh == nullptr && g->dL_dopacity == nullptr && g->dL_dscales == nullptr && g->dL_drotations == nullptr &&
                      g->dL_dcolors == nullptr,
                  "parameter form: DqoRastGrads.dL_dsh / dL_dopacity / dL_dscales / dL_drotations / dL_dcolors must be NULL "
                  "(DqoRastParamGrads holds them)");
    if (p2.P > 0) {
        DQO_CHECK_ARG(pg->dL_dfeatures_dc && pg->dL_dopacity_raw && pg->dL_dscaling_raw && pg->dL_drotation_raw,
                      "parameter form: null raw gradient output");
        DQO_CHECK_ARG(pin->rest == 0 || pg->dL_dfeatures_rest, "parameter form: null dL_dfeatures_rest with rest = %d", pin->rest);
    }
    // the kernels' rows: the activated form's fields carry the raw gradients (gaussian_rows_kernel<true> applies the Jacobians)
    DqoRastGrads g2 = *g;
    g2.dL_dsh = pg->dL_dfeatures_dc, g2.dL_dopacity = pg->dL_dopacity_raw, g2.dL_dscales = pg->dL_dscaling_raw;
    g2.dL_drotations = pg->dL_drotation_raw;
    return rast_backward(&p2, &in2, ctx, dL_dcolor, dL_ddepth, hit_image, &g2, ws, ws_bytes, (hipStream_t)stream, &rest, pg->dL_dfeatures_rest);
}

static int check_adam_step(const DqoAdamStep* st, bool need_grads) {
    DQO_CHECK_ARG(st, "null step");
    DQO_CHECK_ARG(st->P >= 0 && st->M >= 1 && (st->step >= 1 || st->step_dev != nullptr), "bad P / M / step");
    if (st->P == 0) return DQO_OK;
    DQO_CHECK_ARG(st->xyz && st->shs && st->opacity_raw && st->scaling_raw && st->rotation_raw, "null parameter");
    if (need_grads) DQO_CHECK_ARG(st->g_means3D && st->g_sh && st->g_opacity && st->g_scales && st->g_rotations, "null gradient");
    DQO_CHECK_ARG(st->m_xyz && st->m_shs && st->m_opacity && st->m_scaling && st->m_rotation && st->v_xyz && st->v_shs &&
                      st->v_opacity && st->v_scaling && st->v_rotation,
                  "null optimiser state");
    return DQO_OK;
}

DQO_API int dqo_rast_backward_adam(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor,
                                   const float* dL_ddepth, const DqoAdamStep* st, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(p, in, ctx);
    if (rc) return rc;
    rc = check_adam_step(st, false);
    if (rc) return rc;
    DQO_CHECK_ARG(st->P == p->P && st->M == p->M, "step is for P=%d M=%d, the rasteriser call for P=%d M=%d", st->P, st->M, p->P, p->M);
    if (p->P == 0) {
        if (ctx->loss_tap == nullptr) return DQO_OK;
        return dqo_launch_tap_report(dqo_geom_layout(ctx->geom, 0), dqo_tap_dev(ctx->loss_tap), (hipStream_t)stream);
    }
    DQO_CHECK_ARG(in->shs != nullptr, "the fused backward + Adam step needs SH colours (precomputed colours have no parameter group)");
    DQO_CHECK_ARG(p->M <= 16, "the fused backward + Adam step holds gradient rows of at most 16 SH coefficients (M = %d)", p->M);
    DQO_CHECK_ARG((dL_dcolor && dL_ddepth) || ctx->loss_tap, "null upstream gradients");
    DQO_CHECK_ARG(ctx->loss_tap == nullptr || (ctx->loss_tap->gt_color && ctx->loss_tap->gt_depth && ctx->loss_tap->out_color &&
                                               ctx->loss_tap->out_depth && ctx->loss_tap->loss_out && ctx->loss_tap->grad_scale),
                  "loss tap with a null pointer");
    DQO_CHECK_ARG(ctx->binning || ctx->inst_capacity == 0, "null binning buffer");
    if (ws_bytes < dqo_rast_backward_workspace_bytes(ctx->inst_capacity) || (ws == nullptr && ctx->inst_capacity > 0)) {
        dqo_set_error("backward workspace too small (%zu < %zu)", ws_bytes, dqo_rast_backward_workspace_bytes(ctx->inst_capacity));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_backward_adam(p, in, ctx, dL_dcolor, dL_ddepth, st, ws, (hipStream_t)stream);
}

DQO_API int dqo_mark_visible(int32_t P, const float* means3D, const float* view, const float* proj, uint8_t* present, void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(means3D && view && proj && present, "null pointer");
    return dqo_launch_mark_visible(P, means3D, view, proj, present, (hipStream_t)stream);
}

DQO_API size_t dqo_knn3_query_workspace_bytes(int32_t Q, int32_t R) { return dqo_knn3_query_ws_bytes(Q < 1 ? 1 : Q, R < 1 ? 1 : R); }

static int knn3_query(int32_t Q, const float* q_xyz, int32_t R, const float* r_xyz, float max_dist, float* dist2, int32_t* idx3, void* ws,
                      size_t ws_bytes, void* stream, const int32_t* q_group = nullptr, const int32_t* r_group = nullptr,
                      const float* group_box = nullptr) {
    DQO_CHECK_ARG(Q >= 0 && R >= 0, "negative size");
    DQO_CHECK_ARG(max_dist > 0.f, "max_dist must be positive");
    if (Q == 0) return DQO_OK;
    DQO_CHECK_ARG(q_xyz && dist2 && idx3, "null query / output");
    DQO_CHECK_ARG(R > 0 && r_xyz, "empty reference set");
    if (ws == nullptr || ws_bytes < dqo_knn3_query_ws_bytes(Q, R)) {
        dqo_set_error("knn query workspace too small (%zu < %zu)", ws_bytes, dqo_knn3_query_ws_bytes(Q, R));
        return DQO_ERR_WORKSPACE;
    }
    const float bound2 = max_dist < 1.8e19f ? max_dist * max_dist : 3.402823466e+38f;
    return dqo_launch_knn3_query(Q, q_xyz, R, r_xyz, dist2, idx3, ws, ws_bytes, (hipStream_t)stream, bound2, q_group, r_group, group_box);
}

DQO_API int dqo_knn3_query(int32_t Q, const float* q_xyz, int32_t R, const float* r_xyz, float* dist2, int32_t* idx3, void* ws, size_t ws_bytes,
                           void* stream) {
    return knn3_query(Q, q_xyz, R, r_xyz, 3.402823466e+38f, dist2, idx3, ws, ws_bytes, stream);
}

DQO_API int dqo_knn3_query_within(int32_t Q, const float* q_xyz, int32_t R, const float* r_xyz, float max_dist, float* dist2, int32_t* idx3,
                                  void* ws, size_t ws_bytes, void* stream) {
    return knn3_query(Q, q_xyz, R, r_xyz, max_dist, dist2, idx3, ws, ws_bytes, stream);
}

DQO_API int dqo_knn3_query_grouped(int32_t Q, const float* q_xyz, const int32_t* q_group, int32_t R, const float* r_xyz, const int32_t* r_group,
                                   const float* group_box, float max_dist, float* dist2, int32_t* idx3, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(Q == 0 || (q_group && r_group), "null group ids");
    DQO_CHECK_ARG(R < (1 << 25), "the grouped search carries the group id in the index word: at most 2^25 - 1 reference points");
    return knn3_query(Q, q_xyz, R, r_xyz, max_dist, dist2, idx3, ws, ws_bytes, stream, q_group, r_group, group_box);
}

DQO_API size_t dqo_knn3_workspace_bytes(int32_t P) { return dqo_knn3_ws_bytes(P < 0 ? 0 : P); }

DQO_API int dqo_knn3(int32_t P, const float* xyz, float* mean_d2, int32_t* idx3, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(xyz && mean_d2 && idx3, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_knn3_ws_bytes(P)) {
        dqo_set_error("knn workspace too small (%zu < %zu)", ws_bytes, dqo_knn3_ws_bytes(P));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_knn3(P, xyz, mean_d2, idx3, ws, ws_bytes, (hipStream_t)stream);
}

DQO_API int dqo_quadric_iou_fwd_bwd(int32_t B, const float* axes, const float* R, const float* center, const float* P34, const float* obs,
                                    float* bbox, float* loss, int32_t* valid, float* g_axes, float* g_R, float* g_center, void* stream) {
    DQO_CHECK_ARG(B >= 0, "bad B");
    if (B == 0) return DQO_OK;
    DQO_CHECK_ARG(axes && R && center && P34 && obs && bbox && loss && valid && g_axes && g_R && g_center, "null pointer");
    return dqo_launch_quadric_iou(B, axes, R, center, P34, obs, bbox, loss, valid, g_axes, g_R, g_center, (hipStream_t)stream);
}

DQO_API int dqo_map_activate(int32_t P, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, float* opacity,
                             float* scales, float* rotations, void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(opacity_raw && scaling_raw && rotation_raw && opacity && scales && rotations, "null pointer");
    return dqo_launch_map_activate(P, opacity_raw, scaling_raw, rotation_raw, opacity, scales, rotations, (hipStream_t)stream);
}

DQO_API size_t dqo_map_loss_workspace_bytes(void) { return dqo_map_loss_ws_bytes(); }

DQO_API int dqo_map_loss_fwd_bwd(int32_t W, int32_t H, const float* color, const float* depth, const int32_t* depth_index,
                                 const float* gt_color, const float* gt_depth, const uint8_t* render_mask, float color_weight,
                                 float depth_weight, float add_depth_thres, float* loss_out, float* dL_dcolor, float* dL_ddepth, void* ws,
                                 size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0, "bad image size");
    DQO_CHECK_ARG(color && depth && depth_index && gt_color && gt_depth && loss_out && dL_dcolor && dL_ddepth, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_map_loss_ws_bytes()) {
        dqo_set_error("loss workspace too small (%zu < %zu)", ws_bytes, dqo_map_loss_ws_bytes());
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_map_loss(W, H, color, depth, depth_index, gt_color, gt_depth, render_mask, color_weight, depth_weight,
                               add_depth_thres, loss_out, dL_dcolor, dL_ddepth, ws, (hipStream_t)stream);
}

DQO_API size_t dqo_map_ssim_workspace_bytes(int32_t W, int32_t H) { return (W > 0 && H > 0) ? dqo_map_ssim_ws_bytes(W, H) : 0; }

DQO_API int dqo_map_ssim_fwd_bwd(int32_t W, int32_t H, const float* image, const float* gt_image, float weight, float* ssim_out,
                                 float* dL_dimage, int32_t accumulate, float* loss_out8, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0, "bad image size");
    DQO_CHECK_ARG(image && gt_image && ssim_out, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_map_ssim_ws_bytes(W, H)) {
        dqo_set_error("ssim workspace too small (%zu < %zu)", ws_bytes, dqo_map_ssim_ws_bytes(W, H));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_map_ssim(W, H, image, gt_image, weight, ssim_out, dL_dimage, accumulate != 0, loss_out8, ws, (hipStream_t)stream);
}

DQO_API size_t dqo_map_attach_workspace_bytes(int32_t P) { return dqo_map_attach_ws_bytes(P < 0 ? 0 : P); }

DQO_API int dqo_map_history_merge(int32_t P, int32_t M, float max_weight, int32_t first_row, const uint8_t* row_flags, const float* conf0,
                                  const float* conf, const float* xyz0, const float* shs0, const float* scaling0, const float* rot0_unit,
                                  float* xyz, float* shs, float* scaling_raw, float* rotation_raw, void* stream) {
    DQO_CHECK_ARG(P >= 0 && M >= 1 && M * 3 < 256, "bad P / M");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(first_row >= 0 && first_row < P, "first_row %d outside [0, %d)", first_row, P);
    DQO_CHECK_ARG(conf0 && conf && xyz0 && shs0 && scaling0 && rot0_unit && xyz && shs && scaling_raw && rotation_raw, "null tensor");
    return dqo_launch_history_merge(P, M, max_weight, first_row, row_flags, conf0, conf, xyz0, shs0, scaling0, rot0_unit, xyz, shs,
                                    scaling_raw, rotation_raw, (hipStream_t)stream);
}

DQO_API int dqo_map_attach_loss_fwd_bwd(int32_t P, const float* scaling_raw, const float* xyz, const float* rotation_raw,
                                        const float* init_scaling_raw, const float* init_xyz, const float* init_rotation_raw,
                                        const uint8_t* attach_mask, int32_t attach_count, float* loss, float* g_scaling_raw, float* g_xyz,
                                        float* g_rotation_raw, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(P >= 0 && attach_count >= 0, "bad P / attach_count");
    DQO_CHECK_ARG(loss, "null loss");
    if (P == 0) return dqo_launch_zero_words(reinterpret_cast<uint32_t*>(loss), 1, (hipStream_t)stream);
    DQO_CHECK_ARG(scaling_raw && xyz && rotation_raw && init_scaling_raw && init_xyz && init_rotation_raw && attach_mask && g_scaling_raw &&
                      g_xyz && g_rotation_raw, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_map_attach_ws_bytes(P)) {
        dqo_set_error("attach-loss workspace too small (%zu < %zu)", ws_bytes, dqo_map_attach_ws_bytes(P));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_map_attach(P, scaling_raw, xyz, rotation_raw, init_scaling_raw, init_xyz, init_rotation_raw, attach_mask, attach_count,
                                 loss, g_scaling_raw, g_xyz, g_rotation_raw, ws, (hipStream_t)stream);
}

static int check_adam_multi(const DqoAdamTensor* ts, int32_t n_tensors, double beta1, double beta2, double eps) {
    DQO_CHECK_ARG(n_tensors >= 0 && n_tensors <= DQO_ADAM_MULTI_MAX, "n_tensors out of range");
    DQO_CHECK_ARG(n_tensors == 0 || ts != nullptr, "null tensor list");
    DQO_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "bad betas / eps");
    int64_t total = 0;
    for (int t = 0; t < n_tensors; t++) {
        DQO_CHECK_ARG(ts[t].n >= 0, "negative element count");
        DQO_CHECK_ARG(ts[t].n == 0 || (ts[t].p && ts[t].g && ts[t].m && ts[t].v), "null pointer in the tensor list");
        total += ts[t].n;
    }
    DQO_CHECK_ARG(total < ((int64_t)1 << 40), "too many elements");
    return DQO_OK;
}

DQO_API int dqo_adam_multi(const DqoAdamTensor* ts, int32_t n_tensors, int32_t step, double beta1, double beta2, double eps, void* stream) {
    DQO_CHECK_ARG(step >= 1, "step is the 1-based count of this update");
    const int rc = check_adam_multi(ts, n_tensors, beta1, beta2, eps);
    if (rc) return rc;
    return dqo_launch_adam_multi(ts, n_tensors, step, beta1, beta2, eps, (hipStream_t)stream);
}

DQO_API int dqo_adam_multi_dev(const DqoAdamTensor* ts, int32_t n_tensors, int32_t* step_dev, int32_t advance, double beta1, double beta2,
                               double eps, void* stream) {
    DQO_CHECK_ARG(step_dev != nullptr, "null step counter");
    const int rc = check_adam_multi(ts, n_tensors, beta1, beta2, eps);
    if (rc) return rc;
    return dqo_launch_adam_multi(ts, n_tensors, 1, beta1, beta2, eps, (hipStream_t)stream, step_dev, advance != 0);
}

DQO_API int dqo_accumulate_gaussian_error(int32_t H, int32_t W, int32_t P, const float* ce, const float* de, const float* ne,
                                          const int32_t* ci, const int32_t* di, float color_thr, float depth_thr, float normal_thr,
                                          int32_t check_max, float* gs_color, float* gs_depth, float* gs_normal, float* rescale,
                                          int32_t* counters, void* stream) {
    DQO_CHECK_ARG(H > 0 && W > 0 && P >= 0, "bad sizes");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(ce && de && ne && ci && di && gs_color && gs_depth && gs_normal && rescale, "null pointer");
    DQO_CHECK_ARG(check_max || counters, "mean mode needs the counters scratch buffer");
    return dqo_launch_accumulate_error(H, W, P, ce, de, ne, ci, di, color_thr, depth_thr, normal_thr, check_max, gs_color, gs_depth,
                                       gs_normal, rescale, counters, (hipStream_t)stream);
}

DQO_API int dqo_accumulate_gaussian_confidence(int32_t H, int32_t W, int32_t P, const int32_t* gaussian_index_map,
                                               const float* gaussian_confidence_map, float* gs_max, float* gs_min, float* gs_mean,
                                               int32_t* counter, void* stream) {
    DQO_CHECK_ARG(H > 0 && W > 0 && P >= 0, "bad sizes");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(gaussian_index_map && gaussian_confidence_map && gs_max && gs_min && gs_mean && counter, "null pointer");
    return dqo_launch_accumulate_confidence(H, W, P, gaussian_index_map, gaussian_confidence_map, gs_max, gs_min, gs_mean, counter,
                                            (hipStream_t)stream);
}

DQO_API int dqo_tile_count_mask(int32_t W, int32_t H, const uint8_t* pixel_mask, int32_t* tile_count, void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0 && pixel_mask && tile_count, "bad size / null pointer");
    return dqo_launch_tile_count(W, H, 0, pixel_mask, nullptr, nullptr, tile_count, nullptr, (hipStream_t)stream);
}

DQO_API int dqo_transmission_mask(int32_t W, int32_t H, const float* T_map, uint8_t* render_mask, int32_t* tile_count, int32_t* total,
                                  void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0 && T_map && tile_count, "bad size / null pointer");
    return dqo_launch_tile_count(W, H, 1, nullptr, T_map, render_mask, tile_count, total, (hipStream_t)stream);
}

DQO_API int dqo_tile_color_error(int32_t W, int32_t H, const float* render, const float* gt, float* color_error, float* tile_sum,
                                 void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0 && render && gt && tile_sum, "bad size / null pointer");
    return dqo_launch_tile_color_error(W, H, render, gt, color_error, tile_sum, (hipStream_t)stream);
}

// Mapping.evaluate_render_range (SLAM/multiprocess/mapper.py:930-988) as called once per frame of the window by local_optimize (:549-555)
// and global_optimization (:1173-1189): render mask (:945, :970-978), tile mask (transmission2tilemask SLAM/utils.py:752-762 / the top-k of
// colorerror2tilemask :766-799) and render ratio (:987) of one frame, written where the captured graphs read them
static bool window_masks_size_ok(int32_t W, int32_t H) { return W > 0 && H > 0 && (int64_t)W * H < (1ll << 31) / 3; }

DQO_API size_t dqo_window_masks_workspace_bytes(int32_t W, int32_t H) { return window_masks_size_ok(W, H) ? dqo_window_masks_ws_bytes(W, H) : 0; }

DQO_API int dqo_window_masks(int32_t W, int32_t H, int32_t mode, const float* T_map, const float* render, const float* gt, float tile_mask_ratio,
                             int32_t k, uint8_t* render_mask, int32_t* tile_mask, float* ratio_out, const DqoRastHeader* render_header,
                             void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(window_masks_size_ok(W, H), "bad image size");
    DQO_CHECK_ARG(mode >= 0 && mode <= 2, "bad mode %d", mode);
    DQO_CHECK_ARG(render_mask && tile_mask && ratio_out, "null output");
    const int64_t tiles = (int64_t)((W + 15) / 16) * ((H + 15) / 16);
    if (mode == 1) {
        DQO_CHECK_ARG(render && gt, "the error mode needs render and gt");
        DQO_CHECK_ARG(k >= 0 && k <= tiles, "k = %d outside [0, %lld]", k, (long long)tiles);
    } else {
        DQO_CHECK_ARG(T_map != nullptr, "null T_map");
    }
    DQO_CHECK_ARG(ws != nullptr && ws_bytes >= dqo_window_masks_ws_bytes(W, H), "window_masks workspace too small (%zu < %zu)", ws_bytes,
                  dqo_window_masks_ws_bytes(W, H));
    return dqo_launch_window_masks(W, H, mode, T_map, render, gt, tile_mask_ratio, k, render_mask, tile_mask, ratio_out, render_header, ws,
                                   (hipStream_t)stream);
}

DQO_API int dqo_attach_pixels(int32_t n, const float* temp_xyz, const float* viewmatrix, float fx, float fy, float cx, float cy, int32_t W,
                              int32_t H, const int32_t* pixel_object, int32_t* lin, int32_t* sparse_pixel_object, uint64_t* tile_objects,
                              void* stream) {
    DQO_CHECK_ARG(n >= 0 && W > 0 && H > 0 && (int64_t)W * H < (1ll << 31), "bad size");
    DQO_CHECK_ARG(viewmatrix && pixel_object && sparse_pixel_object && tile_objects && (n == 0 || (temp_xyz && lin)), "null pointer");
    return dqo_launch_attach_pixels(n, temp_xyz, viewmatrix, fx, fy, cx, cy, W, H, pixel_object, lin, sparse_pixel_object,
                                    reinterpret_cast<unsigned long long*>(tile_objects), (hipStream_t)stream);
}

DQO_API int dqo_attach_decide(int32_t n, const float* temp_xyz, const float* temp_opacity, const int32_t* temp_object, const int32_t* lin,
                              const int32_t* hit_index, const float* hit_weight, const float* xyz, const float* scaling_raw,
                              const float* rotation_raw, const int32_t* gaussian_object, float plane_thr, float opacity_low, uint8_t* out,
                              void* stream) {
    DQO_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return DQO_OK;
    DQO_CHECK_ARG(temp_xyz && temp_opacity && temp_object && lin && hit_index && hit_weight && xyz && scaling_raw && rotation_raw &&
                      gaussian_object && out, "null pointer");
    return dqo_launch_attach_decide(n, temp_xyz, temp_opacity, temp_object, lin, hit_index, hit_weight, xyz, scaling_raw, rotation_raw,
                                    gaussian_object, plane_thr, opacity_low, out, (hipStream_t)stream);
}

DQO_API int dqo_growth_scales(int32_t n, const float* xyz, const int32_t* object, const float* radius, const int32_t* i_new,
                              const float* d2_old, const int32_t* i_old, const float* extra_radius, float reach2, float min_radius,
                              float max_radius, float* scales, uint8_t* invalid, void* stream) {
    DQO_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return DQO_OK;
    DQO_CHECK_ARG(xyz && object && radius && scales && invalid, "null pointer");
    DQO_CHECK_ARG(i_old == nullptr || (d2_old && extra_radius), "i_old without d2_old / extra_radius");
    return dqo_launch_growth_scales(n, xyz, object, radius, i_new, d2_old, i_old, extra_radius, reach2, min_radius, max_radius, scales, invalid,
                                    (hipStream_t)stream);
}

DQO_API int dqo_growth_inside(int32_t n, const float* d2, const int32_t* idx, const float* radius, uint8_t* inside, void* stream) {
    DQO_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return DQO_OK;
    DQO_CHECK_ARG(d2 && idx && radius && inside, "null pointer");
    return dqo_launch_growth_inside(n, d2, idx, radius, inside, (hipStream_t)stream);
}

DQO_API int dqo_error_maps(int32_t H, int32_t W, const float* gt_color, const float* gt_depth, const float* render, const float* depth,
                           const int32_t* depth_index, const uint8_t* mask, float* color_err, float* depth_err, void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0 && gt_color && gt_depth && render && depth && depth_index && color_err && depth_err, "bad size / null pointer");
    return dqo_launch_error_maps((int64_t)W * H, gt_color, gt_depth, render, depth, depth_index, mask, color_err, depth_err, (hipStream_t)stream);
}

DQO_API size_t dqo_map_lifecycle_workspace_bytes(int32_t P) { return dqo_lifecycle_ws_bytes(P < 0 ? 0 : P); }

static int check_lifecycle(const DqoLifecycle* a) {
    DQO_CHECK_ARG(a != nullptr, "null DqoLifecycle");
    DQO_CHECK_ARG(a->P >= 0 && a->delete_thresh >= 1, "bad P / delete_thresh");
    if (a->P == 0) return DQO_OK;
    DQO_CHECK_ARG(a->xyz && a->opacity_raw && a->scaling_raw && a->confidence && a->alive && a->row_flags && a->stable && a->add_tick &&
                      a->depth_error_counter && a->color_error_counter && a->park && a->vote, "null per-Gaussian buffer / park / vote");
    if (a->workspace == nullptr || a->workspace_bytes < dqo_lifecycle_ws_bytes(a->P)) {
        dqo_set_error("lifecycle workspace too small (%zu < %zu)", a->workspace_bytes, dqo_lifecycle_ws_bytes(a->P));
        return DQO_ERR_WORKSPACE;
    }
    return DQO_OK;
}

DQO_API int dqo_map_lifecycle_vote(const DqoLifecycle* step, const float* gt_color, const float* gt_depth, const float* render_color,
                                   const float* render_depth, const int32_t* depth_index, const int32_t* color_index, void* stream) {
    const int rc = check_lifecycle(step);
    if (rc) return rc;
    DQO_CHECK_ARG(step->W > 0 && step->H > 0 && (int64_t)step->W * step->H < (1ll << 31), "bad image size");
    DQO_CHECK_ARG(gt_color && gt_depth && render_color && render_depth && depth_index && color_index, "null image");
    if (step->P == 0) return DQO_OK;
    return dqo_launch_lifecycle_vote(step, gt_color, gt_depth, render_color, render_depth, depth_index, color_index, (hipStream_t)stream);
}

DQO_API int dqo_map_lifecycle_rows(const DqoLifecycle* step, void* stream) {
    const int rc = check_lifecycle(step);
    if (rc) return rc;
    DQO_CHECK_ARG(step->stats != nullptr, "null stats");
    if (step->P == 0) return dqo_launch_zero_words(reinterpret_cast<uint32_t*>(step->stats), 8, (hipStream_t)stream);
    return dqo_launch_lifecycle_rows(step, (hipStream_t)stream);
}

// Mapping.temp_points_init (SLAM/multiprocess/mapper.py:1231-1347), sample_pixels (SLAM/utils.py:145-212) and
// GaussianPointCloud.add_empty_points (SLAM/gaussian_pointcloud.py:445-517)
DQO_API size_t dqo_growth_sample_workspace_bytes(int32_t W, int32_t H) {
    return (W > 0 && H > 0 && (int64_t)W * H < (1ll << 31) / 3) ? dqo_sample_ws_bytes((int64_t)W * H) : 0;
}

DQO_API int dqo_growth_sample(const DqoGrowthSample* a, void* stream) {
    DQO_CHECK_ARG(a != nullptr, "null DqoGrowthSample");
    DQO_CHECK_ARG(a->W > 0 && a->H > 0 && (int64_t)a->W * a->H < (1ll << 31) / 3, "bad image size");
    DQO_CHECK_ARG(a->uniform_sample_num >= 0 && a->capacity >= 0 && a->M >= 1, "bad uniform_sample_num / capacity / M");
    DQO_CHECK_ARG(a->key_bits >= 1 && a->key_bits <= 32, "key_bits must be in [1, 32]");
    DQO_CHECK_ARG(a->transmission_sample_ratio >= 0.f && a->error_sample_ratio >= 0.f, "negative sample ratio");
    DQO_CHECK_ARG(a->vertex && a->normal && a->color && a->depth && a->header, "null frame image / header");
    DQO_CHECK_ARG(a->first_frame || (a->T && a->render_depth && a->render_color && a->depth_index), "null render image");
    DQO_CHECK_ARG(a->capacity == 0 || (a->xyz && a->scales && a->rotations && a->opacity && a->shs && a->out_normal && a->pixel),
                  "null row buffer");
    if (a->workspace == nullptr || a->workspace_bytes < dqo_sample_ws_bytes((int64_t)a->W * a->H)) {
        dqo_set_error("growth sample workspace too small (%zu < %zu)", a->workspace_bytes, dqo_sample_ws_bytes((int64_t)a->W * a->H));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_growth_sample(a, (hipStream_t)stream);
}

// eval_picture (SLAM/eval.py:38-188): psnr (:63), l1_loss (:70), the depth statements (:115-126)
DQO_API size_t dqo_eval_picture_workspace_bytes(int32_t W, int32_t H) {
    return (W > 0 && H > 0 && (int64_t)W * H < (1ll << 31) / 3) ? dqo_eval_ws_bytes((int64_t)W * H) : 0;
}

DQO_API int dqo_eval_picture(int32_t W, int32_t H, const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                             const int32_t* depth_index, float min_depth, float max_depth, const DqoRastHeader* render_header, float* out,
                             int32_t row, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(W > 0 && H > 0 && (int64_t)W * H < (1ll << 31) / 3, "bad image size");
    DQO_CHECK_ARG(render && gt_color && depth && gt_depth && depth_index && out, "null pointer");
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    if (ws == nullptr || ws_bytes < dqo_eval_ws_bytes((int64_t)W * H)) {
        dqo_set_error("eval_picture workspace too small (%zu < %zu)", ws_bytes, dqo_eval_ws_bytes((int64_t)W * H));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_eval_picture(W, H, render, gt_color, depth, gt_depth, depth_index, min_depth, max_depth, render_header,
                                   out + (size_t)8 * row, ws, (hipStream_t)stream);
}

// eval_picture's "ssim" (SLAM/eval.py:19-25, :64): pytorch_msssim's ms_ssim, which asserts min(H, W) > (11 - 1) * 2^4
static bool msssim_size_ok(int32_t W, int32_t H) { return W > 160 && H > 160 && (int64_t)W * H < (1ll << 31) / 3; }

DQO_API size_t dqo_eval_ms_ssim_workspace_bytes(int32_t W, int32_t H) { return msssim_size_ok(W, H) ? dqo_msssim_ws_bytes(W, H) : 0; }

DQO_API int dqo_eval_ms_ssim(int32_t W, int32_t H, const float* render, const float* gt_color, const DqoRastHeader* render_header, float* out,
                             int32_t row, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(msssim_size_ok(W, H), "bad image size %d x %d: MS-SSIM needs both sides > 160 (five levels of an 11-tap window)", W, H);
    DQO_CHECK_ARG(render && gt_color && out, "null pointer");
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    if (ws == nullptr || ws_bytes < dqo_msssim_ws_bytes(W, H)) {
        dqo_set_error("ms_ssim workspace too small (%zu < %zu)", ws_bytes, dqo_msssim_ws_bytes(W, H));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_msssim(W, H, render, gt_color, render_header, out + (size_t)20 * row, ws, (hipStream_t)stream);
}

// the index word of a sorted point carries 25 index bits (knn.hip: FINE_IDX_BITS)
static bool nn1_size_ok(int32_t n) { return n >= 0 && n < (1 << 25); }

DQO_API size_t dqo_nn1_workspace_bytes(int32_t Q, int32_t R) { return nn1_size_ok(Q) && nn1_size_ok(R) ? dqo_nn1_ws_bytes(Q, R) : 0; }

DQO_API int dqo_nn1(int32_t Q, const float* q_xyz, const uint8_t* q_keep, int32_t R, const float* r_xyz, const uint8_t* r_keep,
                    const float* q_xform, const float* r_xform, float* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(nn1_size_ok(Q) && nn1_size_ok(R), "bad size: at most 2^25 - 1 rows per set");
    if (Q == 0) return DQO_OK;
    DQO_CHECK_ARG(q_xyz && dist2, "null query / output");
    DQO_CHECK_ARG(R == 0 || r_xyz, "null reference set");
    if (ws == nullptr || ws_bytes < dqo_nn1_ws_bytes(Q, R)) {
        dqo_set_error("nn1 workspace too small (%zu < %zu)", ws_bytes, dqo_nn1_ws_bytes(Q, R));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_nn1(Q, q_xyz, q_keep, R, r_xyz, r_keep, q_xform, r_xform, dist2, idx, ws, (hipStream_t)stream);
}

// eval_pcd (SLAM/eval.py:190-282): accuracy, completion, chamfer distance, precision / recall / F1 per threshold
DQO_API size_t dqo_eval_pcd_workspace_bytes(int32_t n_gt, int32_t n_rec) {
    return nn1_size_ok(n_gt) && nn1_size_ok(n_rec) ? dqo_eval_pcd_ws_bytes(n_gt, n_rec) : 0;
}

DQO_API int dqo_eval_pcd(int32_t n_gt, const float* gt_xyz, const uint8_t* gt_keep, int32_t n_rec, const float* rec_xyz, const uint8_t* rec_keep,
                         const float* rec_xform, int32_t n_thres, const float* thres_host, float* out_table, int32_t row, void* ws,
                         size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(nn1_size_ok(n_gt) && nn1_size_ok(n_rec), "bad size: at most 2^25 - 1 rows per set");
    DQO_CHECK_ARG((n_gt == 0 || gt_xyz) && (n_rec == 0 || rec_xyz) && out_table, "null pointer");
    DQO_CHECK_ARG(n_thres >= 0 && n_thres <= 8 && (n_thres == 0 || thres_host), "at most 8 thresholds (got %d)", n_thres);
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    if (ws == nullptr || ws_bytes < dqo_eval_pcd_ws_bytes(n_gt, n_rec)) {
        dqo_set_error("eval_pcd workspace too small (%zu < %zu)", ws_bytes, dqo_eval_pcd_ws_bytes(n_gt, n_rec));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_eval_pcd(n_gt, gt_xyz, gt_keep, n_rec, rec_xyz, rec_keep, rec_xform, n_thres, thres_host, out_table + (size_t)32 * row, ws,
                               (hipStream_t)stream);
}

// GaussianPointCloud.densify (SLAM/gaussian_pointcloud.py:67-130) and eval_pcd's subsample (SLAM/eval.py:244).  M, or 0 for a bad size
static int64_t densify_columns(int32_t P, int32_t circle_num, int32_t levels, int32_t sigma) {
    if (P < 1 || circle_num < 1 || levels < 1 || sigma < 1 || circle_num > 1024) return 0;
    const int64_t ring = (int64_t)circle_num * levels;
    if (ring > 65535) return 0;
    const int64_t M = ring * sigma;
    return (M > 65535 || (int64_t)P * M >= (1ll << 32)) ? 0 : M;
}

DQO_API size_t dqo_surfel_densify_workspace_bytes(int32_t P, int32_t circle_num, int32_t levels, int32_t sigma) {
    const int64_t M = densify_columns(P, circle_num, levels, sigma);
    return M > 0 ? dqo_densify_ws_bytes((uint64_t)P * (uint64_t)M) : 0;
}

DQO_API int dqo_surfel_densify(int32_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const uint8_t* row_keep,
                               int32_t circle_num, int32_t levels, int32_t sigma, const float* circle_cs, int32_t frame, uint64_t seed,
                               int64_t cap, float* points, float* normals, int64_t* index, uint8_t* keep, int32_t* header, void* ws,
                               size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(P >= 1, "bad row count %d", P);
    DQO_CHECK_ARG(circle_num >= 1 && levels >= 1 && sigma >= 1, "circle_num, levels and sigma must be at least 1 (got %d, %d, %d)", circle_num,
                  levels, sigma);
    DQO_CHECK_ARG(circle_num <= 1024, "circle_num %d: at most 1024", circle_num);
    DQO_CHECK_ARG((int64_t)circle_num * levels <= 65535 && (int64_t)circle_num * levels * sigma <= 65535,
                  "circle_num * levels * sigma: at most 65535 points per row");
    const int64_t M = densify_columns(P, circle_num, levels, sigma);
    DQO_CHECK_ARG(M > 0, "P * circle_num * levels * sigma must stay below 2^32");
    DQO_CHECK_ARG(cap >= 1, "bad capacity %lld", (long long)cap);
    DQO_CHECK_ARG(frame == DQO_DENSIFY_FRAME_REFERENCE || frame == DQO_DENSIFY_FRAME_SURFEL, "bad frame %d", frame);
    DQO_CHECK_ARG(xyz && scaling_raw && rotation_raw && circle_cs && points && keep && header, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_densify_ws_bytes((uint64_t)P * (uint64_t)M)) {
        dqo_set_error("surfel densify workspace too small (%zu < %zu)", ws_bytes, dqo_densify_ws_bytes((uint64_t)P * (uint64_t)M));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_surfel_densify(P, xyz, scaling_raw, rotation_raw, row_keep, circle_num, levels, sigma, circle_cs, frame, seed, cap, points,
                                     normals, index, keep, header, ws, (hipStream_t)stream);
}

// trimesh.sample.sample_surface on the ground-truth mesh (SLAM/eval.py:247).  The face table's and dqo_nn1's row limit
static bool mesh_size_ok(int32_t n) { return n >= 1 && n < (1 << 25); }

DQO_API size_t dqo_mesh_sample_workspace_bytes(int32_t F, int32_t count) {
    return mesh_size_ok(F) && mesh_size_ok(count) ? dqo_mesh_sample_ws_bytes(F) : 0;
}

DQO_API int dqo_mesh_sample(int32_t V, const float* vertices, int32_t F, const int32_t* faces, int32_t count, uint64_t seed, float* points,
                            int32_t* face_index, uint8_t* keep, int32_t* header, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(V >= 1, "bad vertex count %d", V);
    DQO_CHECK_ARG(mesh_size_ok(F), "bad face count %d: 1 to 2^25 - 1 faces", F);
    DQO_CHECK_ARG(mesh_size_ok(count), "bad sample count %d: 1 to 2^25 - 1 samples", count);
    DQO_CHECK_ARG(vertices && faces && points && keep && header, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_mesh_sample_ws_bytes(F)) {
        dqo_set_error("mesh sample workspace too small (%zu < %zu)", ws_bytes, dqo_mesh_sample_ws_bytes(F));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_mesh_sample(V, vertices, F, faces, count, seed, points, face_index, keep, header, ws, (hipStream_t)stream);
}

// the vertex table of a map checkpoint: at most 2^31 - 1 floats, SH sizes up to 64 coefficients (a tile of 64 rows stays below 64 KiB of LDS)
static bool map_table_size_ok(int64_t rows, int32_t M, int32_t with_conf) {
    return rows >= 1 && M >= 1 && M <= 64 && rows * (int64_t)(6 + 3 * M + 8 + (with_conf ? 1 : 0)) <= (int64_t)0x7fffffff;
}

DQO_API size_t dqo_map_pack_workspace_bytes(int32_t P) { return P >= 1 ? dqo_map_pack_ws_bytes(P) : 0; }

DQO_API int dqo_map_pack_rows(int32_t P, int32_t M, int32_t include_confidence, const float* xyz, const float* shs, const float* opacity_raw,
                              const float* scaling_raw, const float* rotation_raw, const float* confidence, const uint8_t* alive,
                              const uint8_t* stable, float* table, int64_t table_rows, int32_t* header, void* ws, size_t ws_bytes,
                              void* stream) {
    DQO_CHECK_ARG(P >= 1, "bad row count %d", P);
    DQO_CHECK_ARG(M >= 1 && M <= 64, "bad SH size M = %d: 1 to 64 coefficients", M);
    DQO_CHECK_ARG(map_table_size_ok(P, M, include_confidence), "bad size: a table of %d rows exceeds 2^31 - 1 floats", P);
    DQO_CHECK_ARG(xyz && shs && opacity_raw && scaling_raw && rotation_raw && table && header, "null pointer");
    DQO_CHECK_ARG(table_rows >= (int64_t)P, "table capacity %lld rows is below the map's %d rows", (long long)table_rows, P);
    if (ws == nullptr || ws_bytes < dqo_map_pack_ws_bytes(P)) {
        dqo_set_error("map pack workspace too small (%zu < %zu)", ws_bytes, dqo_map_pack_ws_bytes(P));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_map_pack(P, M, include_confidence != 0, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence, alive, stable, table,
                               header, ws, (hipStream_t)stream);
}

DQO_API int dqo_map_unpack_rows(int32_t P, int32_t M, int32_t n, int32_t first_row, int32_t has_confidence, const float* table, float* xyz,
                                float* shs, float* opacity_raw, float* scaling_raw, float* rotation_raw, float* confidence, void* stream) {
    DQO_CHECK_ARG(P >= 1 && n >= 0 && first_row >= 0 && (int64_t)first_row + n <= (int64_t)P, "bad size: rows [%d, %d + %d) of a map of %d rows",
                  first_row, first_row, n, P);
    DQO_CHECK_ARG(M >= 1 && M <= 64, "bad SH size M = %d: 1 to 64 coefficients", M);
    DQO_CHECK_ARG(map_table_size_ok(P, M, 1), "bad size: a table of %d rows exceeds 2^31 - 1 floats", P);
    if (n == 0) return DQO_OK;
    DQO_CHECK_ARG(table && xyz && shs && opacity_raw && scaling_raw && rotation_raw, "null pointer");
    return dqo_launch_map_unpack(M, n, first_row, has_confidence != 0, table, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence,
                                 (hipStream_t)stream);
}

DQO_API size_t dqo_icp_workspace_bytes(void) { return dqo_icp_ws_bytes(); }

DQO_API int dqo_icp_normal_equations(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0,
                                     const float* normal1, const float* pose10, float fx, float fy, float cx, float cy, float dist_thr,
                                     float normal_thr, float* JtJ, float* JtR, int32_t* valid_count, void* ws, size_t ws_bytes,
                                     void* stream) {
    DQO_CHECK_ARG(H > 1 && W > 1 && (int64_t)H * W < (int64_t)0x7fffffff / 3, "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && normal1 && pose10 && JtJ && JtR && valid_count, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_icp_ws_bytes()) {
        dqo_set_error("icp workspace too small (%zu < %zu)", ws_bytes, dqo_icp_ws_bytes());
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_icp(H, W, vertex0, vertex1, normal0, normal1, pose10, fx, fy, cx, cy, dist_thr, normal_thr, JtJ, JtR, valid_count, ws,
                          (hipStream_t)stream);
}

// image sizes of the tracker entry points: positive, and H * W * 4 floats still indexable with int
static bool track_size_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W < (int64_t)0x7fffffff / 4; }

DQO_API int dqo_icp_gauss_newton(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1,
                                 float* pose10, const float* K, float k_scale, float dist_thr, float normal_thr, float damping,
                                 int32_t* valid_count, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(H > 1 && W > 1 && (int64_t)H * W < (int64_t)0x7fffffff / 3, "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && normal1 && pose10 && K && valid_count, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_icp_ws_bytes()) {
        dqo_set_error("icp workspace too small (%zu < %zu)", ws_bytes, dqo_icp_ws_bytes());
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_icp_gauss_newton(H, W, vertex0, vertex1, normal0, normal1, pose10, K, k_scale, dist_thr, normal_thr, damping, valid_count,
                                       ws, (hipStream_t)stream);
}

DQO_API size_t dqo_track_preprocess_workspace_bytes(int32_t H, int32_t W) {
    return track_size_ok(H, W) ? dqo_track_preprocess_ws_bytes(H, W) : 0;
}

DQO_API int dqo_track_preprocess(int32_t H, int32_t W, const float* depth, const float* K, float min_depth, float max_depth, float conf_thr,
                                 int32_t depth_filter, float* depth_out, float* vertex_out, float* normal_out, float* conf_out, uint8_t* invalid_out, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(depth && K && depth_out && vertex_out && normal_out && conf_out && invalid_out, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_track_preprocess_ws_bytes(H, W)) {
        dqo_set_error("track preprocess workspace too small (%zu < %zu)", ws_bytes, dqo_track_preprocess_ws_bytes(H, W));
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_track_preprocess(H, W, depth, K, min_depth, max_depth, conf_thr, depth_filter ? 1 : 0, depth_out, vertex_out,
                                       normal_out, conf_out, invalid_out, ws, (hipStream_t)stream);
}

DQO_API int64_t dqo_track_pyramid_pixels(int32_t H, int32_t W, int32_t levels) {
    if (!track_size_ok(H, W) || levels < 1 || levels > 4) return -1;
    return dqo_track_pyramid_pixel_count(H, W, levels);
}

DQO_API size_t dqo_track_pyramid_workspace_bytes(void) { return dqo_track_pyramid_ws_bytes(); }

DQO_API int dqo_track_pyramid(int32_t H, int32_t W, int32_t levels, const float* depth, const float* K, float* vertex, float* normal, void* ws,
                              size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(levels >= 1 && levels <= 4, "levels must be in [1, 4]");
    DQO_CHECK_ARG(track_size_ok(H, W) && (H >> (levels - 1)) > 0 && (W >> (levels - 1)) > 0, "bad image size for %d levels", levels);
    DQO_CHECK_ARG(depth && K && vertex && normal, "null pointer");
    if (ws == nullptr || ws_bytes < dqo_track_pyramid_ws_bytes()) {
        dqo_set_error("track pyramid workspace too small (%zu < %zu)", ws_bytes, dqo_track_pyramid_ws_bytes());
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_track_pyramid(H, W, levels, depth, K, vertex, normal, ws, (hipStream_t)stream);
}

DQO_API int dqo_track_fill_model_depth(int32_t H, int32_t W, float* render_depth, const float* frame_depth, const float* render_normal,
                                       const float* frame_normal, float dist_thr, float normal_thr, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(render_depth && frame_depth && render_normal && frame_normal, "null pointer");
    return dqo_launch_track_fill(H, W, render_depth, frame_depth, render_normal, frame_normal, dist_thr, normal_thr, (hipStream_t)stream);
}

DQO_API size_t dqo_track_p2p_workspace_bytes(void) { return dqo_track_p2p_ws_bytes(); }

DQO_API int dqo_track_p2p_loss(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* pose10,
                               float fail_thr, const int32_t* valid_count, float* loss, int32_t* success, float* valid_ratio, void* ws,
                               size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && pose10 && loss && success, "null pointer");
    DQO_CHECK_ARG((valid_count == nullptr) == (valid_ratio == nullptr), "valid_count and valid_ratio go together");
    if (ws == nullptr || ws_bytes < dqo_track_p2p_ws_bytes()) {
        dqo_set_error("track p2p workspace too small (%zu < %zu)", ws_bytes, dqo_track_p2p_ws_bytes());
        return DQO_ERR_WORKSPACE;
    }
    return dqo_launch_track_p2p(H, W, vertex0, vertex1, normal0, pose10, fail_thr, valid_count, loss, success, valid_ratio, ws,
                                (hipStream_t)stream);
}

DQO_API int dqo_map_adam_step(const DqoAdamStep* st, void* stream) {
    const int rc = check_adam_step(st, true);
    if (rc) return rc;
    if (st->P == 0) return DQO_OK;
    return dqo_launch_map_adam(st, (hipStream_t)stream);
}

DQO_API int dqo_quadric_adam(int32_t n_obj, int32_t n_iters, const int32_t* view_offset, const float* P34_views, const float* obs_views,
                             const int32_t* view_schedule, float* axes, float* R, float* center, float* loss_hist, void* stream) {
    DQO_CHECK_ARG(n_obj >= 0 && n_iters >= 0, "bad sizes");
    if (n_obj == 0 || n_iters == 0) return DQO_OK;
    DQO_CHECK_ARG(view_offset && P34_views && obs_views && view_schedule && axes && R && center, "null pointer");
    return dqo_launch_quadric_adam(n_obj, n_iters, view_offset, P34_views, obs_views, view_schedule, axes, R, center, loss_hist,
                                   (hipStream_t)stream);
}

// the object table's capacities: a row per lane of the one workgroup, a detection per lane of its first wave, room for a covering
// replacement's doubled observation; the observation slots stay indexable with int
static bool objmap_caps_ok(int32_t cap_obj, int32_t cap_views) {
    return cap_obj >= 1 && cap_obj <= 1024 && cap_views >= 2 && (int64_t)cap_obj * cap_views * 12 <= (int64_t)0x7fffffff;
}

DQO_API int dqo_objmap_frame(int32_t cap_obj, int32_t cap_views, int32_t cap_det, float* obj_axes, float* obj_R, float* obj_center,
                             int32_t* obj_cat, int32_t* obj_uid, int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state,
                             int32_t M, const float* det_bbox, const float* det_ellipse, const int32_t* det_cat, const float* det_score,
                             const float* depth, const float* K, const float* Rt, int32_t W, int32_t H, int32_t frame_id, uint64_t seed,
                             int32_t* det_fate, int32_t* det_row, float* det_depth, uint8_t* opt_flag, int32_t* frame_header, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(cap_det >= 1 && cap_det <= 64, "bad capacity: cap_det %d (1 to 64)", cap_det);
    DQO_CHECK_ARG(M >= 1 && M <= cap_det, "bad detection count %d: 1 to cap_det = %d", M, cap_det);
    DQO_CHECK_ARG(W >= 1 && H >= 1 && (int64_t)W * H <= (int64_t)0x7fffffff, "bad image size %d x %d", W, H);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_cat && obj_uid && obj_nviews && view_P34 && view_bbox && state, "null pointer (table)");
    DQO_CHECK_ARG(det_bbox && det_ellipse && det_cat && det_score && depth && K && Rt, "null pointer (frame)");
    DQO_CHECK_ARG(det_fate && det_row && det_depth && opt_flag && frame_header, "null pointer (outputs)");
    return dqo_launch_objmap_frame(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_cat, obj_uid, obj_nviews, view_P34, view_bbox, state, M,
                                   det_bbox, det_ellipse, det_cat, det_score, depth, K, Rt, W, H, frame_id, seed, det_fate, det_row, det_depth,
                                   opt_flag, frame_header, (hipStream_t)stream);
}

DQO_API int dqo_objmap_optimize(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_uid,
                                int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state, const uint8_t* opt_flag,
                                int32_t frame_id, uint64_t seed, float* loss_hist, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_uid && obj_nviews && view_P34 && view_bbox && state && opt_flag, "null pointer");
    return dqo_launch_objmap_optimize(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_uid, obj_nviews, view_P34, view_bbox, state, opt_flag,
                                      frame_id, seed, loss_hist, (hipStream_t)stream);
}

DQO_API int dqo_objmap_mean_iou(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_nviews,
                                float* view_P34, float* view_bbox, int32_t* state, float* mean_iou, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_nviews && view_P34 && view_bbox && state && mean_iou, "null pointer");
    return dqo_launch_objmap_mean_iou(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_nviews, view_P34, view_bbox, state, mean_iou,
                                      (hipStream_t)stream);
}

}  // extern "C"
