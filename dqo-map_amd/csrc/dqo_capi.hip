// What the extern "C" entry points of libdqoraster.so (include/dqo_raster.h) share — the error string, the profiling brackets, the
// ABI queries — and the rasteriser's own entry points.  Every other operator's entry points (size query, argument validation, the
// call) sit in the .hip file that owns its launches.  No allocation, no synchronisation (except dqo_rast_read_header), no exceptions.
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
                                sizeof(DqoLifecycle), sizeof(DqoGrowthSample), 0 /* 16: unused */, sizeof(DqoWindowBank), sizeof(DqoTrajRepose),
                                sizeof(DqoReposeTarget)};
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

// The training form: the caller's struct is checked like every forward's, then the launches get a copy without the auxiliary members.
// NULL there is what selects the lean blend kernel (dqo_launch_blend_forward) and keeps K1 from zeroing n_touched; no other entry point
// lets a NULL output through.
DQO_API int dqo_rast_forward_train(const DqoRastParams* p, const DqoRastInputs* in, DqoRastOutputs* out, DqoRastCtx* ctx, void* stream) {
    int rc = check_render(p, in, out, ctx);
    if (rc) return rc;
    DQO_CHECK_ARG(ctx->loss_tap != nullptr, "dqo_rast_forward_train: without a loss tap the loss reads out_hit_depth");
    DQO_CHECK_ARG(dqo_list_split(ctx) == 0, "dqo_rast_forward_train: the list-split blend kernels have no training form");
    DqoRastOutputs lean = *out;
    lean.out_hit_color = nullptr, lean.out_hit_depth = nullptr, lean.out_hit_color_weight = nullptr, lean.out_hit_depth_weight = nullptr;
    lean.out_T = nullptr, lean.n_touched = nullptr;
    rc = dqo_launch_forward_prepare(p, in, &lean, ctx, (hipStream_t)stream);
    if (rc) return rc;
    return dqo_launch_forward_render(p, in, &lean, ctx, (hipStream_t)stream);
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

DQO_API int dqo_rast_backward_adam(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor,
                                   const float* dL_ddepth, const DqoAdamStep* st, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(p, in, ctx);
    if (rc) return rc;
    rc = dqo_check_adam_step(st, false);
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
}  // extern "C"
