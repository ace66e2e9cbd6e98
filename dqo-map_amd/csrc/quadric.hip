// Dual-quadric pose residual for gfx950: ellipsoid -> Q* -> C* = P Q* P^T -> ellipse -> bbox -> 1 - IoU, forward + analytic
// backward, and the whole 20-step Adam loop of Object_Optimize_only in ONE launch.
//
// Replaces /root/reference/SLAM/multiprocess/quadrics.py:285-290 (bboxes_iou), 2018-2091 (Ellipse_tensor),
// 2144-2220 (Ellipsoid_tensor), 2234-2298 (Object_Optimize_only).  The reference runs ~60 eager 4x4 torch ops (+ a
// torch.linalg.eig and two host syncs) per iteration per object — pure launch latency.  Here one lane owns one
// (object, view) pair (residual) or one object (Adam loop); the 2x2 eigen-decomposition is closed form.
#include "dqo_common.h"

#include "dqo_quadric_eval.h"

namespace {

__global__ void quadric_iou_kernel(int B, const float* __restrict__ axes, const float* __restrict__ R, const float* __restrict__ center,
                                   const float* __restrict__ P34, const float* __restrict__ obs, float* __restrict__ bbox,
                                   float* __restrict__ loss, int32_t* __restrict__ valid, float* __restrict__ g_axes,
                                   float* __restrict__ g_R, float* __restrict__ g_center) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float a[3], Rm[9], c[3], P[12], ob[4];
    for (int i = 0; i < 3; i++) a[i] = axes[3 * b + i], c[i] = center[3 * b + i];
    for (int i = 0; i < 9; i++) Rm[i] = R[9 * b + i];
    for (int i = 0; i < 12; i++) P[i] = P34[12 * b + i];
    for (int i = 0; i < 4; i++) ob[i] = obs[4 * b + i];
    QuadOut o;
    quadric_eval(a, Rm, c, P, ob, o);
    for (int i = 0; i < 4; i++) bbox[4 * b + i] = o.bbox[i];
    loss[b] = o.loss;
    valid[b] = o.valid;
    for (int i = 0; i < 3; i++) g_axes[3 * b + i] = o.g_axes[i], g_center[3 * b + i] = o.g_center[i];
    for (int i = 0; i < 9; i++) g_R[9 * b + i] = o.g_R[i];
}

// One lane per object: the whole Adam trajectory (quadrics.py:2251-2285) without leaving registers.
__global__ void quadric_adam_kernel(int n_obj, int n_iters, const int32_t* __restrict__ view_offset, const float* __restrict__ P34_views,
                                    const float* __restrict__ obs_views, const int32_t* __restrict__ view_schedule,
                                    float* __restrict__ axes, float* __restrict__ R, float* __restrict__ center,
                                    float* __restrict__ loss_hist) {
#pragma clang fp contract(off)
    const int ob = blockIdx.x * blockDim.x + threadIdx.x;
    if (ob >= n_obj) return;
    float prm[15], mm[15], vv[15];
    for (int i = 0; i < 3; i++) prm[i] = axes[3 * ob + i], prm[3 + i] = center[3 * ob + i];
    for (int i = 0; i < 9; i++) prm[6 + i] = R[9 * ob + i];
    for (int i = 0; i < 15; i++) mm[i] = 0.f, vv[i] = 0.f;
    const int v0 = view_offset[ob], nv = view_offset[ob + 1] - v0;
    double pow1 = 1.0, pow2 = 1.0;  // beta1^step, beta2^step
    for (int it = 0; it < n_iters; it++) {
        int vi = view_schedule[ob * n_iters + it];
        if (vi < 0) vi += nv;
        vi = min(max(vi, 0), nv - 1);
        float P[12], obx[4];
        for (int i = 0; i < 12; i++) P[i] = P34_views[12 * (v0 + vi) + i];
        for (int i = 0; i < 4; i++) obx[i] = obs_views[4 * (v0 + vi) + i];
        QuadOut o;
        quadric_eval(prm, prm + 6, prm + 3, P, obx, o);
        if (loss_hist) loss_hist[ob * n_iters + it] = o.loss;
        if (!o.valid) continue;  // loss == 1: the reference raises and `continue`s before backward()/step()
        pow1 *= 0.9;
        pow2 *= 0.999;
        const double bc1 = 1.0 - pow1, bc2 = 1.0 - pow2;
        const float bc2_sqrt = (float)sqrt(bc2);
        for (int i = 0; i < 15; i++) {
            const float gi = i < 3 ? o.g_axes[i] : (i < 6 ? o.g_center[i - 3] : o.g_R[i - 6]);
            const double lr = (i >= 3 && i < 6) ? 0.001 : 0.01;
            mm[i] = mm[i] + (gi - mm[i]) * (1.0f - 0.9f);
            vv[i] = vv[i] * 0.999f + (1.0f - 0.999f) * gi * gi;
            const float denom = sqrtf(vv[i]) / bc2_sqrt + 1e-15f;
            const float step_size = (float)(lr / bc1);
            prm[i] = prm[i] - step_size * (mm[i] / denom);
        }
    }
    for (int i = 0; i < 3; i++) axes[3 * ob + i] = prm[i], center[3 * ob + i] = prm[3 + i];
    for (int i = 0; i < 9; i++) R[9 * ob + i] = prm[6 + i];
}

}  // namespace

static int dqo_launch_quadric_iou(int B, const float* axes, const float* R, const float* center, const float* P34, const float* obs,
                                  float* bbox, float* loss, int32_t* valid, float* g_axes, float* g_R, float* g_center, hipStream_t s) {
    DQO_LAUNCH("quadric_iou_kernel", quadric_iou_kernel, dim3((B + 63) / 64), dim3(64), s, B, axes, R, center, P34, obs, bbox, loss, valid, g_axes,
                       g_R, g_center);
    return DQO_OK;
}

static int dqo_launch_quadric_adam(int n_obj, int n_iters, const int32_t* view_offset, const float* P34_views, const float* obs_views,
                                   const int32_t* view_schedule, float* axes, float* R, float* center, float* loss_hist, hipStream_t s) {
    DQO_LAUNCH("quadric_adam_kernel", quadric_adam_kernel, dim3((n_obj + 63) / 64), dim3(64), s, n_obj, n_iters, view_offset, P34_views, obs_views,
                       view_schedule, axes, R, center, loss_hist);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API int dqo_quadric_iou_fwd_bwd(int32_t B, const float* axes, const float* R, const float* center, const float* P34, const float* obs,
                                    float* bbox, float* loss, int32_t* valid, float* g_axes, float* g_R, float* g_center, void* stream) {
    DQO_CHECK_ARG(B >= 0, "bad B");
    if (B == 0) return DQO_OK;
    DQO_CHECK_ARG(axes && R && center && P34 && obs && bbox && loss && valid && g_axes && g_R && g_center, "null pointer");
    return dqo_launch_quadric_iou(B, axes, R, center, P34, obs, bbox, loss, valid, g_axes, g_R, g_center, (hipStream_t)stream);
}

DQO_API int dqo_quadric_adam(int32_t n_obj, int32_t n_iters, const int32_t* view_offset, const float* P34_views, const float* obs_views,
                             const int32_t* view_schedule, float* axes, float* R, float* center, float* loss_hist, void* stream) {
    DQO_CHECK_ARG(n_obj >= 0 && n_iters >= 0, "bad sizes");
    if (n_obj == 0 || n_iters == 0) return DQO_OK;
    DQO_CHECK_ARG(view_offset && P34_views && obs_views && view_schedule && axes && R && center, "null pointer");
    return dqo_launch_quadric_adam(n_obj, n_iters, view_offset, P34_views, obs_views, view_schedule, axes, R, center, loss_hist,
                                   (hipStream_t)stream);
}

}  // extern "C"
