// The activations of DQO-MAP's raw Gaussian parameters (SLAM/gaussian_pointcloud.py:732-733, 746-747, 815-822: sigmoid, exp,
// F.normalize) for the parameter form of the drop-in operator (dqo_rast_*_params, include/dqo_raster.h).  ONE definition for every
// kernel that activates on load — k1_early (preprocess_kernel<…, true>, bin_count_kernel<true, true>), k1_late_block (the sort kernels'
// extra blocks) and gaussian_rows_kernel<true> — so they all form the same bits, and those are the bits of activate_kernel (map_fused.hip), whose
// statements these are.  That kernel is compiled with the default contraction, and its sum of squares came out as four multiplies and
// three adds in this order (no v_fma): spelled the same way here, with contraction off.
// Everything here but DqoShRest and the DqoFormArg selector has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

// the SH coefficients 1.. of the parameter form: features_rest [P, m_rest, 3] (coefficient 0 comes from features_dc [P, 1, 3]).
// A kernel argument, and what the host launchers are handed for the parameter form (NULL = the activated form).
struct DqoShRest {
    const float* rest;
    int m_rest;
};

// A kernel argument that only one of the two forms has (DqoShRest, dL_drest: the parameter form; colors_precomp: the activated form):
// its type T in the instantiation that has it, an empty struct in the other.  dqo_form_arg<HAS>(x) is what a launch passes for it.
// The empty struct has size ZERO (a zero-length array member; `struct {}` has size 1): it takes no kernarg bytes, so neither the
// arguments behind it nor the hidden ones (gridDim, ...) behind the last explicit one move, and the activated-form kernels, which
// gained such an argument when the pairs became templates, keep the layout and the code they had without it.
struct DqoNoArg {
    int none[0];
};
static_assert(sizeof(DqoNoArg) == 0, "DqoNoArg must take no kernarg bytes");
template <bool HAS, class T>
using DqoFormArg = std::conditional_t<HAS, T, DqoNoArg>;
template <bool HAS, class T>
inline DqoFormArg<HAS, T> dqo_form_arg(const T x) {
    if constexpr (HAS) return x;
    else return DqoNoArg{};
}

namespace {

__device__ __forceinline__ float dqo_act_opacity(const float x) { return 1.0f / (1.0f + expf(-x)); }  // torch.sigmoid
__device__ __forceinline__ float dqo_act_scale(const float x) { return expf(x); }                    // torch.exp

__device__ __forceinline__ float dqo_act_rot_norm(const float4 q) {  // F.normalize(eps=1e-12): the divisor
#pragma clang fp contract(off)
    return fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
}
__device__ __forceinline__ float4 dqo_act_rotation(const float4 q) {
    const float n = dqo_act_rot_norm(q);
    return make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
}

// The activation Jacobians applied to the gradient w.r.t. the activated value — the forms of dqo_adam.h (adam_row_update,
// adam_xyz_update), one IEEE operation at a time
__device__ __forceinline__ float dqo_act_opacity_grad(const float g, const float s) {
#pragma clang fp contract(off)
    return g * (s * (1.f - s));
}
__device__ __forceinline__ float dqo_act_scale_grad(const float g, const float e) {
#pragma clang fp contract(off)
    return g * e;
}
// F.normalize backward: y = q / n, n = max(|q|, eps):  dq = (g - y (y . g)) / n
__device__ __forceinline__ float4 dqo_act_rotation_grad(const float4 g, const float4 q) {
#pragma clang fp contract(off)
    const float n = dqo_act_rot_norm(q);
    const float yx = q.x / n, yy = q.y / n, yz = q.z / n, yw = q.w / n;
    const float dot = yx * g.x + yy * g.y + yz * g.z + yw * g.w;
    return make_float4((g.x - yx * dot) / n, (g.y - yy * dot) / n, (g.z - yz * dot) / n, (g.w - yw * dot) / n);
}

}  // namespace
