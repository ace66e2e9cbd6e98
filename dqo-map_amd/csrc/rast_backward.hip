// Backward pass of the depth-aware Gaussian rasteriser for gfx950 (MI355X).
//
// Replaces (semantics, not structure) /root/reference/submodules/diff-gaussian-rasterizer-depth/
//   cuda_rasterizer/backward.cu:808-1066  renderCUDA_flat (+propagateRotationGrad :100-148)  -> blend_backward_kernel (rast_backward_blend.hip)
//   cuda_rasterizer/backward.cu:273-422   computeCov2DCUDA                                    \
//   cuda_rasterizer/backward.cu:492-548   preprocessCUDA (+SH bwd :152-268, cov3D bwd :426-487)/ -> gaussian_rows_kernel (map_fused_tail.hip)
//
// MI355X design: the reference issues ~10 scattered global float atomics per (pixel, Gaussian) pair plus 3-7 per hit
// pixel.  On gfx950 global float atomics execute memory-side and a wave instruction whose 64 lanes hit 64 different rows
// runs ~17x below the streaming rate (MI355X_MICROARCH.md, Global float atomics), so none are used here:
//   * one wave64 owns one 8x8 quadrant of a 16x16 tile (1 pixel per lane); the per-entry gradient is a reduction over the lanes
//     that may have work for it, shared by seven entries (rast_backward_blend.hip);
//   * the wave stores ONE 64-byte partial record per live (quadrant, instance) pair at the instance's gaussian-major
//     slot (4 partial records per slot + a validity word);
//   * gaussian_rows_kernel sums each Gaussian's valid partial records in a fixed order (bitwise reproducible), finishes the chain
//     rule (cov2D, projection, SH, cov3D, depth-hit Jacobians, dqo_gauss_chain.h) and writes the gradient rows.
#include "dqo_common.h"

int dqo_launch_backward(const DqoRastParams* p, const DqoRastInputs* in, const DqoRastCtx* ctx, const float* dL_dcolor,
                        const float* dL_ddepth, const int32_t* hit_image, DqoRastGrads* gr, void* ws, size_t ws_bytes, hipStream_t s,
                        const DqoShRest* pf, float* dL_drest) {
    (void)hit_image;  // the hit Gaussian is recovered from its list position kept in the image context
    (void)ws_bytes;
    if (p->P <= 0) return DQO_OK;
    const DqoView v = dqo_make_view(p, in);
    DqoGeomLayout g = dqo_geom_layout(ctx->geom, p->P);
    DqoImageLayout img = dqo_image_layout(ctx->image, p->W, p->H);
    DqoBinLayout bin = dqo_bin_layout(ctx->binning, ctx->inst_capacity,
                                      dqo_list_cap(ctx->inst_capacity, p->W, p->H, ctx->tile_bucket_capacity), ctx->tile_bucket_capacity);
    const int T = v.gx * v.gy;
    const int64_t cap = (int64_t)ctx->inst_capacity;
    DqoGradRec* recs = (DqoGradRec*)ws;
    uint8_t* valid = reinterpret_cast<uint8_t*>(bin.rec_valid);  // zeroed by the forward (bin_place_kernel)
    int rc = dqo_launch_blend_backward(v, g, img, bin, T, dL_dcolor, dL_ddepth, recs, valid, cap, dqo_tap_dev(ctx->loss_tap),
                                       dqo_gate_dev(ctx->object_gate), dqo_list_split(ctx), s);
    if (rc) return rc;
    // the per-Gaussian half: ONE kernel (record sum -> chain -> coalesced gradient rows, map_fused_tail.hip).
    // DqoRastCtx.frame_prezeroed given to THIS call: the per-Gaussian kernel, the last consumer of the frame's counters, clears them
    // (+ tile histogram and flags) for the next forward on the context and leaves the stamp — what dqo_rast_backward_adam always does.
    // Not with list_split: a second backward over the same forward (retain_graph) would find the long-list queue's counters gone.
    const bool clear = ctx->frame_prezeroed != 0 && dqo_list_split(ctx) == 0;
    return dqo_launch_gaussian_rows(v, g, in, recs, valid, cap, *gr, s, clear ? (uint32_t)dqo_frame_scalar_words(ctx) : 0u, img.tile_count,
                                    clear ? (uint32_t)((img.tile_flag + T) - img.tile_count) : 0u, pf != nullptr, dL_drest);
}
