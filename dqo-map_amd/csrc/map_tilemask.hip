// Tile-mask producers of the mapping loop for gfx950.
//
// Replaces the torch pooling chains of /root/reference/SLAM/utils.py:
//   pixelmask2tilemask :731-743 (pad + max_pool2d),  transmission2tilemask :752-763 (pad + avg_pool2d + threshold),
//   meanpool :720-729 / colorerror2tilemask :766-799 (pad + avg_pool2d; the top-k selection stays in the caller — except in
//   dqo_window_masks below, which selects in the kernel by a rule of its own),
// and the mask / colour-error images of evaluate_render_range, SLAM/multiprocess/mapper.py:930-988
//   (render_mask = T_map != 1;  color_error = sum_c |render - gt| with pixels whose rendered colour sums to 0 zeroed).
// The reference pads to a multiple of the stride with zeros and pools with count_include_pad: every 16x16 tile is divided
// by 256 whatever part of it lies inside the image.  One 256-thread block per tile, one pixel per thread: each image is read
// once, coalesced (64-byte rows), and reduced with a wave ballot / DPP sum + one LDS hop — the reference runs 4-7 eager
// kernels per mask and materialises the padded copies.
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// mode 0: mask_in != 0 (uint8 pixel mask).  mode 1: T_map != 1 (also written to mask_out).
__global__ __launch_bounds__(256) void tile_count_kernel(int W, int H, int gx, int mode, const uint8_t* __restrict__ mask_in,
                                                         const float* __restrict__ T_map, uint8_t* __restrict__ mask_out,
                                                         int32_t* __restrict__ tile_count, int32_t* __restrict__ total) {
    __shared__ int s_cnt[4];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const int px = (tile % gx) * DQO_TILE + (tid & 15), py = (tile / gx) * DQO_TILE + (tid >> 4);
    bool m = false;
    if (px < W && py < H) {
        const size_t pid = (size_t)py * W + px;
        if (mode == 0) {
            m = mask_in[pid] != 0;
        } else {
            m = T_map[pid] != 1.0f;
            if (mask_out) mask_out[pid] = m ? 1 : 0;
        }
    }
    const int c = (int)__popcll(__builtin_amdgcn_ballot_w64(m));
    if ((tid & 63) == 0) s_cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        const int n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        tile_count[tile] = n;
        if (total && n) atomicAdd(total, n);
    }
}

__global__ __launch_bounds__(256) void tile_color_error_kernel(int W, int H, int gx, const float* __restrict__ render,
                                                               const float* __restrict__ gt, float* __restrict__ err_px,
                                                               float* __restrict__ tile_sum) {
#pragma clang fp contract(off)
    __shared__ float s_sum[4];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const int px = (tile % gx) * DQO_TILE + (tid & 15), py = (tile / gx) * DQO_TILE + (tid >> 4);
    const size_t HW = (size_t)W * H;
    float e = 0.f;
    if (px < W && py < H) {
        const size_t pid = (size_t)py * W + px;
        const float r0 = render[pid], r1 = render[HW + pid], r2 = render[2 * HW + pid];
        e = (fabsf(r0 - gt[pid]) + fabsf(r1 - gt[HW + pid])) + fabsf(r2 - gt[2 * HW + pid]);  // torch.sum over the last dim
        if ((r0 + r1) + r2 == 0.f) e = 0.f;                                                   // mapper.py:955-956
        if (err_px) err_px[pid] = e;
    }
    const float s = wave_sum_f(e);
    if ((tid & 63) == 0) s_sum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) tile_sum[tile] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

// ---- dqo_window_masks: Mapping.evaluate_render_range (SLAM/multiprocess/mapper.py:930-988) for one frame of the window, in place ------
//   mode 0 (local, :983-985)   render_mask = T_map != 1;  tile_mask = float(count) / 256.f > tile_mask_ratio  (transmission2tilemask)
//   mode 1 (error, :947-978)   tile_mask = 1 on the k tiles with the largest colour error sum;  render_mask = tile_mask over its pixels
//   mode 2 (final, :980-982)   render_mask = T_map != 1;  tile_mask = 1  (the reference's None)
//   every mode                 ratio_out[0] = float(count of render_mask) / float(H * W)   (:987)
// One 256-thread block per tile, as above: the tile's word (mode 1: its error sum, tile_color_error_kernel's expression and order;
// otherwise its pixel count) goes to the workspace, and the block that takes the launch's last ticket (dqo_last_block) finishes the frame.
// Mode 1's selection is DEFINED here: the k largest by (sum descending, tile index ascending), the sum compared by its bit pattern as
// an unsigned integer (sums are non-negative; a NaN lies above every number).  The last block finds the k-th key by a radix select —
// four 8-bit digits from the top, a 256-bin LDS histogram of the keys that share the digits fixed so far — which also tells how many keys
// lie strictly above it, and then walks the tiles in index order: above the k-th key -> 1, equal to it -> 1 for the first k - above.
// Integer LDS atomics and integer sums only: the same bytes from run to run.  Every pass re-reads the keys from the workspace (L2): any
// tile count, 4 bytes x tiles x 5 passes — 64 KB at 1200 x 680.
// An overflowed render (header->overflow): nothing is read or written but the tickets, and ratio_out[0] = NaN.
struct WmWorkspace {
    int32_t* ticket;
    float* sums;      // [T] mode 1
    int32_t* counts;  // [T] modes 0, 2
};
inline DqoLayout<WmWorkspace> wm_ws(void* base, size_t T) {
    WmWorkspace w;
    DqoCarver k(base);
    w.ticket = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);  // = DQO_WINDOW_MASKS_SUMS_OFFSET
    w.sums = k.take<float>(4 * T);
    w.counts = k.take<int32_t>(4 * T);
    return {w, k.total()};
}

// the block's sum of one word per thread (every thread gets it); s_wave is free again after the call
__device__ __forceinline__ uint32_t wm_block_sum(uint32_t v, uint32_t* s_wave, int tid) {
    v = dqo_wave_sum_u32(v, tid & 63);
    __syncthreads();
    if ((tid & 63) == 0) s_wave[tid >> 6] = v;
    __syncthreads();
    return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ __launch_bounds__(256) void window_masks_kernel(int W, int H, int gx, int T, int mode, const float* __restrict__ T_map,
                                                           const float* __restrict__ render, const float* __restrict__ gt,
                                                           float tile_mask_ratio, int k, uint8_t* __restrict__ render_mask,
                                                           int32_t* __restrict__ tile_mask, float* __restrict__ ratio_out,
                                                           const DqoRastHeader* __restrict__ header, WmWorkspace w) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[4];
    __shared__ float s_sum[4];
    __shared__ uint32_t s_pick[2];
    __shared__ int s_last;
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool valid = header == nullptr || header->overflow == 0u;
    if (valid) {
        const int px = (tile % gx) * DQO_TILE + (tid & 15), py = (tile / gx) * DQO_TILE + (tid >> 4);
        const bool inside = px < W && py < H;
        const size_t pid = (size_t)py * W + px, HW = (size_t)W * H;
        if (mode == 1) {
            float e = 0.f;
            if (inside) {
                const float r0 = render[pid], r1 = render[HW + pid], r2 = render[2 * HW + pid];
                e = (fabsf(r0 - gt[pid]) + fabsf(r1 - gt[HW + pid])) + fabsf(r2 - gt[2 * HW + pid]);
                if ((r0 + r1) + r2 == 0.f) e = 0.f;  // mapper.py:955-956
            }
            const float s = dqo_wave_sum_xor(e, lane);
            if (lane == 0) s_sum[wave] = s;
            __syncthreads();
            if (tid == 0)
                __hip_atomic_store(&w.sums[tile], ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const bool m = inside && T_map[pid] != 1.0f;
            if (inside) render_mask[pid] = m ? 1 : 0;
            const int c = (int)__popcll(__builtin_amdgcn_ballot_w64(m));
            if (lane == 0) s_wave[wave] = (uint32_t)c;
            __syncthreads();
            if (tid == 0) {
                const int n = (int)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
                tile_mask[tile] = mode == 2 ? 1 : ((float)n / 256.f > tile_mask_ratio ? 1 : 0);  // SLAM/utils.py:752-762
                __hip_atomic_store(&w.counts[tile], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (!dqo_last_block(w.ticket, &s_last)) return;
    if (!valid) {
        if (tid == 0) ratio_out[0] = __int_as_float(0x7fc00000);
        return;
    }
    uint32_t pixels = 0;  // this thread's share of the render mask's pixel count
    if (mode != 1) {
        for (int i = tid; i < T; i += 256) pixels += (uint32_t)__hip_atomic_load(&w.counts[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const uint32_t* keys = reinterpret_cast<const uint32_t*>(w.sums);
        uint32_t kth = 0xffffffffu, need = 0u;  // k = 0: nothing lies above the k-th key, no tie is taken
        if (k > 0) {
            uint32_t prefix = 0u, rem = (uint32_t)k;  // rem of the keys that share `prefix` lie at or above the k-th key
            for (int shift = 24; shift >= 0; shift -= 8) {
                const uint32_t fixed = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
                s_hist[tid] = 0u;
                __syncthreads();
                for (int i = tid; i < T; i += 256) {
                    const uint32_t key = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((key & fixed) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                uint32_t above = 0u;  // keys with the prefix and a larger digit than this thread's
                for (int j = tid + 1; j < 256; j++) above += s_hist[j];
                if (above < rem && rem <= above + s_hist[tid]) s_pick[0] = (uint32_t)tid, s_pick[1] = rem - above;  // one thread
                __syncthreads();
                prefix |= s_pick[0] << shift, rem = s_pick[1];
            }
            kth = prefix, need = rem;  // k - need keys lie strictly above kth; the first `need` of its ties complete the k
        }
        uint32_t ties = 0u;  // ties in the tiles walked so far
        for (int base = 0; base < T; base += 256) {
            const int i = base + tid;
            const uint32_t key = i < T ? __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            const bool tie = i < T && key == kth;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(tie);
            __syncthreads();
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t rank = ties + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            for (int v = 0; v < wave; v++) rank += s_wave[v];
            ties += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
            if (i < T) {
                const bool sel = key > kth || (tie && rank < need);
                tile_mask[i] = sel ? 1 : 0;
                if (sel) pixels += (uint32_t)(min(DQO_TILE, W - (i % gx) * DQO_TILE) * min(DQO_TILE, H - (i / gx) * DQO_TILE));
            }
        }
    }
    const uint32_t total = wm_block_sum(pixels, s_wave, tid);
    if (tid == 0) ratio_out[0] = (float)total / (float)((int64_t)W * H);  // :987
}

// mode 1's render mask: every pixel gets its tile's word (mapper.py:970-978, the tile mask repeated 16 x 16 and cropped).  Four pixels
// per thread, one 32-bit store where the mask's address allows it.
__global__ __launch_bounds__(256) void window_mask_expand_kernel(int W, int64_t HW, int gx, const int32_t* __restrict__ tile_mask,
                                                                 uint8_t* __restrict__ render_mask, int words,
                                                                 const DqoRastHeader* __restrict__ header) {
    if (header != nullptr && header->overflow != 0u) return;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= HW) return;
    uint32_t packed = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t p = p0 + j;
        if (p < HW) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            packed |= (tile_mask[(y >> 4) * gx + (x >> 4)] != 0 ? 1u : 0u) << (8 * j);
        }
    }
    if (words && p0 + 3 < HW) {
        *reinterpret_cast<uint32_t*>(render_mask + p0) = packed;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p0 + j < HW) render_mask[p0 + j] = (uint8_t)(packed >> (8 * j));
    }
}

}  // namespace

static int dqo_launch_tile_count(int W, int H, int mode, const uint8_t* mask_in, const float* T_map, uint8_t* mask_out, int32_t* tile_count,
                                 int32_t* total, hipStream_t s) {
    const int gx = (W + DQO_TILE - 1) / DQO_TILE, gy = (H + DQO_TILE - 1) / DQO_TILE;
    if (total) {
        int rc = dqo_launch_zero_words(reinterpret_cast<uint32_t*>(total), 1, s);
        if (rc) return rc;
    }
    DQO_LAUNCH("tile_count_kernel", tile_count_kernel, dim3(gx * gy), dim3(256), s, W, H, gx, mode, mask_in, T_map, mask_out, tile_count,
               total);
    return DQO_OK;
}

static int dqo_launch_tile_color_error(int W, int H, const float* render, const float* gt, float* err_px, float* tile_sum, hipStream_t s) {
    const int gx = (W + DQO_TILE - 1) / DQO_TILE, gy = (H + DQO_TILE - 1) / DQO_TILE;
    DQO_LAUNCH("tile_color_error_kernel", tile_color_error_kernel, dim3(gx * gy), dim3(256), s, W, H, gx, render, gt, err_px, tile_sum);
    return DQO_OK;
}

static size_t dqo_window_masks_ws_bytes(int W, int H) {
    return wm_ws(nullptr, (size_t)((W + DQO_TILE - 1) / DQO_TILE) * ((H + DQO_TILE - 1) / DQO_TILE)).total;
}

static int dqo_launch_window_masks(int W, int H, int mode, const float* T_map, const float* render, const float* gt, float tile_mask_ratio, int k,
                                   uint8_t* render_mask, int32_t* tile_mask, float* ratio_out, const DqoRastHeader* header, void* ws, hipStream_t s) {
    const int gx = (W + DQO_TILE - 1) / DQO_TILE, gy = (H + DQO_TILE - 1) / DQO_TILE, T = gx * gy;
    const WmWorkspace w = wm_ws(ws, (size_t)T).w;
    DQO_LAUNCH("window_masks_kernel", window_masks_kernel, dim3(T), dim3(256), s, W, H, gx, T, mode, T_map, render, gt, tile_mask_ratio, k,
               render_mask, tile_mask, ratio_out, header, w);
    if (mode == 1) {
        const int64_t HW = (int64_t)W * H;
        const int words = (reinterpret_cast<uintptr_t>(render_mask) & 3u) == 0 ? 1 : 0;
        DQO_LAUNCH("window_mask_expand_kernel", window_mask_expand_kernel, dim3((unsigned)((HW + 1023) / 1024)), dim3(256), s, W, HW, gx,
                   tile_mask, render_mask, words, header);
    }
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

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

}  // extern "C"
