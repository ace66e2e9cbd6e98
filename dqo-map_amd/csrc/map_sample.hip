// Map growth for gfx950, the first statement: Mapping.temp_points_init (SLAM/multiprocess/mapper.py:1231-1347) — from one RGB-D frame and
// a render of the map to the candidate rows of FusedMapper.grow(new=...).  include/dqo_raster.h (DqoGrowthSample) states the contract.
//
// The reference draws k of a mask's n pixels with the first k of a CPU torch.randperm (SLAM/utils.py:185).  Here every pixel of the mask
// gets a 32-bit key (dqo_sample_hash.h) and the k smallest (key, pixel) pairs are chosen: the same distribution, a pure function of the
// arguments.  The k-th smallest key is found by a radix select over three digits (11 + 11 + 10 bits), never by a sort (dqo_select.h: the
// digit, the flush, the last block's pick and its single-word ticket, shared with map_densify.hip; this file keeps its two-draw histogram):
//
//     zero            the workspace's head (histograms, counts, tickets)
//     pixel pass      both masks in registers, their counts before and after sample_pixels' in-place strip, one flag byte per pixel,
//                     histogram of the keys' top digit; the last block forms both k and picks each draw's bucket
//     refine x 2      histogram of the next digit over the pixels inside the bucket; the last block picks the next bucket.  After the
//                     second one a draw has its threshold key t and the number r of pixels with key == t it takes (lowest pixels first)
//     rank pass       per block: pixels with key == t; the last block scans them over the blocks in index order (dqo_reduce.h's
//                     dqo_scan_block_counts, as in the rows pass: [blocks][2], one column per draw)
//     rows pass       per block: chosen pixels (key < t, or key == t among the first r) whose normalised normal does not sum to 0
//                     (gaussian_pointcloud.py:457); the last block scans them in index order and writes the header
//     emit pass       ordered compaction by ballot and prefix: rows in ascending pixel index, draw A's before draw B's
//
// Integer atomics only (histograms, counts, tickets): their order cannot reach the output.  No float is ever accumulated across threads.
// A block's histogram is built in LDS and only its non-zero bins go to memory, 2048 different addresses per draw; the five counts are
// reduced per block first (one atomic per block and count, a few hundred to a word per frame — no need to spread them over lines).
// This file is compiled with -ffp-contract=off: every float statement below is the reference's, rounded where torch rounds it.
#include "dqo_common.h"
#include "dqo_reduce.h"
#include "dqo_sample_hash.h"
#include "dqo_select.h"

namespace {

enum {
    SP_THREADS = 256,
    SP_PPT = 2,                      // pixels per thread: pixel = block * SP_PIX + j * 256 + thread
    SP_PIX = SP_THREADS * SP_PPT,
    // words of the workspace's head (zeroed by the first launch of every call)
    SP_HIST = 0,                     // [2 draws][3 levels][DQO_SELECT_BINS]
    SP_CNT = 2 * 3 * DQO_SELECT_BINS,  // [5] A before / after the strip, B before / after, B's pixels that leave if trans is not stripped
    SP_TICKET = SP_CNT + 8,          // [8] one per kernel that ends in a last block: five kernels, words 0..4
    SP_STATE = SP_TICKET + 8,        // [2 draws][8]: 0 key prefix / threshold t, 1 k left / r, 2 clamped k, 3 rows of the draw
    SP_HEAD_WORDS = SP_STATE + 16 + 32,
    // flag byte of a pixel
    SP_IN_A = 1, SP_IN_B = 2, SP_ROW_A = 4, SP_ROW_B = 8,
};
static_assert(SP_HEAD_WORDS * 4 % 256 == 0, "workspace head layout");

struct SpWorkspace {
    uint32_t* head;
    uint32_t* blk_eq;    // [blocks][2] pixels with key == t, then their exclusive prefix over the blocks
    uint32_t* blk_rows;  // [blocks][2] rows of the block, then their exclusive prefix
    uint8_t* flags;      // [H * W]
};

__host__ __device__ inline size_t sp_blocks(int64_t HW) { return (size_t)((HW + SP_PIX - 1) / SP_PIX); }

// the head words | blk_eq | blk_rows | flags
inline DqoLayout<SpWorkspace> sp_workspace(void* base, int64_t HW) {
    SpWorkspace w;
    DqoCarver k(base);
    w.head = k.take_raw<uint32_t>(SP_HEAD_WORDS * 4);
    w.blk_eq = k.take<uint32_t>(sp_blocks(HW) * 2 * sizeof(uint32_t));
    w.blk_rows = k.take<uint32_t>(sp_blocks(HW) * 2 * sizeof(uint32_t));
    w.flags = k.take<uint8_t>((size_t)HW);
    return {w, k.total()};
}

struct SpKeys {
    uint32_t seed_word, draw_word[2], key_mask;
};

// draw d's histogram of a level in the workspace's head
__device__ __forceinline__ uint32_t* sp_hist(uint32_t* head, int level, int d) { return head + SP_HIST + (d * 3 + level) * DQO_SELECT_BINS; }

// The block's histogram of one digit, both draws: LDS first, its non-zero bins to memory.  in[d][j]: pixel j of this thread counts for draw d.
__device__ __forceinline__ void sp_histogram(uint32_t* head, int level, const uint32_t key[2][SP_PPT], const bool in[2][SP_PPT]) {
    __shared__ uint32_t s_hist[2 * DQO_SELECT_BINS];
    for (int i = threadIdx.x; i < 2 * DQO_SELECT_BINS; i += SP_THREADS) s_hist[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 2; d++)
#pragma unroll
        for (int j = 0; j < SP_PPT; j++)
            if (in[d][j]) dqo_select_count(s_hist + d * DQO_SELECT_BINS, key[d][j], level);
    __syncthreads();
    for (int d = 0; d < 2; d++) dqo_select_flush(s_hist + d * DQO_SELECT_BINS, sp_hist(head, level, d));
}

// The last block picks the level's bucket of both draws (dqo_select.h: state[0] the key prefix, state[1] the rank left)
__device__ __forceinline__ void sp_select(uint32_t* head, int level) {
    for (int d = 0; d < 2; d++) dqo_select_pick(sp_hist(head, level, d), head + SP_STATE + 8 * d, level);
}

// Rank of this thread's pixel j among the block's pixels with pred set, in pixel order (j, wave, lane), and the block's count.
__device__ __forceinline__ void sp_block_rank(const bool pred[SP_PPT], uint32_t rank[SP_PPT], uint32_t& total, uint32_t* s_seg /* [8] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t below[SP_PPT];
    __syncthreads();  // (s_seg may still be read by the previous call)
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const unsigned long long b = __ballot(pred[j]);
        below[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_seg[j * 4 + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = 0u;
#pragma unroll
    for (int s = 0; s < SP_PPT * 4; s++) {
#pragma unroll
        for (int j = 0; j < SP_PPT; j++)
            if (s == j * 4 + wave) rank[j] = run + below[j];
        run += s_seg[s];
    }
    total = run;
}

// |v| as torch.norm(p=2, dim=-1) rounds it on three components: the squares enter one fused multiply-add chain
__device__ __forceinline__ float sp_norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

// add_empty_points' normal (gaussian_pointcloud.py:455-457): normalised, and whether the row stays
__device__ __forceinline__ bool sp_unit_normal(const float* __restrict__ normal, int64_t p, float n[3]) {
    const float x = normal[3 * p], y = normal[3 * p + 1], z = normal[3 * p + 2];
    const float den = sp_norm3(x, y, z) + 1e-8f;  // :455-456
    n[0] = x / den, n[1] = y / den, n[2] = z / den;
    return ((n[0] + n[1]) + n[2]) != 0.f;  // :457
}

// ---- the pixel pass (mapper.py:1234-1235, 1251-1262, 1292-1327; utils.py:169-174) ------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void sample_pixel_kernel(DqoGrowthSample a, SpWorkspace w, SpKeys keys, int64_t HW) {
    __shared__ uint32_t s_cnt[5];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 5) s_cnt[tid] = 0u;
    __syncthreads();
    uint32_t key[2][SP_PPT];
    bool in[2][SP_PPT];
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + tid;
        bool a_pre = false, a_post = false, b_pre = false, b_post = false, b_leaves = false;
        if (p < HW) {
            const float d = a.depth[p];
            const bool dpos = d > 0.f;
            // sample_pixels' in-place strip: the normal's (utils.py:169-170) and the instance colour's (:172-174) components sum to 0
            bool keep = ((a.normal[3 * p] + a.normal[3 * p + 1]) + a.normal[3 * p + 2]) != 0.f;
            if (a.instance != nullptr) keep = keep && ((a.instance[3 * p] + a.instance[3 * p + 1]) + a.instance[3 * p + 2]) != 0.f;
            if (a.first_frame) {
                a_pre = dpos;  // mapper.py:1235
                a_post = a_pre && keep;
            } else {
                const float T = a.T[p];
                a_pre = T > a.add_transmission_thres && dpos;  // :1251-1253
                a_post = a_pre && keep;                         // (what the call at :1269 leaves in the mask)
                const float depth_error = fabsf(d - a.render_depth[p]);  // :1292-1294
                const float color_error = ((fabsf(a.color[3 * p] - a.render_color[p]) + fabsf(a.color[3 * p + 1] - a.render_color[HW + p])) +
                                           fabsf(a.color[3 * p + 2] - a.render_color[2 * HW + p])) / 3.f;  // :1295-1297
                const bool depth_mask = depth_error > a.add_depth_thres && dpos && a.depth_index[p] > -1;   // :1300-1304
                const bool color_mask = color_error > a.add_color_thres && dpos && T < a.add_transmission_thres;  // :1305-1309
                const bool err = color_mask || depth_mask;  // :1321
                b_pre = err && !a_post;                     // :1326, trans as the first call left it
                b_leaves = err && a_pre && !keep;           // ... which is untouched when that call had k == 0 (utils.py:155-156)
                b_post = b_pre && keep;                     // (the same pixels either way)
            }
        }
        in[0][j] = a_post, in[1][j] = b_post;
        key[0][j] = dqo_sample_key(keys.seed_word, keys.draw_word[0], (uint32_t)p, keys.key_mask);
        key[1][j] = dqo_sample_key(keys.seed_word, keys.draw_word[1], (uint32_t)p, keys.key_mask);
        if (p < HW) w.flags[p] = (uint8_t)((a_post ? SP_IN_A : 0) | (b_post ? SP_IN_B : 0));
        const bool c[5] = {a_pre, a_post, b_pre, b_post, b_leaves};
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int n = __popcll(__ballot(c[k]));
            if (lane == 0 && n > 0) atomicAdd(&s_cnt[k], (uint32_t)n);
        }
    }
    __syncthreads();
    if (tid < 5 && s_cnt[tid] != 0u) atomicAdd(&w.head[SP_CNT + tid], s_cnt[tid]);
    sp_histogram(w.head, 0, key, in);
    if (!dqo_single_ticket_last_block(&w.head[SP_TICKET + 0])) return;
    if (tid == 0) {
        const uint32_t a_pre = dqo_ld_u32(&w.head[SP_CNT + 0]), a_post = dqo_ld_u32(&w.head[SP_CNT + 1]), b_post = dqo_ld_u32(&w.head[SP_CNT + 3]);
        uint32_t b_pre = dqo_ld_u32(&w.head[SP_CNT + 2]);
        int64_t k_a, k_b = 0;
        if (a.first_frame) {
            k_a = a.uniform_sample_num;  // mapper.py:1242
        } else {
            const float ratio = (float)a_pre / (float)HW;                                            // :1254-1256
            k_a = (int64_t)((a.transmission_sample_ratio * ratio) * (float)a.uniform_sample_num);  // :1258-1262, devI truncates
            if (k_a == 0) b_pre -= dqo_ld_u32(&w.head[SP_CNT + 4]);
            k_b = (int64_t)((float)b_pre * a.error_sample_ratio);  // :1327
        }
        k_a = k_a < 0 ? 0 : k_a > (int64_t)a_post ? (int64_t)a_post : k_a;  // utils.py:176-177
        k_b = k_b < 0 ? 0 : k_b > (int64_t)b_post ? (int64_t)b_post : k_b;
        dqo_st_u32(&w.head[SP_STATE + 1], (uint32_t)k_a), dqo_st_u32(&w.head[SP_STATE + 2], (uint32_t)k_a);
        dqo_st_u32(&w.head[SP_STATE + 8 + 1], (uint32_t)k_b), dqo_st_u32(&w.head[SP_STATE + 8 + 2], (uint32_t)k_b);
        a.header[0] = (int32_t)a_pre, a.header[1] = (int32_t)a_post, a.header[2] = (int32_t)b_pre, a.header[3] = (int32_t)b_post;
        a.header[4] = (int32_t)k_a, a.header[5] = (int32_t)k_b;
        __threadfence();
    }
    __syncthreads();
    sp_select(w.head, 0);
}

// a pixel's flags and keys as the later passes need them
__device__ __forceinline__ void sp_load_pixels(const SpWorkspace& w, const SpKeys& keys, int64_t HW, uint8_t flag[SP_PPT],
                                               uint32_t key[2][SP_PPT]) {
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + threadIdx.x;
        flag[j] = p < HW ? w.flags[p] : (uint8_t)0;
        key[0][j] = dqo_sample_key(keys.seed_word, keys.draw_word[0], (uint32_t)p, keys.key_mask);
        key[1][j] = dqo_sample_key(keys.seed_word, keys.draw_word[1], (uint32_t)p, keys.key_mask);
    }
}

// ---- the refine passes: the next digit, over the pixels of the bucket picked so far ------------------------------------------------------
template <int LEVEL>
__global__ __launch_bounds__(SP_THREADS) void sample_refine_kernel(SpWorkspace w, SpKeys keys, int64_t HW) {
    uint8_t flag[SP_PPT];
    uint32_t key[2][SP_PPT];
    bool in[2][SP_PPT];
    sp_load_pixels(w, keys, HW, flag, key);
    const uint32_t prefix[2] = {w.head[SP_STATE + 0], w.head[SP_STATE + 8]};
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        in[0][j] = (flag[j] & SP_IN_A) && dqo_select_in_bucket(key[0][j], prefix[0], LEVEL);
        in[1][j] = (flag[j] & SP_IN_B) && dqo_select_in_bucket(key[1][j], prefix[1], LEVEL);
    }
    sp_histogram(w.head, LEVEL, key, in);
    if (!dqo_single_ticket_last_block(&w.head[SP_TICKET + LEVEL])) return;
    sp_select(w.head, LEVEL);
}

// ---- the rank pass: ties at the threshold key go to the lowest pixels, so a block needs the ties in the blocks before it ----------------
__global__ __launch_bounds__(SP_THREADS) void sample_rank_kernel(SpWorkspace w, SpKeys keys, int64_t HW) {
    __shared__ uint32_t s_seg[SP_PPT * 4], s_wave[4];
    uint8_t flag[SP_PPT];
    uint32_t key[2][SP_PPT], rank[SP_PPT], total;
    bool eq[SP_PPT];
    sp_load_pixels(w, keys, HW, flag, key);
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const uint32_t t = w.head[SP_STATE + 8 * d];
#pragma unroll
        for (int j = 0; j < SP_PPT; j++) eq[j] = (flag[j] & (d == 0 ? SP_IN_A : SP_IN_B)) && key[d][j] == t;
        sp_block_rank(eq, rank, total, s_seg);
        if (threadIdx.x == 0) dqo_st_u32(&w.blk_eq[2 * (size_t)blockIdx.x + d], total);
    }
    if (!dqo_single_ticket_last_block(&w.head[SP_TICKET + 3])) return;
    for (int d = 0; d < 2; d++) dqo_scan_block_counts<uint32_t, 1>(w.blk_eq + d, gridDim.x, 2, s_wave);
}

// ---- the rows pass: which chosen pixels become rows (gaussian_pointcloud.py:455-460), and how many come before each block ---------------
__global__ __launch_bounds__(SP_THREADS) void sample_rows_kernel(DqoGrowthSample a, SpWorkspace w, SpKeys keys, int64_t HW) {
    __shared__ uint32_t s_seg[SP_PPT * 4], s_wave[4];
    uint8_t flag[SP_PPT];
    uint32_t key[2][SP_PPT], rank[SP_PPT], total;
    bool eq[SP_PPT], row[SP_PPT];
    sp_load_pixels(w, keys, HW, flag, key);
    bool stays[SP_PPT];
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + threadIdx.x;
        float n[3];
        stays[j] = (flag[j] & (SP_IN_A | SP_IN_B)) ? sp_unit_normal(a.normal, p, n) : false;
    }
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const uint32_t in_bit = d == 0 ? SP_IN_A : SP_IN_B, row_bit = d == 0 ? SP_ROW_A : SP_ROW_B;
        const uint32_t t = w.head[SP_STATE + 8 * d], r = w.head[SP_STATE + 8 * d + 1];
        const uint32_t ties_before = w.blk_eq[2 * (size_t)blockIdx.x + d];
#pragma unroll
        for (int j = 0; j < SP_PPT; j++) eq[j] = (flag[j] & in_bit) && key[d][j] == t;
        sp_block_rank(eq, rank, total, s_seg);
#pragma unroll
        for (int j = 0; j < SP_PPT; j++) {
            const bool chosen = (flag[j] & in_bit) && (key[d][j] < t || (eq[j] && ties_before + rank[j] < r));
            row[j] = chosen && stays[j];
            if (row[j]) flag[j] |= (uint8_t)row_bit;
        }
        sp_block_rank(row, rank, total, s_seg);
        if (threadIdx.x == 0) dqo_st_u32(&w.blk_rows[2 * (size_t)blockIdx.x + d], total);
    }
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + threadIdx.x;
        if (p < HW && (flag[j] & (SP_ROW_A | SP_ROW_B))) w.flags[p] = flag[j];
    }
    if (!dqo_single_ticket_last_block(&w.head[SP_TICKET + 4])) return;
    const uint32_t rows_a = dqo_scan_block_counts<uint32_t, 1>(w.blk_rows, gridDim.x, 2, s_wave);
    const uint32_t rows_b = dqo_scan_block_counts<uint32_t, 1>(w.blk_rows + 1, gridDim.x, 2, s_wave);
    if (threadIdx.x == 0) {
        const uint64_t rows = (uint64_t)rows_a + rows_b;
        dqo_st_u32(&w.head[SP_STATE + 3], rows_a);
        a.header[6] = (int32_t)(rows > (uint64_t)a.capacity ? (uint64_t)a.capacity : rows);
        a.header[7] = rows > (uint64_t)a.capacity ? 1 : 0;
    }
}

// ---- the emit pass (gaussian_pointcloud.py:455-516) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void sample_emit_kernel(DqoGrowthSample a, SpWorkspace w, int64_t HW) {
    __shared__ uint32_t s_seg[SP_PPT * 4];
    uint8_t flag[SP_PPT];
    uint32_t rank[SP_PPT], total;
    bool row[SP_PPT];
#pragma unroll
    for (int j = 0; j < SP_PPT; j++) {
        const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + threadIdx.x;
        flag[j] = p < HW ? w.flags[p] : (uint8_t)0;
    }
    const uint32_t rows_a = w.head[SP_STATE + 3];
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const uint32_t base = (d == 0 ? 0u : rows_a) + w.blk_rows[2 * (size_t)blockIdx.x + d];
#pragma unroll
        for (int j = 0; j < SP_PPT; j++) row[j] = (flag[j] & (d == 0 ? SP_ROW_A : SP_ROW_B)) != 0;
        sp_block_rank(row, rank, total, s_seg);
#pragma unroll
        for (int j = 0; j < SP_PPT; j++) {
            const uint64_t q = (uint64_t)base + rank[j];
            if (!row[j] || q >= (uint64_t)a.capacity) continue;  // rows beyond the capacity are never written
            const int64_t p = (int64_t)blockIdx.x * SP_PIX + j * SP_THREADS + threadIdx.x;
            float n[3];
            sp_unit_normal(a.normal, p, n);
            a.pixel[q] = (int32_t)p;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                a.xyz[3 * q + c] = a.vertex[3 * p + c];
                a.out_normal[3 * q + c] = n[c];
                a.scales[3 * q + c] = 1e-6f;  // :468
                a.shs[(size_t)q * a.M * 3 + c] = (a.color[3 * p + c] - 0.5f) / 0.28209479177387814f;  // RGB2SH, utils/sh_utils.py:123-124
            }
            for (int m = 3; m < 3 * a.M; m++) a.shs[(size_t)q * a.M * 3 + m] = 0.f;  // :463-466
            a.opacity[q] = a.init_opacity;  // :481-483 (activated)
            if (a.obj_id != nullptr && a.instance != nullptr) a.obj_id[q] = (int32_t)(a.instance[3 * p] * 255.f);  // :497
            float rot[4] = {1.f, 0.f, 0.f, 0.f};  // :475-476
            if (!a.identity_rotation) {
                // compute_rot(z_axis, normal), utils.py:246-251: torch.cross written out, the products with 0 and 1 kept (signed zeros)
                const float zx = 0.f, zy = 0.f, zz = 1.f;
                float ax = zy * n[2] - zz * n[1], ay = zz * n[0] - zx * n[2], az = zx * n[1] - zy * n[0];  // :247
                float den = sp_norm3(ax, ay, az) + 1e-8f;                                                   // :248
                ax = ax / den, ay = ay / den, az = az / den;
                const float angle = acosf(((zx * n[0] + zy * n[1]) + zz * n[2]));  // :249
                den = sp_norm3(ax, ay, az) + 1e-8f;  // quaternion_from_axis_angle, utils/general_utils.py:186
                ax = ax / den, ay = ay / den, az = az / den;
                const float half = angle / 2.f;  // :187
                const float s = sinf(half);
                rot[0] = cosf(half), rot[1] = ax * s, rot[2] = ay * s, rot[3] = az * s;  // :188-190
            }
#pragma unroll
            for (int c = 0; c < 4; c++) a.rotations[4 * q + c] = rot[c];
        }
    }
}

}  // namespace

static size_t dqo_sample_ws_bytes(int64_t HW) { return sp_workspace(nullptr, HW).total; }

static int dqo_launch_growth_sample(const DqoGrowthSample* a, hipStream_t s) {
    const int64_t HW = (int64_t)a->W * a->H;
    const SpWorkspace w = sp_workspace(a->workspace, HW).w;
    SpKeys keys;
    keys.seed_word = dqo_sample_seed_word(a->seed);
    keys.draw_word[0] = dqo_sample_draw_word(keys.seed_word, a->first_frame ? 0u : 1u);
    keys.draw_word[1] = dqo_sample_draw_word(keys.seed_word, 2u);
    keys.key_mask = a->key_bits >= 32 ? 0xffffffffu : ((1u << a->key_bits) - 1u);
    const dim3 grid((unsigned)sp_blocks(HW)), block(SP_THREADS);
    const int rc = dqo_launch_zero_words(w.head, SP_HEAD_WORDS, s);
    if (rc) return rc;
    DQO_LAUNCH("sample_pixel_kernel", sample_pixel_kernel, grid, block, s, *a, w, keys, HW);
    DQO_LAUNCH("sample_refine_kernel<1>", sample_refine_kernel<1>, grid, block, s, w, keys, HW);
    DQO_LAUNCH("sample_refine_kernel<2>", sample_refine_kernel<2>, grid, block, s, w, keys, HW);
    DQO_LAUNCH("sample_rank_kernel", sample_rank_kernel, grid, block, s, w, keys, HW);
    DQO_LAUNCH("sample_rows_kernel", sample_rows_kernel, grid, block, s, *a, w, keys, HW);
    DQO_LAUNCH("sample_emit_kernel", sample_emit_kernel, grid, block, s, *a, w, HW);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

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
    DQO_CHECK_WS("growth sample", a->workspace, a->workspace_bytes, dqo_sample_ws_bytes((int64_t)a->W * a->H));
    return dqo_launch_growth_sample(a, (hipStream_t)stream);
}

}  // extern "C"
