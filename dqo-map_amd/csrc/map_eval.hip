// Keyframe evaluation for gfx950: the numbers eval_picture reports for a rendered frame (SLAM/eval.py:38-188, called from slam.py:155,
// 184 and metric.py), in ONE pass over the frame and ONE launch, nothing read back:
//
//     psnr_value = psnr(gt_image, image).mean()                          :63      utils/loss_utils.py:23-25, per channel, then the mean
//     color_loss = l1_loss(gt_image, image)                              :70      utils/loss_utils.py:27-29
//     valid_range_mask = (gt_depth > min_depth) & (gt_depth < max_depth) :116-117 gt_depth = 0 outside the range
//     invalid_depth_mask = (index == -1) | (gt_depth == 0)               :120-123
//     valid_pixel_ratio = valid_depth_mask.sum() / pixel_num             :124-125
//     depth_loss = l1_loss(depth[valid], gt_depth[valid])                :126     NaN when nothing is valid (the mean of an empty selection)
//
// The reference forms every difference and every mean in float32 with torch's summation tree.  Here the differences of the float inputs
// are formed in double (exact: a float difference, its square and its magnitude all fit) and summed in double, so what remains is the order
// of the additions — at most H W 2^-53 relative — and one rounding to float32 per output.
//
// No float or double atomic anywhere: a thread adds its EV_PIX pixels in order, and the rest is dqo_reduce.h — a wave its lanes by the xor
// butterfly, a block its waves in order, and the block that takes the launch's last integer ticket adds the blocks' partials IN
// BLOCK-INDEX ORDER and writes the row: the same bits from run to run, and an entry without a zero fill that is capturable in a hipGraph.
#include <algorithm>

#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

enum {
    EV_PIX = 4,                              // pixels per thread: a 1200 x 680 frame is 797 blocks — every CU busy, and a short last sum
    EV_SUMS = 6,                             // squared colour error r, g, b | absolute colour error | absolute depth error | valid pixels
    EV_STRIDE = 8,                           // doubles per block partial: one 64-byte line
    EV_STAGE = 256,                          // partials staged through LDS at a time by the last block
};

struct EvWorkspace {
    int32_t* ticket;
    double* partial;  // [blocks][EV_STRIDE]
};

inline size_t ev_blocks(int64_t HW) { return (size_t)((HW + 256 * EV_PIX - 1) / (256 * EV_PIX)); }

// the head of every workspace of this file: the ticket words | `lines` partial lines of `stride` doubles
inline EvWorkspace ev_take(DqoCarver& k, size_t lines, size_t stride) {
    EvWorkspace w;
    w.ticket = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.partial = k.take<double>(lines * stride * sizeof(double));
    return w;
}
// dqo_eval_picture's workspace: that head alone
inline DqoLayout<EvWorkspace> ev_ws(void* base, int64_t HW) {
    DqoCarver k(base);
    const EvWorkspace w = ev_take(k, ev_blocks(HW), EV_STRIDE);
    return {w, k.total()};
}

__global__ __launch_bounds__(256) void eval_picture_kernel(int64_t HW, const float* __restrict__ render, const float* __restrict__ gt_color,
                                                           const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                           const int32_t* __restrict__ depth_index, float min_depth, float max_depth,
                                                           const DqoRastHeader* __restrict__ header, EvWorkspace w, float* __restrict__ out) {
    __shared__ double s_stage[EV_STAGE * EV_STRIDE];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    double a[EV_SUMS];
#pragma unroll
    for (int q = 0; q < EV_SUMS; q++) a[q] = 0.0;
#pragma unroll
    for (int k = 0; k < EV_PIX; k++) {
        const int64_t i = ((int64_t)blockIdx.x * EV_PIX + k) * 256 + tid;
        if (i < HW) {
            const double dr = (double)gt_color[i] - (double)render[i];
            const double dg = (double)gt_color[HW + i] - (double)render[HW + i];
            const double db = (double)gt_color[2 * HW + i] - (double)render[2 * HW + i];
            a[0] += dr * dr, a[1] += dg * dg, a[2] += db * db;
            a[3] += (fabs(dr) + fabs(dg)) + fabs(db);
            const float gd = gt_depth[i];
            if (depth_index[i] != -1 && gd > min_depth && gd < max_depth) {  // (a NaN target is outside the range, as in the reference)
                a[4] += fabs((double)depth[i] - (double)gd);
                a[5] += 1.0;
            }
        }
    }
    dqo_block_partial<EV_SUMS, EV_STRIDE>(a, s_stage, w.partial);
    if (!dqo_last_block(w.ticket, &s_last)) return;
    const double total = dqo_fold_partials<EV_SUMS, EV_STRIDE, EV_STAGE>(w.partial, 0, (int)gridDim.x, s_stage);
    if (tid < EV_SUMS) s_stage[tid] = total;
    __syncthreads();
    if (tid != 0) return;
    if (header != nullptr && header->overflow != 0u) {  // the render outgrew its context: its images are invalid, and so is the row
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = __int_as_float(0x7fc00000);
        return;
    }
    const double n = (double)HW;
    double psnr = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double mse = s_stage[c] / n;
        out[5 + c] = (float)mse;
        psnr += 20.0 * log10(1.0 / sqrt(mse));  // (mse = 0: 1 / 0 = inf, log10(inf) = inf — the reference's value)
    }
    out[0] = (float)(psnr / 3.0);
    out[1] = (float)(s_stage[3] / (3.0 * n));
    out[2] = (float)(s_stage[4] / s_stage[5]);  // (nothing valid: 0 / 0 = NaN — torch's mean of an empty selection)
    out[3] = (float)s_stage[5] / (float)n;      // valid_depth_mask.sum() / pixel_num: torch divides the two integers as float32
}


// ---- geometry evaluation: eval_pcd's numbers (SLAM/eval.py:190-282) from the two nearest-neighbour searches ---------------------------
//     completion_ratio / accuracy_ratio   :190-201   np.mean(distances < dist_th)        -> R / P of :264-268, F1 :269
//     accuracy / completion               :204-215   np.mean(distances)                  -> cm, :273-274
//     chamfer_distance                    :218-226   the two means added (metres; the reference prints it, :253-254)
// The reference builds a KDTree and queries it anew for every one of these statements; here d2_rec (every reconstructed point to its
// nearest ground-truth point) and d2_gt (the other way round) come from two dqo_nn1 searches, and ONE launch reduces both: per kept row
// sqrt((double)d2) and, per threshold, (double)d2 < (double)th * (double)th — both sides exact in double, so a count is an exact function
// of the search's bits (the reference's strict '<' on distances).  Sums as in eval_picture_kernel: a thread's rows in order, then
// dqo_reduce.h, the last block folding the partials of each side on their own.
enum {
    PC_ROWS = 4,           // rows of a set per thread
    PC_THRES = 8,          // thresholds at most
    PC_SUMS = 2 + PC_THRES,  // distance | kept rows | rows under threshold t
    PC_STRIDE = 16,        // doubles per block partial: two 64-byte lines
    PC_STAGE = 128,        // partials staged through LDS at a time by the last block
    PC_SLOTS = 32,         // floats of a table row
};

struct PcThres {
    float th[PC_THRES];
};

inline size_t pc_blocks(int n) { return ((size_t)n + 256 * PC_ROWS - 1) / (256 * PC_ROWS); }

// one table row from the PC_SUMS sums of each side (an object's, or the whole sets'); a side without a kept row: a row of NaN
__device__ __forceinline__ void pc_table_row(const double* rec, const double* gt, int n_thres, float* __restrict__ out) {
    const float nan = __int_as_float(0x7fc00000);
    for (int q = 0; q < PC_SLOTS; q++) out[q] = nan;
    if (rec[1] == 0.0 || gt[1] == 0.0) return;
    const double acc = rec[0] / rec[1], comp = gt[0] / gt[1];
    out[0] = (float)(100.0 * acc);   // :273 (cm)
    out[1] = (float)(100.0 * comp);  // :274
    out[2] = (float)(acc + comp);    // :225 (metres)
    out[3] = (float)n_thres;
    for (int t = 0; t < n_thres; t++) {
        const double P = 100.0 * (rec[2 + t] / rec[1]), R = 100.0 * (gt[2 + t] / gt[1]);  // :264-268
        out[4 + 3 * t] = (float)P;
        out[5 + 3 * t] = (float)R;
        out[6 + 3 * t] = (float)(2.0 * P * R / (P + R));  // :269 (P + R = 0: 0 / 0 = NaN, numpy's value)
    }
}

// blocks [0, blocks_rec) reduce d2_rec, the rest d2_gt
__global__ __launch_bounds__(256) void eval_pcd_kernel(int n_rec, const float* __restrict__ d2_rec, const uint8_t* __restrict__ rec_keep, int n_gt,
                                                       const float* __restrict__ d2_gt, const uint8_t* __restrict__ gt_keep, int n_thres,
                                                       PcThres thres, int blocks_rec, EvWorkspace w, float* __restrict__ out) {
    __shared__ double s_stage[PC_STAGE * PC_STRIDE];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const bool rec_side = (int)blockIdx.x < blocks_rec;
    const int n = rec_side ? n_rec : n_gt, block = rec_side ? (int)blockIdx.x : (int)blockIdx.x - blocks_rec;
    const float* __restrict__ d2 = rec_side ? d2_rec : d2_gt;
    const uint8_t* __restrict__ keep = rec_side ? rec_keep : gt_keep;
    double th2[PC_THRES];
#pragma unroll
    for (int t = 0; t < PC_THRES; t++) th2[t] = (double)thres.th[t] * (double)thres.th[t];
    double a[PC_SUMS];
#pragma unroll
    for (int q = 0; q < PC_SUMS; q++) a[q] = 0.0;
#pragma unroll
    for (int k = 0; k < PC_ROWS; k++) {
        const int64_t i = ((int64_t)block * PC_ROWS + k) * 256 + tid;
        if (i < n && (keep == nullptr || keep[i] != 0)) {
            const double v = (double)d2[i];
            a[0] += sqrt(v);
            a[1] += 1.0;
#pragma unroll
            for (int t = 0; t < PC_THRES; t++)
                if (t < n_thres && v < th2[t]) a[2 + t] += 1.0;
        }
    }
    dqo_block_partial<PC_SUMS, PC_STRIDE>(a, s_stage, w.partial);
    if (!dqo_last_block(w.ticket, &s_last)) return;
    const double tot_rec = dqo_fold_partials<PC_SUMS, PC_STRIDE, PC_STAGE>(w.partial, 0, blocks_rec, s_stage);
    const double tot_gt = dqo_fold_partials<PC_SUMS, PC_STRIDE, PC_STAGE>(w.partial, blocks_rec, (int)gridDim.x, s_stage);
    if (tid < PC_SUMS) s_stage[tid] = tot_rec, s_stage[PC_STRIDE + tid] = tot_gt;
    __syncthreads();
    if (tid == 0) pc_table_row(s_stage, s_stage + PC_STRIDE, n_thres, out);
}

struct PcWorkspace {
    EvWorkspace ev;
    float *d2_rec, *d2_gt;
    void* nn1;
    size_t total;
};
inline PcWorkspace pc_ws(void* base, int n_gt, int n_rec) {
    PcWorkspace w;
    DqoCarver k(base);
    w.ev = ev_take(k, pc_blocks(n_rec) + pc_blocks(n_gt) + 1, PC_STRIDE);
    w.d2_rec = k.take<float>(4 * (size_t)n_rec);
    w.d2_gt = k.take<float>(4 * (size_t)n_gt);
    w.nn1 = k.take_raw(std::max(dqo_nn1_ws_bytes(n_rec, n_gt), dqo_nn1_ws_bytes(n_gt, n_rec)));  // the two searches run one after the other
    w.total = k.total();
    return w;
}

// ---- per-object geometry evaluation: eval_pcd's row for each of up to 64 objects (metric_obj.py:169-236) ------------------------------
// Two dqo_nn1 searches by object id leave, per side, {dist2, object id} of every row in the search's SORTED order (by object, then by Morton
// code; rows without an object last, id 64): an object's rows are one contiguous run.  Block b of a side takes the sorted rows
// [1024 b, 1024 b + 1024) and stores one partial per object g it meets, at line b + g of the side's partials — the runs ascend with b, so
// no two (block, object) pairs share a line, and an object's lines are the contiguous range [first block + g, last block + g].
// THE ORDER OF EVERY SUM, fixed by the search's sorted order alone: a thread adds its rows (4 b + k) * 256 + tid, k ascending; a wave
// its lanes by the xor butterfly; a block its four waves in order; the last block (integer ticket, dqo_reduce.h) an object's lines in
// ascending block order.  No float or double atomic; the arithmetic per row and per table row is eval_pcd_kernel's.
enum {
    PCG_OBJECTS = 64,
};

__global__ __launch_bounds__(256) void eval_pcd_grouped_kernel(int n_rec, const float2* __restrict__ rk_rec, int n_gt,
                                                               const float2* __restrict__ rk_gt, int n_thres, PcThres thres, int blocks_rec,
                                                               EvWorkspace w, float* __restrict__ out) {
    __shared__ double s_stage[PC_STAGE * PC_STRIDE];
    __shared__ double s_tot[2][PCG_OBJECTS][PC_SUMS];
    __shared__ int s_first[2][PCG_OBJECTS + 1];  // where object g's run starts in a side's sorted order; [64]: where the rows without one start
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool rec_side = (int)blockIdx.x < blocks_rec;
    const int n = rec_side ? n_rec : n_gt, block = rec_side ? (int)blockIdx.x : (int)blockIdx.x - blocks_rec;
    const float2* __restrict__ rk = rec_side ? rk_rec : rk_gt;
    const int gt_base = blocks_rec + PCG_OBJECTS;  // the first line of the ground truth's partials
    if ((int64_t)block * (256 * PC_ROWS) < n) {
        double th2[PC_THRES];
#pragma unroll
        for (int t = 0; t < PC_THRES; t++) th2[t] = (double)thres.th[t] * (double)thres.th[t];
        double v[PC_ROWS];
        int obj[PC_ROWS];
#pragma unroll
        for (int k = 0; k < PC_ROWS; k++) {
            const int64_t i = ((int64_t)block * PC_ROWS + k) * 256 + tid;
            const float2 e = i < n ? rk[i] : make_float2(0.f, __int_as_float(PCG_OBJECTS));
            v[k] = (double)e.x, obj[k] = __float_as_int(e.y);
        }
        const int row0 = block * (256 * PC_ROWS), row1 = min(n, row0 + 256 * PC_ROWS) - 1;
        const int g0 = __float_as_int(rk[row0].y), g1 = min(PCG_OBJECTS - 1, __float_as_int(rk[row1].y));  // (block-uniform)
        for (int g = g0; g <= g1; g++) {
            double a[PC_SUMS];
#pragma unroll
            for (int q = 0; q < PC_SUMS; q++) a[q] = 0.0;
#pragma unroll
            for (int k = 0; k < PC_ROWS; k++)
                if (obj[k] == g) {
                    a[0] += sqrt(v[k]);
                    a[1] += 1.0;
#pragma unroll
                    for (int t = 0; t < PC_THRES; t++)
                        if (t < n_thres && v[k] < th2[t]) a[2 + t] += 1.0;
                }
#pragma unroll
            for (int q = 0; q < PC_SUMS; q++) a[q] = dqo_wave_sum_f64(a[q], lane);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < PC_SUMS; q++) s_stage[wave * PC_STRIDE + q] = a[q];
            }
            __syncthreads();
            if (tid < PC_SUMS) {
                double t = 0.0;
                for (int u = 0; u < 4; u++) t += s_stage[u * PC_STRIDE + tid];
                __hip_atomic_store(&w.partial[(size_t)((rec_side ? 0 : gt_base) + block + g) * PC_STRIDE + tid], t, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
        }
    }
    if (!dqo_last_block(w.ticket, &s_last)) return;
    if (tid < 2 * (PCG_OBJECTS + 1)) {  // the first sorted row whose object id is not below g
        const int side = tid / (PCG_OBJECTS + 1), g = tid % (PCG_OBJECTS + 1);
        const float2* __restrict__ r = side == 0 ? rk_rec : rk_gt;
        int lo = 0, hi = side == 0 ? n_rec : n_gt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (__float_as_int(r[mid].y) < g) lo = mid + 1;
            else hi = mid;
        }
        s_first[side][g] = lo;
    }
    __syncthreads();
    for (int side = 0; side < 2; side++)
        for (int g = 0; g < PCG_OBJECTS; g++) {
            const int a = s_first[side][g], b = s_first[side][g + 1];  // (block-uniform)
            double tot = 0.0;
            if (b > a) {
                const int base = (side == 0 ? 0 : gt_base) + g;
                tot = dqo_fold_partials<PC_SUMS, PC_STRIDE, PC_STAGE>(w.partial, base + a / (256 * PC_ROWS), base + (b - 1) / (256 * PC_ROWS) + 1,
                                                                      s_stage);
            }
            if (tid < PC_SUMS) s_tot[side][g][tid] = tot;
        }
    __syncthreads();
    if (tid < PCG_OBJECTS) pc_table_row(s_tot[0][tid], s_tot[1][tid], n_thres, out + (size_t)PC_SLOTS * tid);
}

struct PcgWorkspace {
    EvWorkspace ev;
    float2 *rk_rec, *rk_gt;  // {dist2, object id} in the searches' sorted order
    void* nn1;
    size_t total;
};
inline PcgWorkspace pcg_ws(void* base, int n_gt, int n_rec) {
    PcgWorkspace w;
    DqoCarver k(base);
    w.ev = ev_take(k, pc_blocks(n_rec) + pc_blocks(n_gt) + 2 * PCG_OBJECTS, PC_STRIDE);
    w.rk_rec = k.take<float2>(8 * (size_t)n_rec);
    w.rk_gt = k.take<float2>(8 * (size_t)n_gt);
    w.nn1 = k.take_raw(std::max(dqo_nn1_ws_bytes(n_rec, n_gt), dqo_nn1_ws_bytes(n_gt, n_rec)));
    w.total = k.total();
    return w;
}

// ---- Depth L1: two depth stacks compared pixel by pixel (the NICE-SLAM lineage's number; include/dqo_raster.h, dqo_eval_depth_l1) ------
// a = the truth, b = the other, float32 [n,H,W], 0 = no hit.  Per pixel of a used view: ha = a > 0 && a <= depth_trunc, hb = b > 0; the
// differences in double from the floats (exact), a side without a hit taken as 0.  Launch 1: a block takes DL_PIX * 256 pixels of ONE
// view and stores seven double sums and the float maximum as one 64-byte line (eval_picture_kernel's order: a thread its pixels in order,
// dqo_block_partial).  Launch 2: block k adds view k's lines IN BLOCK-INDEX ORDER and writes row k; the block that takes the last ticket
// reads the n rows back and writes row n.  No float or double atomic: a table is bitwise reproducible (tests/depth_l1_oracle.py).
enum {
    DL_PIX = 4,      // pixels per thread
    DL_SUMS = 7,     // |a - b| valid | (a - b)^2 valid | |a' - b'| every pixel | both | only a | only b | neither
    DL_STRIDE = 8,   // doubles per line: the sums and, in word 7, the largest |a - b| of the valid pixels (a float, widened)
    DL_STAGE = 256,
    DL_MAX_HW = 1 << 24,  // a view's counts are exact float32
};

struct DlArgs {
    int32_t HW, bpv, n_views;  // bpv: blocks (lines) per view
    const float *a, *b;
    const uint8_t* view_keep;
    float depth_trunc;
};

inline int64_t dl_bpv(int64_t HW) { return (HW + 256 * DL_PIX - 1) / (256 * DL_PIX); }
inline bool dl_size_ok(int64_t n, int64_t W, int64_t H) {
    return n >= 1 && n <= 65535 && W >= 1 && H >= 1 && W * H < DL_MAX_HW && n * dl_bpv(W * H) < (1ll << 30);
}
inline DqoLayout<EvWorkspace> dl_ws(void* base, int64_t n, int64_t HW) {
    DqoCarver k(base);
    const EvWorkspace w = ev_take(k, (size_t)(n * dl_bpv(HW)), DL_STRIDE);
    return {w, k.total()};
}

// the block's maximum of non-negative floats (compared as their bits), for every thread.  s_max: 4 words, free again after a barrier
__device__ __forceinline__ float dl_block_max(float m, uint32_t* s_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wm = dqo_wave_max_u32(__float_as_uint(m), lane);
    if (lane == 0) s_max[wave] = wm;
    __syncthreads();
    return __uint_as_float(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
}

__global__ __launch_bounds__(256) void depth_l1_partial_kernel(DlArgs g, EvWorkspace w) {
    __shared__ double s_stage[4 * DL_STRIDE];
    __shared__ uint32_t s_max[4];
    const int tid = threadIdx.x;
    const int k = (int)(blockIdx.x / (uint32_t)g.bpv), j = (int)(blockIdx.x % (uint32_t)g.bpv);
    if (g.view_keep != nullptr && g.view_keep[k] == 0) return;  // (block-uniform: an unused view has no lines)
    const float* __restrict__ a = g.a + (size_t)k * (size_t)g.HW;
    const float* __restrict__ b = g.b + (size_t)k * (size_t)g.HW;
    double s[DL_SUMS];
#pragma unroll
    for (int q = 0; q < DL_SUMS; q++) s[q] = 0.0;
    float mx = 0.0f;
#pragma unroll
    for (int p = 0; p < DL_PIX; p++) {
        const int64_t i = ((int64_t)j * DL_PIX + p) * 256 + tid;
        if (i < g.HW) {
            const float av = a[i], bv = b[i];
            const bool ha = av > 0.0f && av <= g.depth_trunc, hb = bv > 0.0f;
            const double diff = (ha ? (double)av : 0.0) - (hb ? (double)bv : 0.0), ad = fabs(diff);
            s[2] += ad;
            if (ha && hb) {
                s[0] += ad, s[1] += diff * diff, s[3] += 1.0;
                mx = fmaxf(mx, (float)ad);
            } else if (ha) s[4] += 1.0;
            else if (hb) s[5] += 1.0;
            else s[6] += 1.0;
        }
    }
    const float bm = dl_block_max(mx, s_max);
    dqo_block_partial<DL_SUMS, DL_STRIDE>(s, s_stage, w.partial);
    if (tid == DL_SUMS) __hip_atomic_store(&w.partial[(size_t)blockIdx.x * DL_STRIDE + DL_SUMS], (double)bm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid: n_views blocks.  table: float32 [n_views + 1][8]
__global__ __launch_bounds__(256) void depth_l1_rows_kernel(DlArgs g, EvWorkspace w, float* __restrict__ table) {
    __shared__ double s_stage[DL_STAGE * DL_STRIDE];
    __shared__ double s_tot[DL_STRIDE];
    __shared__ uint32_t s_max[4];
    __shared__ int s_last;
    const int tid = threadIdx.x, k = (int)blockIdx.x;
    const float nan = __int_as_float(0x7fc00000);
    float* const row = table + (size_t)8 * k;
    if (g.view_keep != nullptr && g.view_keep[k] == 0) {
        if (tid < 8) __hip_atomic_store(&row[tid], nan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const int first = k * g.bpv, last = first + g.bpv;
        const double total = dqo_fold_partials<DL_SUMS, DL_STRIDE, DL_STAGE>(w.partial, first, last, s_stage);
        float mx = 0.0f;
        for (int j = first + tid; j < last; j += 256)
            mx = fmaxf(mx, (float)__hip_atomic_load(&w.partial[(size_t)j * DL_STRIDE + DL_SUMS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        mx = dl_block_max(mx, s_max);
        if (tid < DL_SUMS) s_tot[tid] = total;
        __syncthreads();
        if (tid == 0) {
            const double both = s_tot[3];
            float r[8];
            r[0] = (float)(s_tot[0] / both);  // (both == 0: 0 / 0 = NaN)
            r[1] = both > 0.0 ? (float)(s_tot[2] / (double)g.HW) : nan;
            r[2] = (float)sqrt(s_tot[1] / both);
            r[3] = (float)both, r[4] = (float)s_tot[4], r[5] = (float)s_tot[5], r[6] = (float)s_tot[6];
            r[7] = mx;
#pragma unroll
            for (int q = 0; q < 8; q++) __hip_atomic_store(&row[q], r[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!dqo_last_block(w.ticket, &s_last)) return;
    // row n, column q by thread q over the rows in view order: 0-2 the mean of the rows where the value is defined, 3-6 the sum, 7 the maximum
    float* const stage = reinterpret_cast<float*>(s_stage);  // DL_STAGE rows of 8 floats
    double sum = 0.0, cnt = 0.0;
    float mx = 0.0f;
    for (int base = 0; base < g.n_views; base += DL_STAGE) {
        const int m = min((int)DL_STAGE, g.n_views - base);
        for (int j = tid; j < m * 8; j += 256) stage[j] = __hip_atomic_load(&table[(size_t)base * 8 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tid < 8)
            for (int v = 0; v < m; v++) {
                const float x = stage[v * 8 + tid];
                if (x == x) sum += (double)x, cnt += 1.0, mx = fmaxf(mx, x);
            }
        __syncthreads();
    }
    if (tid < 8) table[(size_t)8 * g.n_views + tid] = tid < 3 ? (float)(sum / cnt) : (tid < 7 ? (cnt > 0.0 ? (float)sum : nan) : (cnt > 0.0 ? mx : nan));
}

}  // namespace

static size_t dqo_eval_ws_bytes(int64_t HW) { return ev_ws(nullptr, HW).total; }

static int dqo_launch_eval_picture(int W, int H, const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                                   const int32_t* depth_index, float min_depth, float max_depth, const DqoRastHeader* header, float* out_row,
                                   void* ws, hipStream_t s) {
    const int64_t HW = (int64_t)W * H;
    const EvWorkspace w = ev_ws(ws, HW).w;
    DQO_LAUNCH("eval_picture_kernel", eval_picture_kernel, dim3((unsigned)ev_blocks(HW)), dim3(256), s, HW, render, gt_color, depth, gt_depth,
               depth_index, min_depth, max_depth, header, w, out_row);
    return DQO_OK;
}

static size_t dqo_eval_pcd_ws_bytes(int n_gt, int n_rec) { return pc_ws(nullptr, n_gt, n_rec).total; }

static int dqo_launch_eval_pcd(int n_gt, const float* gt_xyz, const uint8_t* gt_keep, int n_rec, const float* rec_xyz, const uint8_t* rec_keep,
                               const float* rec_xform, int n_thres, const float* thres, float* out_row, void* ws, hipStream_t s) {
    const PcWorkspace w = pc_ws(ws, n_gt, n_rec);
    const DqoNn1Rows gt_rows = {gt_keep, nullptr}, rec_rows = {rec_keep, nullptr};
    // accuracy: every reconstructed point to the ground truth (:204-208); completion: the other way round (:211-215)
    int rc = dqo_launch_nn1(n_rec, rec_xyz, rec_rows, n_gt, gt_xyz, gt_rows, rec_xform, nullptr, w.d2_rec, nullptr, nullptr, w.nn1, s);
    if (rc) return rc;
    rc = dqo_launch_nn1(n_gt, gt_xyz, gt_rows, n_rec, rec_xyz, rec_rows, nullptr, rec_xform, w.d2_gt, nullptr, nullptr, w.nn1, s);
    if (rc) return rc;
    PcThres th;
    for (int t = 0; t < PC_THRES; t++) th.th[t] = t < n_thres ? thres[t] : 0.f;
    const int blocks_rec = (int)pc_blocks(n_rec), blocks = std::max(1, blocks_rec + (int)pc_blocks(n_gt));  // (two empty sets: one block writes the NaN row)
    DQO_LAUNCH("eval_pcd_kernel", eval_pcd_kernel, dim3((unsigned)blocks), dim3(256), s, n_rec, w.d2_rec, rec_keep, n_gt, w.d2_gt, gt_keep, n_thres,
               th, blocks_rec, w.ev, out_row);
    return DQO_OK;
}

// ---- dqo_eval_pcd_surface: eval_pcd's row with a side's distances taken to the other side's SURFACE where that side has a mesh ----------
// The two dist2 columns come from dqo_mesh_nearest (knn.hip) for a side with a mesh and from dqo_nn1 for a side without; eval_pcd_kernel
// reduces them unchanged.  The searches run one after the other in one workspace part; each mesh search has its own int32 [8] header.
struct PcMesh {
    const float* vertices;
    const int32_t* faces;
    const int32_t* counts;
    int cap_v, cap_f;  // 0, 0: the side has no mesh
    bool has() const { return cap_f > 0; }
};
struct PcsWorkspace {
    EvWorkspace ev;
    float *d2_rec, *d2_gt;
    int32_t *header_gt, *header_rec;  // dqo_mesh_nearest's headers: rec points against the gt mesh, gt points against the rec mesh
    void* search;
    size_t total;
};
inline size_t pcs_search_bytes(int Q, int R, const PcMesh& m) {  // Q queries against the other side: its mesh, or its R points
    if (!m.has()) return dqo_nn1_ws_bytes(Q, R);
    return Q > 0 ? dqo_mesh_nearest_ws_bytes(Q, m.cap_v, m.cap_f) : 0;
}
inline PcsWorkspace pcs_ws(void* base, int n_gt, int n_rec, const PcMesh& gt_mesh, const PcMesh& rec_mesh) {
    PcsWorkspace w;
    DqoCarver k(base);
    w.ev = ev_take(k, pc_blocks(n_rec) + pc_blocks(n_gt) + 1, PC_STRIDE);
    w.d2_rec = k.take<float>(4 * (size_t)n_rec);
    w.d2_gt = k.take<float>(4 * (size_t)n_gt);
    w.header_gt = k.take<int32_t>(32);
    w.header_rec = k.take<int32_t>(32);
    w.search = k.take_raw(std::max(pcs_search_bytes(n_rec, n_gt, gt_mesh), pcs_search_bytes(n_gt, n_rec, rec_mesh)));
    w.total = k.total();
    return w;
}

static int dqo_launch_eval_pcd_surface(int n_gt, const float* gt_xyz, const uint8_t* gt_keep, const PcMesh& gt_mesh, int n_rec,
                                       const float* rec_xyz, const uint8_t* rec_keep, const PcMesh& rec_mesh, const float* rec_xform, int n_thres,
                                       const float* thres, float* out_row, void* ws, hipStream_t s) {
    const PcsWorkspace w = pcs_ws(ws, n_gt, n_rec, gt_mesh, rec_mesh);
    const DqoNn1Rows gt_rows = {gt_keep, nullptr}, rec_rows = {rec_keep, nullptr};
    int rc = DQO_OK;
    // accuracy: every reconstructed point (under rec_xform) to the ground truth — its surface, or its points
    if (!gt_mesh.has())
        rc = dqo_launch_nn1(n_rec, rec_xyz, rec_rows, n_gt, gt_xyz, gt_rows, rec_xform, nullptr, w.d2_rec, nullptr, nullptr, w.search, s);
    else if (n_rec > 0)
        rc = dqo_launch_mesh_nearest(n_rec, rec_xyz, rec_keep, rec_xform, gt_mesh.vertices, gt_mesh.faces, gt_mesh.counts, gt_mesh.cap_v,
                                     gt_mesh.cap_f, nullptr, w.d2_rec, nullptr, nullptr, w.header_gt, w.search, s);
    if (rc) return rc;
    // completion: every ground-truth point to the reconstruction — its surface with the vertices under rec_xform, or its points
    if (!rec_mesh.has())
        rc = dqo_launch_nn1(n_gt, gt_xyz, gt_rows, n_rec, rec_xyz, rec_rows, nullptr, rec_xform, w.d2_gt, nullptr, nullptr, w.search, s);
    else if (n_gt > 0)
        rc = dqo_launch_mesh_nearest(n_gt, gt_xyz, gt_keep, nullptr, rec_mesh.vertices, rec_mesh.faces, rec_mesh.counts, rec_mesh.cap_v,
                                     rec_mesh.cap_f, rec_xform, w.d2_gt, nullptr, nullptr, w.header_rec, w.search, s);
    if (rc) return rc;
    PcThres th;
    for (int t = 0; t < PC_THRES; t++) th.th[t] = t < n_thres ? thres[t] : 0.f;
    const int blocks_rec = (int)pc_blocks(n_rec), blocks = std::max(1, blocks_rec + (int)pc_blocks(n_gt));
    DQO_LAUNCH("eval_pcd_kernel", eval_pcd_kernel, dim3((unsigned)blocks), dim3(256), s, n_rec, w.d2_rec, rec_keep, n_gt, w.d2_gt, gt_keep, n_thres,
               th, blocks_rec, w.ev, out_row);
    return DQO_OK;
}

static int dqo_launch_eval_pcd_grouped(int n_gt, const float* gt_xyz, const int32_t* gt_group, int n_rec, const float* rec_xyz,
                                       const int32_t* rec_group, const float* rec_xform, int n_thres, const float* thres, float* out_rows, void* ws,
                                       hipStream_t s) {
    const PcgWorkspace w = pcg_ws(ws, n_gt, n_rec);
    const DqoNn1Rows gt_rows = {nullptr, gt_group}, rec_rows = {nullptr, rec_group};
    if (n_gt == 0 || n_rec == 0) n_gt = n_rec = 0;  // an empty set: no object has rows on both sides — one block writes the 64 NaN rows
    if (n_rec > 0) {
        int rc = dqo_launch_nn1(n_rec, rec_xyz, rec_rows, n_gt, gt_xyz, gt_rows, rec_xform, nullptr, nullptr, nullptr, w.rk_rec, w.nn1, s);
        if (rc) return rc;
        rc = dqo_launch_nn1(n_gt, gt_xyz, gt_rows, n_rec, rec_xyz, rec_rows, nullptr, rec_xform, nullptr, nullptr, w.rk_gt, w.nn1, s);
        if (rc) return rc;
    }
    PcThres th;
    for (int t = 0; t < PC_THRES; t++) th.th[t] = t < n_thres ? thres[t] : 0.f;
    const int blocks_rec = (int)pc_blocks(n_rec), blocks = std::max(1, blocks_rec + (int)pc_blocks(n_gt));
    DQO_LAUNCH("eval_pcd_grouped_kernel", eval_pcd_grouped_kernel, dim3((unsigned)blocks), dim3(256), s, n_rec, w.rk_rec, n_gt, w.rk_gt, n_thres, th,
               blocks_rec, w.ev, out_rows);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

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
    DQO_CHECK_WS("eval_picture", ws, ws_bytes, dqo_eval_ws_bytes((int64_t)W * H));
    return dqo_launch_eval_picture(W, H, render, gt_color, depth, gt_depth, depth_index, min_depth, max_depth, render_header,
                                   out + (size_t)8 * row, ws, (hipStream_t)stream);
}

// eval_pcd (SLAM/eval.py:190-282): accuracy, completion, chamfer distance, precision / recall / F1 per threshold
DQO_API size_t dqo_eval_pcd_workspace_bytes(int32_t n_gt, int32_t n_rec) {
    return dqo_nn1_size_ok(n_gt) && dqo_nn1_size_ok(n_rec) ? dqo_eval_pcd_ws_bytes(n_gt, n_rec) : 0;
}

DQO_API int dqo_eval_pcd(int32_t n_gt, const float* gt_xyz, const uint8_t* gt_keep, int32_t n_rec, const float* rec_xyz, const uint8_t* rec_keep,
                         const float* rec_xform, int32_t n_thres, const float* thres_host, float* out_table, int32_t row, void* ws,
                         size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(dqo_nn1_size_ok(n_gt) && dqo_nn1_size_ok(n_rec), "bad size: at most 2^25 - 1 rows per set");
    DQO_CHECK_ARG((n_gt == 0 || gt_xyz) && (n_rec == 0 || rec_xyz) && out_table, "null pointer");
    DQO_CHECK_ARG(n_thres >= 0 && n_thres <= 8 && (n_thres == 0 || thres_host), "at most 8 thresholds (got %d)", n_thres);
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    DQO_CHECK_WS("eval_pcd", ws, ws_bytes, dqo_eval_pcd_ws_bytes(n_gt, n_rec));
    return dqo_launch_eval_pcd(n_gt, gt_xyz, gt_keep, n_rec, rec_xyz, rec_keep, rec_xform, n_thres, thres_host, out_table + (size_t)32 * row, ws,
                               (hipStream_t)stream);
}

// eval_pcd's row with exact point-to-triangle distances on every side that has a mesh (a side without one: capacities 0, 0 and no buffers)
static bool pcs_mesh_ok(const PcMesh& m) {
    if (m.cap_v == 0 && m.cap_f == 0) return m.vertices == nullptr && m.faces == nullptr && m.counts == nullptr;
    return dqo_mesh_nearest_size_ok(1, m.cap_v, m.cap_f);
}

DQO_API size_t dqo_eval_pcd_surface_workspace_bytes(int32_t n_gt, int32_t gt_cap_vertices, int32_t gt_cap_faces, int32_t n_rec,
                                                    int32_t rec_cap_vertices, int32_t rec_cap_faces) {
    const PcMesh gt_mesh = {nullptr, nullptr, nullptr, gt_cap_vertices, gt_cap_faces}, rec_mesh = {nullptr, nullptr, nullptr, rec_cap_vertices, rec_cap_faces};
    if (!dqo_nn1_size_ok(n_gt) || !dqo_nn1_size_ok(n_rec) || !pcs_mesh_ok(gt_mesh) || !pcs_mesh_ok(rec_mesh)) return 0;
    return pcs_ws(nullptr, n_gt, n_rec, gt_mesh, rec_mesh).total;
}

DQO_API int dqo_eval_pcd_surface(int32_t n_gt, const float* gt_xyz, const uint8_t* gt_keep, const float* gt_vertices, const int32_t* gt_faces,
                                 const int32_t* gt_counts, int32_t gt_cap_vertices, int32_t gt_cap_faces, int32_t n_rec, const float* rec_xyz,
                                 const uint8_t* rec_keep, const float* rec_vertices, const int32_t* rec_faces, const int32_t* rec_counts,
                                 int32_t rec_cap_vertices, int32_t rec_cap_faces, const float* rec_xform, int32_t n_thres, const float* thres_host,
                                 float* out_table, int32_t row, void* ws, size_t ws_bytes, void* stream) {
    const PcMesh gt_mesh = {gt_vertices, gt_faces, gt_counts, gt_cap_vertices, gt_cap_faces};
    const PcMesh rec_mesh = {rec_vertices, rec_faces, rec_counts, rec_cap_vertices, rec_cap_faces};
    DQO_CHECK_ARG(dqo_nn1_size_ok(n_gt) && dqo_nn1_size_ok(n_rec), "bad size: at most 2^25 - 1 rows per set");
    DQO_CHECK_ARG(pcs_mesh_ok(gt_mesh) && pcs_mesh_ok(rec_mesh),
                  "bad mesh: a side without one has capacities 0, 0 and null buffers, else faces in [1, 2^25 - 1] and vertices in [1, 2^28)");
    DQO_CHECK_ARG((!gt_mesh.has() || (gt_vertices && gt_faces)) && (!rec_mesh.has() || (rec_vertices && rec_faces)), "null mesh buffer");
    DQO_CHECK_ARG((n_gt == 0 || gt_xyz) && (n_rec == 0 || rec_xyz) && out_table, "null pointer");
    DQO_CHECK_ARG(n_thres >= 0 && n_thres <= 8 && (n_thres == 0 || thres_host), "at most 8 thresholds (got %d)", n_thres);
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    DQO_CHECK_WS("eval_pcd surface", ws, ws_bytes, pcs_ws(nullptr, n_gt, n_rec, gt_mesh, rec_mesh).total);
    return dqo_launch_eval_pcd_surface(n_gt, gt_xyz, gt_keep, gt_mesh, n_rec, rec_xyz, rec_keep, rec_mesh, rec_xform, n_thres, thres_host,
                                       out_table + (size_t)32 * row, ws, (hipStream_t)stream);
}

// metric_obj.py:169-236: eval_pcd of every object's cloud against its own ground truth — one row per object id
DQO_API size_t dqo_eval_pcd_grouped_workspace_bytes(int32_t n_gt, int32_t n_rec) {
    return dqo_nn1_size_ok(n_gt) && dqo_nn1_size_ok(n_rec) ? pcg_ws(nullptr, n_gt, n_rec).total : 0;
}

DQO_API int dqo_eval_pcd_grouped(int32_t n_gt, const float* gt_xyz, const int32_t* gt_group, int32_t n_rec, const float* rec_xyz,
                                 const int32_t* rec_group, const float* rec_xform, int32_t n_thres, const float* thres_host, float* out_table,
                                 int64_t table_rows, int64_t first_row, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(dqo_nn1_size_ok(n_gt) && dqo_nn1_size_ok(n_rec), "bad size: at most 2^25 - 1 rows per set");
    DQO_CHECK_ARG((n_gt == 0 || gt_xyz) && (n_rec == 0 || rec_xyz) && out_table, "null pointer");
    DQO_CHECK_ARG((n_gt == 0 || gt_group) && (n_rec == 0 || rec_group), "null group ids");
    DQO_CHECK_ARG(n_thres >= 0 && n_thres <= 8 && (n_thres == 0 || thres_host), "at most 8 thresholds (got %d)", n_thres);
    DQO_CHECK_ARG(first_row >= 0 && first_row <= table_rows - 64, "bad rows: [%lld, %lld + 64) of a table of %lld", (long long)first_row,
                  (long long)first_row, (long long)table_rows);
    DQO_CHECK_WS("eval_pcd grouped", ws, ws_bytes, pcg_ws(nullptr, n_gt, n_rec).total);
    return dqo_launch_eval_pcd_grouped(n_gt, gt_xyz, gt_group, n_rec, rec_xyz, rec_group, rec_xform, n_thres, thres_host,
                                       out_table + (size_t)32 * first_row, ws, (hipStream_t)stream);
}

// Depth L1 of two depth stacks: a row per view and the row of the whole set
DQO_API size_t dqo_eval_depth_l1_workspace_bytes(int32_t n_views, int32_t W, int32_t H) {
    return dl_size_ok(n_views, W, H) ? dl_ws(nullptr, n_views, (int64_t)W * H).total : 0;
}

DQO_API int dqo_eval_depth_l1(int32_t n_views, int32_t W, int32_t H, const float* a, const float* b, const uint8_t* view_keep, float depth_trunc,
                              float* out_table, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(n_views >= 1 && n_views <= 65535, "bad n_views %d: 1 to 65535 views", n_views);
    DQO_CHECK_ARG(dl_size_ok(n_views, W, H), "bad image size %d x %d for %d views: both sides are at least 1, W * H is below 2^24", W, H, n_views);
    DQO_CHECK_ARG(a && b && out_table, "null pointer");
    DQO_CHECK_ARG(depth_trunc > 0.0f, "bad depth_trunc: it is above 0 (it may be +inf)");
    const int64_t HW = (int64_t)W * H;
    DQO_CHECK_WS("depth L1", ws, ws_bytes, dl_ws(nullptr, n_views, HW).total);
    DlArgs g;
    g.HW = (int32_t)HW, g.bpv = (int32_t)dl_bpv(HW), g.n_views = n_views, g.a = a, g.b = b, g.view_keep = view_keep, g.depth_trunc = depth_trunc;
    const EvWorkspace w = dl_ws(ws, n_views, HW).w;
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("depth_l1_partial_kernel", depth_l1_partial_kernel, dim3((unsigned)(n_views * g.bpv)), dim3(256), s, g, w);
    DQO_LAUNCH("depth_l1_rows_kernel", depth_l1_rows_kernel, dim3((unsigned)n_views), dim3(256), s, g, w, out_table);
    return DQO_OK;
}

}  // extern "C"
