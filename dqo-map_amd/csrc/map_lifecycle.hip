// Map maintenance for gfx950: the three statements that close every frame of the reference mapper, on ONE map with a `stable` flag per row
// instead of the reference's two clouds (SLAM/multiprocess/mapper.py:217-219, and :214 on optimise frames):
//
//     gaussians_fix()            :657-676    unstable -> stable once confidence > stable_confidence_thres (confidence clipped to it)
//     error_gaussians_remove()   :989-1102   per-Gaussian error of a render of the whole map, strike counters, delete / release (:679-689)
//     gaussians_delete()         :692-730    oversized or too-long-unstable Gaussians leave the map
//
// Everything is rewritten in place (a deleted row becomes a spare row: exactly what FusedMapper._free_rows writes), nothing is read back
// by the host, every output is an integer, a flag or a copied value.
//
// The reference scatters a per-Gaussian MAXIMUM of the pixel errors and then tests `max > 2 * thres` (:1029-1068): true exactly when some
// pixel of the Gaussian exceeds the threshold.  So the pixel pass keeps no error image and no float accumulator — a pixel over the
// threshold sets a bit of its Gaussian's vote word with an integer atomicOr (order-independent; most pixels issue nothing), and the row
// pass that consumes a vote word clears it: no zero fill per frame.
//
// The two `10 x mean radius` limits are whole-cloud reductions over the membership the earlier statements left.  No float atomics: every
// block writes a double partial sum and a count, the block that takes the last integer ticket adds the partials in index order
// (dqo_reduce.h), rounds the mean to float once and multiplies by 10 in float — bitwise the same from run to run.
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

// words of the workspace's head (int32; zero when the workspace is made, handed back at zero by every launch that uses them): the
// ticket words of dqo_reduce.h — the row kernels run one after the other and share them —, the results in free words of word 0's line,
// and the frame's counts.  Same-address atomics are served one at a time memory-side (dqo_reduce.h): with ONE word per count the last row
// kernel — whose two what-is-left counts take an atomic from every wave of the map — ran 272 us on a 550 k map
// (profiles/lifecycle_single_counter_kernel_stats.csv), so the counts are spread over DQO_COUNT_LINES lines of 256 bytes that the last block of
// the last row kernel adds up.
enum {
    LC_COUNT = 4,          // [2] rows of the stable / unstable cloud the limits below were formed over
    LC_LIMIT = 6,          // [2] float bits: 10 x mean radius of the stable / unstable cloud
    LC_ACC = DQO_REDUCE_HEAD_WORDS,  // [DQO_COUNT_LINES][64] word k of a line: count k of the frame while the row kernels run (DqoLifecycle.stats gets the sums)
    LC_HEAD_WORDS = LC_ACC + DQO_COUNT_LINES * 64,
    LC_SUMS = 2,           // doubles per block partial: radius sum | member rows
    LC_STAGE = 128,        // partials staged through LDS at a time by the last block
};
static_assert(LC_LIMIT + 2 <= 16 && LC_HEAD_WORDS * 4 % 256 == 0, "workspace head layout");

struct LcWorkspace {
    int32_t* head;
    double* partial;  // [blocks][LC_SUMS]
};

__host__ __device__ inline size_t lc_blocks(int64_t P) { return (size_t)((P + 255) / 256); }

inline LcWorkspace lc_workspace(void* base) {
    LcWorkspace w;
    w.head = (int32_t*)base;
    w.partial = (double*)((char*)base + LC_HEAD_WORDS * 4);
    return w;
}

// GaussianPointCloud.get_radius (gaussian_pointcloud.py:739-743): the mean of the two larger scales
__device__ __forceinline__ float lc_radius(const float* __restrict__ scaling_raw, size_t i) {
    const float a = expf(scaling_raw[3 * i]), b = expf(scaling_raw[3 * i + 1]), c = expf(scaling_raw[3 * i + 2]);
    return (((a + b) + c) - fminf(fminf(a, b), c)) / 2.f;
}

// 10 x the mean radius of the rows with `member` set, over the whole launch: head[LC_LIMIT + which] (float bits) and the row count in
// head[LC_COUNT + which], written by the last block.  Every thread of every block calls it.
__device__ __forceinline__ void lc_cloud_limit(const LcWorkspace& w, int which, float radius, bool member) {
    __shared__ double s_stage[LC_STAGE * LC_SUMS];
    __shared__ int s_last;
    double a[LC_SUMS] = {member ? (double)radius : 0.0, member ? 1.0 : 0.0};  // (the count is exact in a double)
    dqo_block_partial<LC_SUMS, LC_SUMS>(a, s_stage, w.partial);
    if (!dqo_last_block(w.head, &s_last)) return;
    const double total = dqo_fold_partials<LC_SUMS, LC_SUMS, LC_STAGE>(w.partial, 0, (int)gridDim.x, s_stage);
    if (threadIdx.x < LC_SUMS) s_stage[threadIdx.x] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = s_stage[0], rows = s_stage[1];
        const float mean = rows > 0.0 ? (float)(sum / rows) : 0.f;  // rounded to float once
        w.head[LC_LIMIT + which] = __float_as_int(mean * 10.f);
        w.head[LC_COUNT + which] = (int32_t)rows;
    }
}

// ---- the pixel pass (mapper.py:1015-1026, 1064-1068) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lifecycle_vote_kernel(int64_t HW, int P, const float* __restrict__ gt_color,
                                                             const float* __restrict__ gt_depth, const float* __restrict__ render,
                                                             const float* __restrict__ depth, const int32_t* __restrict__ depth_index,
                                                             const int32_t* __restrict__ color_index, float color_thr, float depth_thr,
                                                             uint32_t* __restrict__ vote, const DqoRastHeader* __restrict__ header) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    if (header != nullptr && header->overflow != 0u) return;  // the render outgrew its context: its images are invalid
    const float gd = gt_depth[i];
    if (gd == 0.f) return;  // both errors are zero there (:1021, 1025)
    const int di = depth_index[i], ci = color_index[i];
    const float diff = gd - depth[i];
    const float de = (diff < 0.f || di == -1) ? 0.f : fabsf(diff);  // (:1015-1016, 1021-1024)
    // (a Gaussian covers many pixels: the plain read spares most of them the atomic; a stale 0 only costs a redundant one)
    if (de > depth_thr && di >= 0 && di < P && !(vote[di] & 1u)) atomicOr(&vote[di], 1u);
    const float ce = (fabsf(gt_color[i] - render[i]) + fabsf(gt_color[HW + i] - render[HW + i])) + fabsf(gt_color[2 * HW + i] - render[2 * HW + i]);
    if (ce > color_thr && ci >= 0 && ci < P && !(vote[ci] & 2u)) atomicOr(&vote[ci], 2u);
}

// ---- the row kernels --------------------------------------------------------------------------------------------------------------------
// (optional) the limit of the STABLE cloud as the frame finds it: gaussians_delete(unstable=False), mapper.py:214
__global__ __launch_bounds__(256) void lifecycle_stable_limit_kernel(DqoLifecycle a, LcWorkspace w) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool member = i < (size_t)a.P && a.alive[i] != 0 && a.stable[i] != 0;
    lc_cloud_limit(w, 0, member ? lc_radius(a.scaling_raw, i) : 0.f, member);
}

// statements 0 (optional), 1 and 2, and the limit of the unstable cloud they leave
__global__ __launch_bounds__(256) void lifecycle_fix_kernel(DqoLifecycle a, LcWorkspace w) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < (size_t)a.P;
    bool alive = in && a.alive[i] != 0;
    bool stable = alive && a.stable[i] != 0;
    const float radius = alive ? lc_radius(a.scaling_raw, i) : 0.f;
    // 0. gaussians_delete(unstable=False): oversized rows of the stable cloud (a cloud with a member has a limit)
    const bool big_stable = a.stable_oversized != 0 && stable && radius > __int_as_float(w.head[LC_LIMIT + 0]);
    if (big_stable) dqo_map_free_row(a, i), alive = stable = false;
    // 1. gaussians_fix
    const bool promoted = alive && !stable && a.confidence[i] > a.stable_confidence_thres;
    if (promoted) {
        a.stable[i] = 1, stable = true;
        a.confidence[i] = a.stable_confidence_thres;  // torch.clip(confidence, max=thres) of a value above it
    }
    // 2. error_gaussians_remove: strikes count on rows that are stable now; delete wins over release; a released row keeps its counters
    bool by_depth = false, released = false;
    if (a.use_votes != 0 && in) {
        const uint32_t v = a.vote[i];
        if (v != 0u) a.vote[i] = 0u;
        if (stable) {
            const int dc = a.depth_error_counter[i] + (int)(v & 1u), cc = a.color_error_counter[i] + (int)((v >> 1) & 1u);
            by_depth = dc >= a.delete_thresh;
            released = !by_depth && cc >= a.delete_thresh;
            if (by_depth) {
                dqo_map_free_row(a, i), alive = stable = false;
            } else {
                if (v & 1u) a.depth_error_counter[i] = dc;
                if (v & 2u) a.color_error_counter[i] = cc;
                if (released) {  // gaussians_release, :679-689
                    a.stable[i] = 0, stable = false;
                    a.confidence[i] = 0.f;
                    a.add_tick[i] = a.tick;
                }
            }
        }
    }
    dqo_line_count(w.head + LC_ACC, 0, promoted, lane);
    dqo_line_count(w.head + LC_ACC, 1, released, lane);
    dqo_line_count(w.head + LC_ACC, 2, by_depth, lane);
    dqo_line_count(w.head + LC_ACC, 5, big_stable, lane);
    lc_cloud_limit(w, 1, radius, alive && !stable);
}

// statement 3: gaussians_delete(unstable=True), the counts of what is left, and the frame's counts handed over
__global__ __launch_bounds__(256) void lifecycle_delete_kernel(DqoLifecycle a, LcWorkspace w) {
    __shared__ int s_last;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool alive = i < (size_t)a.P && a.alive[i] != 0;
    const bool stable = alive && a.stable[i] != 0, unstable = alive && !stable;
    const bool big = unstable && lc_radius(a.scaling_raw, i) > __int_as_float(w.head[LC_LIMIT + 1]);
    const bool old = unstable && !big && a.tick - a.add_tick[i] > a.unstable_time_window;  // (a row that is both counts as oversized)
    if (big || old) dqo_map_free_row(a, i);
    dqo_line_count(w.head + LC_ACC, 3, big, lane);
    dqo_line_count(w.head + LC_ACC, 4, old, lane);
    dqo_line_count(w.head + LC_ACC, 6, unstable && !big && !old, lane);
    dqo_line_count(w.head + LC_ACC, 7, stable, lane);
    if (!dqo_last_block(w.head, &s_last)) return;
    dqo_line_totals(w.head + LC_ACC, 0xffu, a.stats);  // the eight counts
}

}  // namespace

static size_t dqo_lifecycle_ws_bytes(int64_t P) { return LC_HEAD_WORDS * 4 + dqo_align_up(lc_blocks(P) * LC_SUMS * sizeof(double), 256); }

static int dqo_launch_lifecycle_vote(const DqoLifecycle* a, const float* gt_color, const float* gt_depth, const float* render, const float* depth,
                                     const int32_t* depth_index, const int32_t* color_index, hipStream_t s) {
    const int64_t HW = (int64_t)a->W * a->H;
    DQO_LAUNCH("lifecycle_vote_kernel", lifecycle_vote_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), s, HW, a->P, gt_color, gt_depth,
               render, depth, depth_index, color_index, 2.f * a->add_color_thres, 2.f * a->add_depth_thres, a->vote, a->render_header);
    return DQO_OK;
}

static int dqo_launch_lifecycle_rows(const DqoLifecycle* a, hipStream_t s) {
    const LcWorkspace w = lc_workspace(a->workspace);
    const dim3 grid((unsigned)lc_blocks(a->P)), block(256);
    if (a->stable_oversized) {
        DQO_LAUNCH("lifecycle_stable_limit_kernel", lifecycle_stable_limit_kernel, grid, block, s, *a, w);
    }
    DQO_LAUNCH("lifecycle_fix_kernel", lifecycle_fix_kernel, grid, block, s, *a, w);
    DQO_LAUNCH("lifecycle_delete_kernel", lifecycle_delete_kernel, grid, block, s, *a, w);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_map_lifecycle_workspace_bytes(int32_t P) { return dqo_lifecycle_ws_bytes(P < 0 ? 0 : P); }

static int check_lifecycle(const DqoLifecycle* a) {
    DQO_CHECK_ARG(a != nullptr, "null DqoLifecycle");
    DQO_CHECK_ARG(a->P >= 0 && a->delete_thresh >= 1, "bad P / delete_thresh");
    if (a->P == 0) return DQO_OK;
    DQO_CHECK_ARG(a->xyz && a->opacity_raw && a->scaling_raw && a->confidence && a->alive && a->row_flags && a->stable && a->add_tick &&
                      a->depth_error_counter && a->color_error_counter && a->park && a->vote, "null per-Gaussian buffer / park / vote");
    DQO_CHECK_WS("lifecycle", a->workspace, a->workspace_bytes, dqo_lifecycle_ws_bytes(a->P));
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

}  // extern "C"
