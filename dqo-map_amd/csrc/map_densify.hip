// Geometry evaluation for gfx950, the reconstruction's point set: GaussianPointCloud.densify (SLAM/gaussian_pointcloud.py:67-130; called as
// densify(1, 30, 5) from slam.py:202-206 for the configs with pcd_densify) followed by the subsample of eval_pcd (SLAM/eval.py:244) — in
// one device step that never holds the densified cloud.  include/dqo_raster.h (dqo_surfel_densify) states the contract.
//
// Row i becomes M = circle_num * levels * sigma virtual points v = i * M + c on ellipses in its plane.  The reference keeps
// min(N, sample_nums) of the N points of the kept rows by np.random.choice; here a virtual point gets the 32-bit key of dqo_sample_hash.h
// (draw 3) and the n = min(N, cap) smallest keys are chosen: the same distribution, a pure function of the arguments.  fmix32 is a
// bijection and v < 2^32, so two keys never tie: "key <= t" with t the n-th smallest key names exactly n points, and no rank pass is needed.
// t is found by a radix select over three digits (11 + 11 + 10 bits), never by a sort (dqo_select.h: the digit, the flush, the last
// block's pick and its single-word ticket, shared with map_sample.hip; the scans over a block's threads and over the chunks: dqo_reduce.h):
//
//     zero            the workspace's head (histograms, tickets, state): the workspace needs no initialisation
//     histogram x 3   keys of the kept rows' virtual points, one digit per launch, inside the bucket picked so far; a block's histogram is
//                     built in LDS over all its chunks and only its non-zero bins go to memory; the last block picks the next bucket
//                     (the first one also forms N and n).  Needs row_keep[v / M] and the hash, no parameters.
//     count pass      chosen points per chunk of 2048 virtual points; the last block scans the chunks in index order, writes the header
//     emit pass       ordered compaction (a thread owns 8 consecutive virtual points; exclusive prefix over the block's threads) of a
//                     chunk's chosen v into a list in LDS, then a run of consecutive list entries per thread: the chosen points in
//                     ascending v; and keep[] for all cap rows
//
// cap >= P * M (known on the host): no key can be rejected, t = 0xffffffff and the three histogram launches are skipped.  Above 2048
// blocks a launch is grid-strided: block b serves chunks b, b + 2048, ...
// Integer atomics only (histograms, tickets): their order cannot reach the output.  Nothing is allocated, read back or synchronised.
//
// This file is compiled with -ffp-contract=off.  The float statements of one point, one rounding each, in this order:
//     s_j   = expf(scaling_raw[j]); the three axes in ascending order of the RAW scales (exp is monotone), equal ones lower index first
//     q     = rotation_raw / sqrtf(((r r + x x) + y y) + z z)                               (one normalisation; the reference's second
//                                                                                            one divides by a norm that is 1 up to rounding)
//     R     = build_rotation(q) (utils/general_utils.py:122-130), n / p0 / p1 = its columns order[0] / order[1] / order[2],
//             each divided by (sqrtf((a a + b b) + c c) + 1e-8f)                             (:791, :808-809)
//     f_l   = float(double(l + 0.5) / double(levels));  a = (s[order[1]] * float(sigma)) * f_l, in blocks b >= 1 a = a + s[order[1]] * float(b)
//             (:84-102); b_ the same with s[order[2]]
//     x     = a * cos[k];  z = b_ * sin[k]                                                   (:104-105, the caller's float32 table)
//     frame 0 (the reference's, :107-121 — the three vectors are the ROWS of its matrix):
//             out = mean + (p0.x x + p0.z z,  n.x x + n.z z,  p1.x x + p1.z z)
//     frame 1 (the surfel's plane): out_c = mean_c + (p0_c x + p1_c z)
// with c = (b * levels + l) * circle_num + k.  A thread keeps the frame of the row it last formed: the consecutive chosen columns of a
// row it emits share it.
#include "dqo_common.h"
#include "dqo_reduce.h"
#include "dqo_sample_hash.h"
#include "dqo_select.h"

namespace {

enum {
    DN_THREADS = 256,
    DN_VPT = 8,                      // virtual points per thread: v = chunk * DN_CHUNK + thread * 8 + j
    DN_CHUNK = DN_THREADS * DN_VPT,
    DN_MAX_BLOCKS = 2048,
    // words of the workspace's head (zeroed by the first launch of every call)
    DN_HIST = 0,                     // [3 levels][DQO_SELECT_BINS]
    DN_TICKET = 3 * DQO_SELECT_BINS,  // [4] one per kernel that ends in a last block
    DN_STATE = DN_TICKET + 8,        // 0 key prefix / threshold t, 1 rank left in the bucket, 2 N, 4 n, 5 nothing is rejected (n == N)
    DN_HEAD_WORDS = DN_STATE + 56,
};
static_assert(DN_HEAD_WORDS * 4 % 256 == 0, "workspace head layout");

struct DnArgs {
    uint64_t total;  // P * M < 2^32
    uint64_t cap;
    uint32_t M, circle_num, ring, levels, sigma;  // ring = circle_num * levels
    uint32_t nchunks;
    uint32_t seed_word, draw_word;
    int frame, skip_select;
    const float *xyz, *scaling_raw, *rotation_raw, *circle_cs;
    const uint8_t* row_keep;
    float *points, *normals;
    int64_t* index;
    uint8_t* keep;
    int32_t* header;
    uint32_t* head;
    uint32_t* chunk_count;  // [nchunks] chosen points of a chunk, then their exclusive prefix
};

// f(j, key) for each of this thread's eight virtual points of `chunk` that lie in a kept row: v = chunk * DN_CHUNK + thread * 8 + j
template <class F>
__device__ __forceinline__ void dn_kept_points(const DnArgs& a, uint32_t chunk, F f) {
    const uint64_t v0 = (uint64_t)chunk * DN_CHUNK + (uint64_t)threadIdx.x * DN_VPT;
    if (v0 >= a.total) return;
    uint32_t row = (uint32_t)v0 / a.M, c = (uint32_t)v0 % a.M;  // (v0 < P * M < 2^32)
    bool kept = a.row_keep == nullptr || a.row_keep[row] != 0;
#pragma unroll
    for (int j = 0; j < DN_VPT; j++) {
        if (v0 + j >= a.total) break;
        if (kept) f(j, dqo_sample_key(a.seed_word, a.draw_word, (uint32_t)(v0 + j), 0xffffffffu));
        if (++c == a.M) {
            c = 0u, row++;
            kept = a.row_keep == nullptr || ((uint64_t)row * a.M < a.total && a.row_keep[row] != 0);
        }
    }
}

// The chosen virtual points among this thread's eight of `chunk` as a bit mask: kept row, key <= t
__device__ __forceinline__ uint32_t dn_chosen(const DnArgs& a, uint32_t chunk, uint32_t t) {
    uint32_t mask = 0u;
    dn_kept_points(a, chunk, [&](int j, uint32_t key) {
        if (key <= t) mask |= 1u << j;
    });
    return mask;
}

// ---- the histogram passes: one digit of the keys of the kept rows' virtual points, inside the bucket picked so far ----------------------
template <int LEVEL>
__global__ __launch_bounds__(DN_THREADS) void densify_hist_kernel(DnArgs a) {
    __shared__ uint32_t s_hist[DQO_SELECT_BINS];
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x;
    uint32_t* const hist = a.head + DN_HIST + LEVEL * DQO_SELECT_BINS;
    if (LEVEL > 0 && a.head[DN_STATE + 5] != 0u) return;  // (every block: nothing is rejected, the first pass left t = 0xffffffff)
    const uint32_t prefix = LEVEL > 0 ? a.head[DN_STATE + 0] : 0u;
    for (int i = tid; i < DQO_SELECT_BINS; i += DN_THREADS) s_hist[i] = 0u;
    __syncthreads();
    for (uint32_t chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x)
        dn_kept_points(a, chunk, [&](int, uint32_t key) {
            if (dqo_select_in_bucket(key, prefix, LEVEL)) dqo_select_count(s_hist, key, LEVEL);
        });
    __syncthreads();
    dqo_select_flush(s_hist, hist);
    if (!dqo_single_ticket_last_block(&a.head[DN_TICKET + LEVEL])) return;
    uint32_t* const state = a.head + DN_STATE;
    if (LEVEL == 0) {
        // N = the keys counted (P * M < 2^32: a word holds it), n = min(N, cap)
        uint32_t sum = 0u, N;
#pragma unroll
        for (int j = 0; j < 8; j++) sum += dqo_ld_u32(&hist[tid * 8 + j]);
        dqo_block_exclusive(sum, N, s_wave);
        if (tid == 0) {
            const uint32_t n = (uint64_t)N <= a.cap ? N : (uint32_t)a.cap;
            dqo_st_u32(&state[1], n), dqo_st_u32(&state[2], N);
            dqo_st_u32(&state[5], n == N ? 1u : 0u);
            if (n == N) dqo_st_u32(&state[0], 0xffffffffu);
            __threadfence();
        }
        __syncthreads();
        if (dqo_ld_u32(&state[5]) != 0u) return;
    }
    dqo_select_pick(hist, state, LEVEL);
}

// ---- the count pass: chosen points per chunk, and how many come before each chunk ----------------------------------------------------------
__global__ __launch_bounds__(DN_THREADS) void densify_count_kernel(DnArgs a) {
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x;
    const uint32_t t = a.skip_select ? 0xffffffffu : a.head[DN_STATE + 0];
    for (uint32_t chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
        uint32_t total;
        dqo_block_exclusive((uint32_t)__popc(dn_chosen(a, chunk, t)), total, s_wave);
        if (tid == 0) dqo_st_u32(&a.chunk_count[chunk], total);
    }
    if (!dqo_single_ticket_last_block(&a.head[DN_TICKET + 3])) return;
    // exclusive prefix of the chunks' counts in index order, in place: a thread takes eight consecutive chunks of a round
    const uint32_t n = dqo_scan_block_counts<uint32_t, 8>(a.chunk_count, a.nchunks, 1, s_wave);
    if (tid == 0) {
        uint32_t* const state = a.head + DN_STATE;
        const uint32_t N = a.skip_select ? n : dqo_ld_u32(&state[2]);
        if (a.skip_select) dqo_st_u32(&state[0], t);
        dqo_st_u32(&state[4], n);
        a.header[0] = (int32_t)(N / a.M), a.header[1] = (int32_t)N, a.header[2] = 0;  // (N < 2^32: the high word)
        a.header[3] = (int32_t)n, a.header[4] = (int32_t)a.M, a.header[5] = (int32_t)t, a.header[6] = a.frame, a.header[7] = 0;
    }
}

// what one row gives all its points
struct DnFrame {
    float mean[3], n[3], p0[3], p1[3], axis0, axis1;
};

__device__ __forceinline__ void dn_column(float r, float x, float y, float z, int k, float out[3]) {
    float a, b, c;
    if (k == 0) a = 1.f - 2.f * (y * y + z * z), b = 2.f * (x * y + r * z), c = 2.f * (x * z - r * y);
    else if (k == 1) a = 2.f * (x * y - r * z), b = 1.f - 2.f * (x * x + z * z), c = 2.f * (y * z + r * x);
    else a = 2.f * (x * z + r * y), b = 2.f * (y * z - r * x), c = 1.f - 2.f * (x * x + y * y);
    const float nn = sqrtf((a * a + b * b) + c * c) + 1e-8f;
    out[0] = a / nn, out[1] = b / nn, out[2] = c / nn;
}

__device__ __forceinline__ void dn_frame(const DnArgs& a, uint32_t row, DnFrame& f) {
    const size_t i = row;
    const float raw[3] = {a.scaling_raw[3 * i], a.scaling_raw[3 * i + 1], a.scaling_raw[3 * i + 2]};
    // ascending, the first of equal ones first: argmin (get_normal, :783), then the other two in index order unless the later is smaller
    const int o0 = (raw[0] <= raw[1] && raw[0] <= raw[2]) ? 0 : (raw[1] <= raw[2] ? 1 : 2);
    int o1 = o0 == 0 ? 1 : 0, o2 = o0 == 2 ? 1 : 2;
    if (raw[o2] < raw[o1]) {
        const int s = o1;
        o1 = o2, o2 = s;
    }
    float r = a.rotation_raw[4 * i], x = a.rotation_raw[4 * i + 1], y = a.rotation_raw[4 * i + 2], z = a.rotation_raw[4 * i + 3];
    const float nq = sqrtf(((r * r + x * x) + y * y) + z * z);
    r = r / nq, x = x / nq, y = y / nq, z = z / nq;
    dn_column(r, x, y, z, o0, f.n), dn_column(r, x, y, z, o1, f.p0), dn_column(r, x, y, z, o2, f.p1);
    f.axis0 = expf(raw[o1]), f.axis1 = expf(raw[o2]);
    f.mean[0] = a.xyz[3 * i], f.mean[1] = a.xyz[3 * i + 1], f.mean[2] = a.xyz[3 * i + 2];
}

// ---- the emit pass (gaussian_pointcloud.py:84-123) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(DN_THREADS) void densify_emit_kernel(DnArgs a) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_list[DN_CHUNK];
    const int tid = threadIdx.x;
    const uint32_t t = a.head[DN_STATE + 0], n = a.head[DN_STATE + 4];
    for (uint64_t q = (uint64_t)blockIdx.x * DN_THREADS + tid; q < a.cap; q += (uint64_t)gridDim.x * DN_THREADS) a.keep[q] = q < n ? 1 : 0;
    const float sig = (float)a.sigma;
    DnFrame f;
    uint32_t f_row = 0xffffffffu;
    for (uint32_t chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
        // the chunk's chosen virtual points, in ascending v, as a list in LDS: with a million of 75 million chosen a wave holds one or
        // two, and forming them where they are found runs the whole statement sequence below once per such lane and slot
        const uint32_t mask = dn_chosen(a, chunk, t);
        uint32_t total;
        uint32_t pos = dqo_block_exclusive((uint32_t)__popc(mask), total, s_wave);
        const uint32_t v0 = chunk * (uint32_t)DN_CHUNK + (uint32_t)tid * DN_VPT;  // (mask != 0: v0 < P * M < 2^32)
#pragma unroll
        for (int j = 0; j < DN_VPT; j++)
            if (mask & (1u << j)) s_list[pos++] = v0 + j;
        __syncthreads();
        // a thread takes a run of consecutive entries (one entry when few are chosen): they mostly share a row, and its frame
        const uint32_t per = (total + DN_THREADS - 1) / DN_THREADS;
        const uint32_t e0 = min((uint32_t)tid * per, total), e1 = min(e0 + per, total);
        for (uint32_t e = e0; e < e1; e++) {
            const uint64_t q = (uint64_t)a.chunk_count[chunk] + e;
            if (q >= a.cap || q >= n) break;  // (cannot happen: exactly n keys are <= t; rows at and behind n are never written)
            const uint32_t v = s_list[e];
            const uint32_t row = v / a.M, c = v % a.M;
            if (row != f_row) dn_frame(a, row, f), f_row = row;
            const uint32_t b = c / a.ring, rem = c % a.ring, l = rem / a.circle_num, k = rem % a.circle_num;
            const float fl = (float)(((double)l + 0.5) / (double)a.levels);  // :88-93, a Python double rounded into the float product
            float ra = (f.axis0 * sig) * fl, rb = (f.axis1 * sig) * fl;      // :84-85
            if (b >= 1u) ra = ra + f.axis0 * (float)b, rb = rb + f.axis1 * (float)b;  // :101-102
            const float x = ra * a.circle_cs[k], z = rb * a.circle_cs[a.circle_num + k];  // :104-105
            float o[3];
            if (a.frame == 0) {  // :107-121: stack(...).permute(0, 2, 1) has p0, n, p1 as rows
                o[0] = f.mean[0] + (f.p0[0] * x + f.p0[2] * z);
                o[1] = f.mean[1] + (f.n[0] * x + f.n[2] * z);
                o[2] = f.mean[2] + (f.p1[0] * x + f.p1[2] * z);
            } else {
#pragma unroll
                for (int d = 0; d < 3; d++) o[d] = f.mean[d] + (f.p0[d] * x + f.p1[d] * z);
            }
#pragma unroll
            for (int d = 0; d < 3; d++) a.points[3 * q + d] = o[d];
            if (a.normals != nullptr) {
#pragma unroll
                for (int d = 0; d < 3; d++) a.normals[3 * q + d] = f.n[d];  // :122
            }
            if (a.index != nullptr) a.index[q] = (int64_t)v;
        }
        __syncthreads();  // (the next chunk's list overwrites this one)
    }
}

inline uint32_t dn_chunks(uint64_t total) { return (uint32_t)((total + DN_CHUNK - 1) / DN_CHUNK); }

}  // namespace

static size_t dqo_densify_ws_bytes(uint64_t total) { return DN_HEAD_WORDS * 4 + dqo_align_up((size_t)dn_chunks(total) * sizeof(uint32_t), 256); }

static int dqo_launch_surfel_densify(int P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const uint8_t* row_keep,
                                     int circle_num, int levels, int sigma, const float* circle_cs, int frame, uint64_t seed, int64_t cap,
                                     float* points, float* normals, int64_t* index, uint8_t* keep, int32_t* header, void* ws, hipStream_t s) {
    DnArgs a;
    a.M = (uint32_t)circle_num * (uint32_t)levels * (uint32_t)sigma;
    a.total = (uint64_t)P * a.M, a.cap = (uint64_t)cap;
    a.circle_num = (uint32_t)circle_num, a.levels = (uint32_t)levels, a.sigma = (uint32_t)sigma, a.ring = (uint32_t)circle_num * (uint32_t)levels;
    a.nchunks = dn_chunks(a.total);
    a.seed_word = dqo_sample_seed_word(seed), a.draw_word = dqo_sample_draw_word(a.seed_word, 3u);
    a.frame = frame, a.skip_select = a.total <= a.cap ? 1 : 0;
    a.xyz = xyz, a.scaling_raw = scaling_raw, a.rotation_raw = rotation_raw, a.circle_cs = circle_cs, a.row_keep = row_keep;
    a.points = points, a.normals = normals, a.index = index, a.keep = keep, a.header = header;
    a.head = (uint32_t*)ws, a.chunk_count = (uint32_t*)((char*)ws + DN_HEAD_WORDS * 4);
    const dim3 grid(a.nchunks < DN_MAX_BLOCKS ? a.nchunks : (unsigned)DN_MAX_BLOCKS), block(DN_THREADS);
    const int rc = dqo_launch_zero_words(a.head, DN_HEAD_WORDS, s);
    if (rc) return rc;
    if (!a.skip_select) {
        DQO_LAUNCH("densify_hist_kernel<0>", densify_hist_kernel<0>, grid, block, s, a);
        DQO_LAUNCH("densify_hist_kernel<1>", densify_hist_kernel<1>, grid, block, s, a);
        DQO_LAUNCH("densify_hist_kernel<2>", densify_hist_kernel<2>, grid, block, s, a);
    }
    DQO_LAUNCH("densify_count_kernel", densify_count_kernel, grid, block, s, a);
    DQO_LAUNCH("densify_emit_kernel", densify_emit_kernel, grid, block, s, a);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

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
    DQO_CHECK_WS("surfel densify", ws, ws_bytes, dqo_densify_ws_bytes((uint64_t)P * (uint64_t)M));
    return dqo_launch_surfel_densify(P, xyz, scaling_raw, rotation_raw, row_keep, circle_num, levels, sigma, circle_cs, frame, seed, cap, points,
                                     normals, index, keep, header, ws, (hipStream_t)stream);
}

}  // extern "C"
