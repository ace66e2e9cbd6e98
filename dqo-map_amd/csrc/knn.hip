// Exact 3-nearest-neighbour search (mean squared distance + neighbour indices) for gfx950.
//
// Replaces /root/reference/submodules/simple-knn/simple_knn.cu:45-252 (SimpleKNN::knn) and spatial.cu:15-28 (distCUDA2):
// same result = for every point the three smallest squared distances to OTHER positions, ties resolved by the order of
// a stable sort on the 30-bit Morton code (the order in which the reference's scan meets the candidates).
//
// MI355X design: no cudaMalloc / thrust allocations / D2H copies inside the call (the reference does 2 blocking 12-byte
// reads for the bounding box and allocates five temporaries per call): one caller-owned workspace, everything on the
// caller's stream.  Points are gathered ONCE into Morton order as float4 (xyz + original index), so the candidate scan
// reads contiguous, wave-uniform addresses (broadcast loads) instead of chasing an index indirection per candidate.
// The sort is a stable LSD radix sort of the 30-bit codes (index as payload: equal codes keep index order = the reference's stable
// sort), four 8-bit passes of histogram -> scan -> scatter; the rank of a key among the equal digits of its block comes from wave
// ballots (eight ballots match the lanes with the same digit) + per-wave counts in LDS.  12 launches for any size; the first
// version — a 64-bit bitonic network, 4096-key runs in LDS, merge steps >= 4096 in global memory — needed 55 launches and 0.73 ms
// for 2 M keys.
#include <float.h>
#include <limits.h>

#include <algorithm>

#include "dqo_common.h"
#include "dqo_mesh_operand.h"

namespace {

constexpr int KNN_BOX = 1024;  // simple_knn.cu:16 BOX_SIZE (part of the pruning structure only)
constexpr int KNN_SUB = 64;    // second pruning level of the query search: one wave-load of sorted points
constexpr int SORT_RUN = 4096;
constexpr int RDX_T = 256, RDX_KPT = 8, RDX_BLK = RDX_T * RDX_KPT;  // radix sort: keys per block

struct KnnWs {
    float* bbox;        // [8] min xyz, max xyz
    uint64_t* keys;     // [P2] (morton << 32 | original index), padded to a power of two with ~0
    float4* sorted;     // [P] (x, y, z, bits(original index)) in Morton order
    float* boxes;       // [nb][8] min xyz, max xyz of each run of 1024 sorted points
    float* sub;         // [ceil(P / 64)][8] ... of each run of 64 sorted points (query search only)
    uint32_t* hist;     // [256][ceil(P / RDX_BLK)] digit histograms / scatter offsets of one radix pass
    float* groups;      // [ceil(nb / 64)][8] min / max of each run of 64 level-1 boxes = 65 536 sorted points (query search only)
    size_t total;
};

inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

inline KnnWs knn_ws(void* base, int P) {
    KnnWs w;
    DqoCarver k(base);
    const int P2 = next_pow2(P < SORT_RUN ? SORT_RUN : P);
    w.bbox = k.take<float>(32);
    w.keys = k.take<uint64_t>(8 * (size_t)P2);
    w.sorted = k.take<float4>(16 * (size_t)P);
    w.boxes = k.take<float>(32 * (size_t)((P + KNN_BOX - 1) / KNN_BOX));
    w.sub = k.take<float>(32 * (size_t)((P + KNN_SUB - 1) / KNN_SUB));
    w.hist = k.take<uint32_t>(4 * 256 * ((size_t)((P + RDX_BLK - 1) / RDX_BLK) + 1));  // + the 256 row totals behind the table
    w.groups = k.take<float>(32 * (size_t)(((P + KNN_BOX - 1) / KNN_BOX + 63) / 64));
    w.total = k.total();
    return w;
}

// min / max over all points with init {0,0,0}: the bounding box always contains the origin (simple_knn.cu:222-231, B15).
// Two stages: every block reduces a strided slice of the points into a partial box, one block folds the partial boxes (a single
// block over all points took 0.68 ms on a 2 M-point map — a quarter of a map-growth query).
constexpr int BBOX_BLOCKS_MAX = 512;
__device__ __forceinline__ void bbox_block_reduce(float mn[3], float mx[3], float* __restrict__ out) {
    __shared__ float s[6][16];
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int a = 0; a < 3; a++) s[a][wave] = mn[a], s[3 + a][wave] = mx[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = s[threadIdx.x][0];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = threadIdx.x < 3 ? fminf(r, s[threadIdx.x][w]) : fmaxf(r, s[threadIdx.x][w]);
        out[threadIdx.x] = r;
    }
}
// group (dqo_knn3_query_grouped): points without a group (id outside [0, 64): spare rows parked far away, deleted Gaussians) take no part
// in the search — they do not stretch the bounding box the Morton grid is laid over, sort behind every real point and are gathered as
// a far sentinel, so the boxes they fill are pruned by distance
__device__ __forceinline__ bool knn_in_group(const int32_t* __restrict__ group, int i) {
    if (group == nullptr) return true;
    const int gid = group[i];
    return gid >= 0 && gid < 64;
}
__global__ __launch_bounds__(1024) void bbox_kernel(int P, const float* __restrict__ xyz, float* __restrict__ partial,
                                                    const int32_t* __restrict__ group) {
    float mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
        if (!knn_in_group(group, i)) continue;
        for (int a = 0; a < 3; a++) {
            const float v = xyz[3 * i + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
    bbox_block_reduce(mn, mx, partial + 8 * blockIdx.x);
}
__global__ __launch_bounds__(512) void bbox_fold_kernel(int n, const float* __restrict__ partial, float* __restrict__ bbox) {
    float mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        for (int a = 0; a < 3; a++) mn[a] = fminf(mn[a], partial[8 * i + a]), mx[a] = fmaxf(mx[a], partial[8 * i + 3 + a]);
    bbox_block_reduce(mn, mx, bbox);
}

__device__ __forceinline__ uint32_t prep_morton(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FF;
    x = (x | (x << 8)) & 0x0300F00F;
    x = (x | (x << 4)) & 0x030C30C3;
    x = (x | (x << 2)) & 0x09249249;
    return x;
}
// CUDA float -> uint32 conversion semantics (NaN -> 0, saturating) for the degenerate 0/0 axis.
__device__ __forceinline__ uint32_t f2u(float v) {
    if (!(v == v) || v <= 0.f) return 0u;
    if (v >= 4294967296.f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}

// coord2Morton, simple_knn.cu:54-70
__global__ void morton_kernel(int P, int P2, const float* __restrict__ xyz, const float* __restrict__ bbox, uint64_t* __restrict__ keys) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P2) return;
    if (i >= P) {
        keys[i] = ~0ull;
        return;
    }
    const float mnx = bbox[0], mny = bbox[1], mnz = bbox[2], mxx = bbox[3], mxy = bbox[4], mxz = bbox[5];
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const uint32_t cx = prep_morton(f2u(((x - mnx) / (mxx - mnx)) * (float)((1 << 10) - 1)));
    const uint32_t cy = prep_morton(f2u(((y - mny) / (mxy - mny)) * (float)((1 << 10) - 1)));
    const uint32_t cz = prep_morton(f2u(((z - mnz) / (mxz - mnz)) * (float)((1 << 10) - 1)));
    const uint32_t code = cx | (cy << 1) | (cz << 2);
    keys[i] = ((uint64_t)code << 32) | (uint32_t)i;  // unique keys: order == stable sort by code
}

// The query search's reference set is not bound to the reference's 10 bits per axis (its ties are "resolved arbitrarily"): 13 bits per
// axis (39-bit code above a 25-bit index: up to 33 M points) keep the 1024-point Morton boxes tight when the points spread over tens of
// metres — the per-object growth search moves every object into a cell of its own (dqo_mapgrowth.object_offsets), and at 10 bits a
// 30 m extent means 3 cm cells: boxes of neighbouring surfels overlap and the scan visits 2.3x the sub-boxes.
constexpr int FINE_BITS = 13, FINE_IDX_BITS = 25;
__device__ __forceinline__ uint64_t prep_morton64(uint64_t x) {  // bit i -> bit 3 i, up to 21 bits
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
// the 39-bit code of a position on the grid laid over `bbox`; a position outside the box takes the code of the nearest cell
__device__ __forceinline__ uint64_t morton_fine_code(float x, float y, float z, const float* __restrict__ bbox) {
#pragma clang fp contract(off)
    const float mnx = bbox[0], mny = bbox[1], mnz = bbox[2], mxx = bbox[3], mxy = bbox[4], mxz = bbox[5];
    const float top = (float)((1 << FINE_BITS) - 1);
    const uint64_t cx = prep_morton64(min(f2u(((x - mnx) / (mxx - mnx)) * top), (uint32_t)top));
    const uint64_t cy = prep_morton64(min(f2u(((y - mny) / (mxy - mny)) * top), (uint32_t)top));
    const uint64_t cz = prep_morton64(min(f2u(((z - mnz) / (mxz - mnz)) * top), (uint32_t)top));
    return cx | (cy << 1) | (cz << 2);
}
__global__ void morton_fine_kernel(int P, int P2, const float* __restrict__ xyz, const float* __restrict__ bbox, uint64_t* __restrict__ keys,
                                   const int32_t* __restrict__ group) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P2) return;
    if (i >= P) {
        keys[i] = ~0ull;
        return;
    }
    if (!knn_in_group(group, i)) {  // behind every real point (the padding keys ~0 are larger still)
        keys[i] = (((1ull << (3 * FINE_BITS)) - 1ull) << FINE_IDX_BITS) | (uint64_t)i;
        return;
    }
    keys[i] = (morton_fine_code(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], bbox) << FINE_IDX_BITS) | (uint64_t)i;
}

// ---- stable LSD radix sort, one 8-bit pass = three kernels ----
// The digit of a key: eight bits of it, or (BY_GROUP: the pass that sorts dqo_nn1_grouped's queries by object) the group id of the row
// the key's index bits name — [0, 64), 64 for a row without a group, so those sort behind every object.
template <bool BY_GROUP>
__device__ __forceinline__ uint32_t radix_digit(uint64_t key, int shift, const int32_t* __restrict__ group) {
    if (!BY_GROUP) return (uint32_t)(key >> shift) & 255u;
    const int gid = group[(uint32_t)key & ((1u << 25) - 1u)];  // (FINE_IDX_BITS index bits)
    return gid >= 0 && gid < 64 ? (uint32_t)gid : 64u;
}
// (1) digit histogram of every block of RDX_BLK keys, stored digit-major: hist[digit][block]
template <bool BY_GROUP>
__global__ __launch_bounds__(RDX_T) void radix_hist_kernel(int n, const uint64_t* __restrict__ keys, int shift, uint32_t* __restrict__ hist,
                                                            int nblk, const int32_t* __restrict__ group) {
    __shared__ uint32_t s[256];
    s[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * RDX_BLK;
#pragma unroll
    for (int r = 0; r < RDX_KPT; r++) {
        const int i = base + r * RDX_T + threadIdx.x;
        if (i < n) atomicAdd(&s[radix_digit<BY_GROUP>(keys[i], shift, group)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s[threadIdx.x];
}
// (2) one block per digit: exclusive prefix over that digit's row (its count in block 0, 1, ...) in place, the row's total to tot[digit]
__global__ __launch_bounds__(256) void radix_scan_kernel(uint32_t* __restrict__ hist, int nblk, uint32_t* __restrict__ tot) {
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* row = hist + (size_t)blockIdx.x * nblk;
    const int per = (nblk + 255) / 256, a = tid * per, b = min(nblk, a + per);
    uint32_t sum = 0;
    for (int i = a; i < b; i++) sum += row[i];
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t pre = incl - sum;
    for (int w = 0; w < wave; w++) pre += s_w[w];
    for (int i = a; i < b; i++) {
        const uint32_t h = row[i];
        row[i] = pre;
        pre += h;
    }
    if (tid == 255) tot[blockIdx.x] = pre;  // (the last thread's running sum is the row total)
}
// (3) scatter: key -> offs[digit][block] + its rank among the block's keys of the same digit, in block order (stable)
template <bool BY_GROUP>
__global__ __launch_bounds__(RDX_T) void radix_scatter_kernel(int n, const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int shift,
                                                               const uint32_t* __restrict__ offs, int nblk,
                                                               const uint32_t* __restrict__ tot, const int32_t* __restrict__ group) {
    __shared__ uint32_t s_run[256];              // next free position of every digit (earlier rounds of this block included)
    __shared__ uint32_t s_wc[RDX_T / 64][256];   // this round's keys per (wave, digit)
    __shared__ uint32_t s_t[RDX_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // where digit `tid` starts in the output = the keys of all smaller digits: exclusive prefix over the 256 row totals
        const uint32_t t = tot[tid];
        uint32_t incl = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_t[wave] = incl;
        __syncthreads();
        uint32_t pre = incl - t;
        for (int w = 0; w < wave; w++) pre += s_t[w];
        s_run[tid] = pre + offs[(size_t)tid * nblk + blockIdx.x];
    }
#pragma unroll
    for (int w = 0; w < RDX_T / 64; w++) s_wc[w][tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * RDX_BLK;
    for (int r = 0; r < RDX_KPT; r++) {
        const int i = base + r * RDX_T + tid;
        const bool valid = i < n;
        const uint64_t key = valid ? in[i] : 0ull;
        const uint32_t d = valid ? radix_digit<BY_GROUP>(key, shift, group) : 0u;
        // the lanes of this wave that hold the same digit: eight ballots
        unsigned long long peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = ((d >> bit) & 1u) != 0u;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(one);
            peers &= one ? bal : ~bal;
        }
        const uint32_t rank_w = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank_w == 0u) s_wc[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = s_run[d] + rank_w;
            for (int w = 0; w < wave; w++) pos += s_wc[w][d];
            out[pos] = key;
        }
        __syncthreads();
        {   // digit `tid`: advance its position by this round's keys, clear the round's counts
            uint32_t c = 0;
#pragma unroll
            for (int w = 0; w < RDX_T / 64; w++) c += s_wc[w][tid], s_wc[w][tid] = 0;
            s_run[tid] += c;
        }
        __syncthreads();
    }
}

// group (dqo_knn3_query_grouped): the point's group id + 1 rides in bits 25..31 of the index word (0 = the point belongs to no group)
constexpr int KNN_GROUP_SHIFT = 25;
__global__ void gather_sorted_kernel(int P, const float* __restrict__ xyz, const uint64_t* __restrict__ keys, float4* __restrict__ sorted,
                                     uint64_t idx_mask, const int32_t* __restrict__ group) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t src = (uint32_t)(keys[i] & idx_mask);
    uint32_t w = src;
    if (group != nullptr) {
        const int gid = group[src];
        if (!(gid >= 0 && gid < 64)) {
            sorted[i] = make_float4(1e18f, 1e18f, 1e18f, __uint_as_float(w));  // no group: a far sentinel (group word 0 matches no query)
            return;
        }
        w |= (uint32_t)(gid + 1) << KNN_GROUP_SHIFT;
    }
    sorted[i] = make_float4(xyz[3 * src], xyz[3 * src + 1], xyz[3 * src + 2], __uint_as_float(w));
}

// Every pruning record (level-1 box, run of 64 points, group of 64 boxes: 8 floats, 6 of them min / max) carries in its two spare words
// the SET OF GROUPS present among its points (dqo_knn3_query_grouped; all zero without groups): a record without the query's group is
// skipped whatever its distance — objects are spatially coherent, so most Morton boxes hold one or two of them.
__device__ __forceinline__ unsigned long long knn_group_bit(float w) {
    const uint32_t g1 = __float_as_uint(w) >> KNN_GROUP_SHIFT;  // group id + 1, 0 = none (always 0 in an ungrouped build of the set)
    return g1 ? 1ull << (g1 - 1u) : 0ull;
}
__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}
__device__ __forceinline__ unsigned long long knn_record_groups(const float* rec) {
    return ((unsigned long long)__float_as_uint(rec[7]) << 32) | (unsigned long long)__float_as_uint(rec[6]);
}
// boxMinMax, simple_knn.cu:78-117
__global__ __launch_bounds__(256) void box_minmax_kernel(int P, const float4* __restrict__ sorted, float* __restrict__ boxes, int grouped) {
    __shared__ float s[6][4];
    __shared__ unsigned long long s_g[4];
    const int b = blockIdx.x;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    unsigned long long gm = 0ull;
    for (int i = b * KNN_BOX + threadIdx.x; i < min(P, (b + 1) * KNN_BOX); i += blockDim.x) {
        const float4 p = sorted[i];
        mn[0] = fminf(mn[0], p.x), mn[1] = fminf(mn[1], p.y), mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x), mx[1] = fmaxf(mx[1], p.y), mx[2] = fmaxf(mx[2], p.z);
        if (grouped) gm |= knn_group_bit(p.w);
    }
    gm = wave_or64(gm);
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        for (int a = 0; a < 3; a++) s[a][wave] = mn[a], s[3 + a][wave] = mx[a];
        s_g[wave] = gm;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = s[threadIdx.x][0];
        for (int w = 1; w < 4; w++) r = threadIdx.x < 3 ? fminf(r, s[threadIdx.x][w]) : fmaxf(r, s[threadIdx.x][w]);
        boxes[8 * b + threadIdx.x] = r;
    } else if (threadIdx.x < 8) {
        const unsigned long long g = s_g[0] | s_g[1] | s_g[2] | s_g[3];
        boxes[8 * b + threadIdx.x] = __uint_as_float(threadIdx.x == 6 ? (uint32_t)g : (uint32_t)(g >> 32));
    }
}

// updateKBest_idx, simple_knn.cu:147-167 (strict '>' keeps the earlier-visited candidate on ties)
__device__ __forceinline__ void kbest(const float4 ref, const float4 cand, float (&best)[3], int (&bidx)[3]) {
#pragma clang fp contract(off)
    const float dx = cand.x - ref.x, dy = cand.y - ref.y, dz = cand.z - ref.z;
    float dist = dx * dx + dy * dy + dz * dz;
    int id = (int)__float_as_uint(cand.w);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if (best[j] > dist) {
            const float t = best[j];
            best[j] = dist;
            dist = t;
            const int r = bidx[j];
            bidx[j] = id;
            id = r;
        }
    }
}

// distBoxPoint, simple_knn.cu:119-129
__device__ __forceinline__ float dist_box_point(const float* bx, const float4 p) {
#pragma clang fp contract(off)
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (p.x < bx[0] || p.x > bx[3]) dx = fminf(fabsf(p.x - bx[0]), fabsf(p.x - bx[3]));
    if (p.y < bx[1] || p.y > bx[4]) dy = fminf(fabsf(p.y - bx[1]), fabsf(p.y - bx[4]));
    if (p.z < bx[2] || p.z > bx[5]) dz = fminf(fabsf(p.z - bx[2]), fabsf(p.z - bx[5]));
    return dx * dx + dy * dy + dz * dz;
}

// boxMeanDist, simple_knn.cu:169-214.  One lane per (Morton-sorted) query; a wave's 64 queries are spatially close, so a
// box is scanned by the whole wave if ANY lane still needs it: candidate loads are wave-uniform (one broadcast load
// feeds 64 lanes) and lanes that did not need the box are unaffected (its points can never enter their top 3).
// Second level (not in the reference; changes no result): a box of 1024 Morton-consecutive points is a loose volume, so before its
// points are scanned each of its sixteen runs of 64 points is tested against its own bounding box with the same predicate — a run
// that fails it for every lane holds no point that could enter any lane's top 3 (strict '>' in kbest), and the runs that are scanned
// are scanned in the reference's order.  540 k points: 9.8 -> 1.5 ms.
__global__ __launch_bounds__(256) void knn_scan_kernel(int P, const float4* __restrict__ sorted, const float* __restrict__ boxes,
                                                       const float* __restrict__ sub, float* __restrict__ mean_d2,
                                                       int32_t* __restrict__ idx3) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < P;
    const float4 me = live ? sorted[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    float best[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    int bidx[3] = {INT_MAX, INT_MAX, INT_MAX};
    if (live)
        for (int i = max(0, idx - 3); i <= min(P - 1, idx + 3); i++) {
            if (i == idx) continue;
            kbest(me, sorted[i], best, bidx);
        }
    const float reject = best[2];
    best[0] = best[1] = best[2] = FLT_MAX;
    bidx[0] = bidx[1] = bidx[2] = INT_MAX;
    const int nb = (P + KNN_BOX - 1) / KNN_BOX;
    for (int b = 0; b < nb; b++) {
        float bx[6];
#pragma unroll
        for (int a = 0; a < 6; a++) bx[a] = boxes[8 * b + a];
        const float d = dist_box_point(bx, me);
        const bool need = live && !(d > reject || d > best[2]);
        if (__ballot(need) == 0) continue;
        const int lo = b * KNN_BOX, hi = min(P, (b + 1) * KNN_BOX);
        for (int r0 = lo; r0 < hi; r0 += KNN_SUB) {
            float sx[6];
#pragma unroll
            for (int a = 0; a < 6; a++) sx[a] = sub[8 * (r0 / KNN_SUB) + a];  // wave-uniform address
            const float ds = dist_box_point(sx, me);
            const bool need_run = need && !(ds > reject || ds > best[2]);
            if (__ballot(need_run) == 0) continue;
            const int r1 = min(hi, r0 + KNN_SUB);
            for (int i = r0; i < r1; i++) {
                const float4 c = sorted[i];  // wave-uniform address
                if (need_run && i != idx) kbest(me, c, best, bidx);
            }
        }
    }
    if (live) {
        const uint32_t dst = __float_as_uint(me.w);
        mean_d2[dst] = (best[0] + best[1] + best[2]) / 3.0f;
        idx3[dst * 3 + 0] = bidx[0];
        idx3[dst * 3 + 1] = bidx[1];
        idx3[dst * 3 + 2] = bidx[2];
    }
}

// min / max of each run of 64 sorted points: one wave per run
__global__ __launch_bounds__(256) void sub_minmax_kernel(int P, const float4* __restrict__ sorted, float* __restrict__ sub) {
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const int ns = (P + KNN_SUB - 1) / KNN_SUB;
    if (w >= ns) return;
    const int i = w * KNN_SUB + lane;
    const float4 p = sorted[min(i, P - 1)];  // (the run's last point again for the padding lanes: no effect on min / max)
    float mn[3] = {p.x, p.y, p.z}, mx[3] = {p.x, p.y, p.z};
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    const unsigned long long g = wave_or64(i < P ? knn_group_bit(p.w) : 0ull);
    if (lane < 3) sub[8 * w + lane] = lane == 0 ? mn[0] : (lane == 1 ? mn[1] : mn[2]);
    else if (lane < 6) sub[8 * w + lane] = lane == 3 ? mx[0] : (lane == 4 ? mx[1] : mx[2]);
    else if (lane < 8) sub[8 * w + lane] = __uint_as_float(lane == 6 ? (uint32_t)g : (uint32_t)(g >> 32));
}

// third pruning level of the query search: min / max over runs of 64 level-1 boxes (one wave per group)
__global__ __launch_bounds__(256) void group_minmax_kernel(int nb, const float* __restrict__ boxes, float* __restrict__ groups) {
    const int gidx = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const int ng = (nb + 63) / 64;
    if (gidx >= ng) return;
    const float* bx = boxes + 8 * (size_t)min(gidx * 64 + lane, nb - 1);  // (the last box again for the padding lanes)
    float mn[3] = {bx[0], bx[1], bx[2]}, mx[3] = {bx[3], bx[4], bx[5]};
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    const unsigned long long g = wave_or64(gidx * 64 + lane < nb ? knn_record_groups(bx) : 0ull);
    if (lane < 3) groups[8 * gidx + lane] = lane == 0 ? mn[0] : (lane == 1 ? mn[1] : mn[2]);
    else if (lane < 6) groups[8 * gidx + lane] = lane == 3 ? mx[0] : (lane == 4 ? mx[1] : mx[2]);
    else if (lane < 8) groups[8 * gidx + lane] = __uint_as_float(lane == 6 ? (uint32_t)g : (uint32_t)(g >> 32));
}

// wave64 minimum, result wave-uniform.  DPP lanes that are not written keep `v` itself (old = v), so the minimum is unaffected.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_self(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_min_f(float v) {
    v = fminf(v, dpp_self<0xB1, 0xF>(v));   // quad_perm [1,0,3,2]
    v = fminf(v, dpp_self<0x4E, 0xF>(v));   // quad_perm [2,3,0,1]
    v = fminf(v, dpp_self<0x141, 0xF>(v));  // row_half_mirror
    v = fminf(v, dpp_self<0x140, 0xF>(v));  // row_mirror: every lane holds its row's minimum
    v = fminf(v, dpp_self<0x142, 0xA>(v));  // row_bcast15 into rows 1, 3
    v = fminf(v, dpp_self<0x143, 0xC>(v));  // row_bcast31 into rows 2, 3: lane 63 holds the wave's minimum
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// K = 3 nearest REFERENCE points of every QUERY point (row f3: Mapping.temp_points_filter, SLAM/multiprocess/mapper.py:
// 1351-1380, which calls pytorch3d.ops.knn_points(temp_xyz, exist_xyz, K=3, norm=2): exact squared L2 distances, ascending).
// ONE WAVE PER QUERY.  The references are Morton-sorted and boxed on two levels (runs of 1024 and of 64 points).  The wave's 64
// lanes test 64 level-1 boxes per trip; a box that cannot be excluded (box distance <= current third-best) has its 16 sub-boxes
// tested by 16 lanes, and a sub-box that cannot be excluded is ONE coalesced wave load: 64 candidates, one per lane, merged into
// the (wave-uniform) top 3 by up to three wave minima.  The first pass finds the level-1 box nearest to the query and scans it, so
// the second pass starts with finite bounds.  (The first version gave each query a lane and scanned a box with the whole wave as
// soon as ANY of its 64 queries needed it: with few queries against a large map — the growth step's 40 800 new points against
// 2 M Gaussians — a wave's queries lie far apart and it scanned ~45 boxes of 1024 points each: 39 ms, now 1 ms.)
// GROUPED (dqo_knn3_query_grouped): a reference only counts for a query of the same group (ids in [0, 64); a point with another id
// belongs to no group) and, with `group_box`, if it lies strictly inside its group's box [lo xyz, hi xyz] — the per-object growth
// decisions of the mapper in one search over the map as it is stored: no shifted copies, no gathered subsets.
template <bool GROUPED>
__global__ __launch_bounds__(256) void knn_query_wave_kernel(int Q, const float* __restrict__ q_xyz, int R,
                                                             const float4* __restrict__ sorted_r, const float* __restrict__ boxes,
                                                             const float* __restrict__ sub, const float* __restrict__ groups,
                                                             float* __restrict__ dist2, int32_t* __restrict__ idx3, const float bound2,
                                                             const int32_t* __restrict__ q_group, const float* __restrict__ group_box) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (q >= Q) return;
    const float4 me = make_float4(q_xyz[3 * q], q_xyz[3 * q + 1], q_xyz[3 * q + 2], 0.f);
    uint32_t my_group = 0u;  // group id + 1
    unsigned long long my_bit = ~0ull;
    float gl0 = -FLT_MAX, gl1 = -FLT_MAX, gl2 = -FLT_MAX, gh0 = FLT_MAX, gh1 = FLT_MAX, gh2 = FLT_MAX;
    if (GROUPED) {
        const int gid = q_group[q];
        if (!(gid >= 0 && gid < 64)) {  // a query without a group has no neighbours
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) dist2[3 * q + k] = FLT_MAX, idx3[3 * q + k] = -1;
            }
            return;
        }
        my_group = (uint32_t)(gid + 1);
        my_bit = 1ull << gid;
        if (group_box != nullptr) {
            const float* b = group_box + 6 * gid;
            gl0 = b[0], gl1 = b[1], gl2 = b[2], gh0 = b[3], gh1 = b[4], gh2 = b[5];
        }
    }
    // wave-uniform top 3 (ascending).  bound2 (dqo_knn3_query_within): only references closer than sqrt(bound2) count — the search starts
    // with that bound instead of an open one, so a query far from every reference prunes the whole map at once
    float b0 = bound2, b1 = bound2, b2 = bound2;
    int i0 = -1, i1 = -1, i2 = -1;
    const int nb = (R + KNN_BOX - 1) / KNN_BOX, ns = (R + KNN_SUB - 1) / KNN_SUB;

    auto scan_sub = [&](int sb) {
        const int i = sb * KNN_SUB + lane;
        const float4 c = sorted_r[min(i, R - 1)];
        float dist;
        {
#pragma clang fp contract(off)
            const float dx = c.x - me.x, dy = c.y - me.y, dz = c.z - me.z;
            dist = i < R ? dx * dx + dy * dy + dz * dz : FLT_MAX;
        }
        if (GROUPED) {
            const bool ok = (__float_as_uint(c.w) >> KNN_GROUP_SHIFT) == my_group && c.x > gl0 && c.y > gl1 && c.z > gl2 && c.x < gh0 &&
                            c.y < gh1 && c.z < gh2;
            dist = ok ? dist : FLT_MAX;
        }
        const int cid = (int)(__float_as_uint(c.w) & (GROUPED ? (1u << KNN_GROUP_SHIFT) - 1u : 0xffffffffu));
        for (int rep = 0; rep < 3; rep++) {
            const float m = wave_min_f(dist);
            if (!(m < b2)) break;
            const int owner = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(dist == m));
            const int id = __builtin_amdgcn_readlane(cid, owner);
            if (m < b0) b2 = b1, i2 = i1, b1 = b0, i1 = i0, b0 = m, i0 = id;
            else if (m < b1) b2 = b1, i2 = i1, b1 = m, i1 = id;
            else b2 = m, i2 = id;
            if (lane == owner) dist = FLT_MAX;
        }
    };
    auto scan_box = [&](int b) {
        const int s = b * (KNN_BOX / KNN_SUB) + lane;
        const bool in = lane < KNN_BOX / KNN_SUB && s < ns;
        const float ds = in ? dist_box_point(sub + 8 * (size_t)s, me) : FLT_MAX;
        const bool has = !GROUPED || (in && (knn_record_groups(sub + 8 * (size_t)s) & my_bit) != 0ull);
        unsigned long long m2 = __builtin_amdgcn_ballot_w64(in && has && !(ds > b2));
        while (m2 != 0ull) {
            const int l = (int)__builtin_ctzll(m2);
            m2 &= m2 - 1ull;
            const float dl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ds), l));
            if (dl > b2) continue;  // the bound has tightened since the ballot
            scan_sub(b * (KNN_BOX / KNN_SUB) + l);
        }
    };
    // pass 1: the level-1 box nearest to the query
    int bmin = 0;
    {
        float dmin = FLT_MAX;
        int bl = 0;
        for (int bb = 0; bb < nb; bb += 64) {
            const int b = bb + lane;
            float d = b < nb ? dist_box_point(boxes + 8 * (size_t)b, me) : FLT_MAX;
            if (GROUPED && b < nb && (knn_record_groups(boxes + 8 * (size_t)b) & my_bit) == 0ull) d = FLT_MAX;  // (nothing of the query's group)
            if (d < dmin) dmin = d, bl = b;
        }
        const float m = wave_min_f(dmin);
        const int owner = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(dmin == m));
        bmin = __builtin_amdgcn_readlane(bl, owner);
    }
    scan_box(bmin);
    // pass 2: every other box that cannot be excluded, group by group (runs of 64 boxes = 65 536 sorted points: a group that cannot hold
    // a better candidate is skipped whole — 31 group tests instead of 1954 box tests against a 2 M-point map)
    const int ng = (nb + 63) / 64;
    for (int gg = 0; gg < ng; gg += 64) {
        const int gr = gg + lane;
        const float dg = gr < ng ? dist_box_point(groups + 8 * (size_t)gr, me) : FLT_MAX;
        const bool hasg = !GROUPED || (gr < ng && (knn_record_groups(groups + 8 * (size_t)gr) & my_bit) != 0ull);
        unsigned long long mg = __builtin_amdgcn_ballot_w64(gr < ng && hasg && !(dg > b2));
        while (mg != 0ull) {
            const int lg = (int)__builtin_ctzll(mg);
            mg &= mg - 1ull;
            const float dgl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dg), lg));
            if (dgl > b2) continue;  // the bound has tightened since the ballot
            const int b = (gg + lg) * 64 + lane;
            const bool in = b < nb && b != bmin;
            const float d = in ? dist_box_point(boxes + 8 * (size_t)b, me) : FLT_MAX;
            const bool hasb = !GROUPED || (in && (knn_record_groups(boxes + 8 * (size_t)b) & my_bit) != 0ull);
            unsigned long long m1 = __builtin_amdgcn_ballot_w64(in && hasb && !(d > b2));
            while (m1 != 0ull) {
                const int l = (int)__builtin_ctzll(m1);
                m1 &= m1 - 1ull;
                const float dl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), l));
                if (dl > b2) continue;
                scan_box((gg + lg) * 64 + l);
            }
        }
    }
    if (lane == 0) {  // (a slot no reference made it into: FLT_MAX / -1, whatever the starting bound was)
        dist2[3 * q + 0] = i0 >= 0 ? b0 : FLT_MAX, dist2[3 * q + 1] = i1 >= 0 ? b1 : FLT_MAX, dist2[3 * q + 2] = i2 >= 0 ? b2 : FLT_MAX;
        idx3[3 * q + 0] = i0, idx3[3 * q + 1] = i1, idx3[3 * q + 2] = i2;
    }
}


// ---- dqo_nn1 / dqo_nn1_grouped: the exact nearest REFERENCE of every QUERY when both sets are large and lie among each other ----------
// (eval_pcd, SLAM/eval.py:190-226: scipy's KDTree(a).query(b), one million points against one million; metric_obj.py:169-236: the same
// for every object's cloud against that object's own mesh.)  knn_query_wave_kernel puts a wave on every query: right for few scattered
// queries, but a million queries among a million references repeat the same walk over the level-1 boxes a million times.  Here the
// QUERIES are sorted too — by their Morton code on the REFERENCE's grid, so that a wave's 64 lanes hold 64 neighbouring queries — and the
// search is knn_scan_kernel's: one lane per query, a record (group of 64 boxes, box, run of 64 points) is opened by the whole wave when
// any lane cannot exclude it, its candidates arrive by wave-uniform loads.  K = 1, so a lane keeps one distance; the references either
// side of its own rank among the reference keys come first, then the box that rank falls into.
// ONE SEARCH, THREE ROW SOURCES.  Every row of either set has a group word, id + 1, 0 = the row takes no part (DqoNn1Rows): 1 for every
// row (the plain search), keep[i] != 0 (a keep byte column: the kept rows are object 0) or an int32 id column (up to 64 objects).  A
// query's word rides in bits 25..31 of its index word.  A reference set WITH a source is built on knn_build's group path (a row without
// a group: outside the bounding box, sorted last, a far sentinel; the word in a point's index word, the set of groups under it in every
// record) and scanned with FILTER: a record is opened only if one of the lanes that cannot exclude it belongs to a group the record
// holds (a ballot over `need && (record's set & my bit)`: the record's set is wave-uniform), and a lane takes a candidate only if the
// candidate's word is its own — so a lane may start without a bound, and then opens every record that holds its group until it has met
// a reference of its own.  A reference set WITHOUT one is built without groups (its words are 0) and scanned with those tests compiled
// out.  Queries given by ids are sorted by object first (the sort's last pass takes the id as its digit), so a wave holds one object
// where it can; dropped queries sort last by their all-ones code either way.  Every candidate a lane takes is a reference of its group,
// every record it skips holds none of its group or has dist_box_point > its best: the result is the minimum of kbest's float
// expression over ALL references of the query's group, bit for bit, whatever the order and whichever source named the group.
constexpr uint32_t NN1_IDX_MASK = (1u << FINE_IDX_BITS) - 1u;
static_assert(FINE_IDX_BITS == KNN_GROUP_SHIFT, "a query's group word sits where knn_build puts a reference's");

__device__ __forceinline__ uint32_t nn1_row_group(const DqoNn1Rows rows, int i) {
    if (rows.ids != nullptr) return knn_in_group(rows.ids, i) ? (uint32_t)(rows.ids[i] + 1) : 0u;
    return rows.keep == nullptr || rows.keep[i] != 0 ? 1u : 0u;
}

// the point as it is searched: row i under the row-major 3x4 transform m (NULL: as stored) — open3d's rec_pc.transform(transform)
__device__ __forceinline__ float4 nn1_point(const float* __restrict__ xyz, const float* __restrict__ m, int i) {
#pragma clang fp contract(off)
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (m == nullptr) return make_float4(x, y, z, 0.f);
    return make_float4((m[0] * x + m[1] * y) + m[2] * z + m[3], (m[4] * x + m[5] * y) + m[6] * z + m[7],
                       (m[8] * x + m[9] * y) + m[10] * z + m[11], 0.f);
}

// reference side, only with a mask or a transform: the transformed rows and / or the group ids knn_build reads
__global__ void nn1_prepare_ref_kernel(int R, const float* __restrict__ xyz, const uint8_t* __restrict__ keep, const float* __restrict__ xform,
                                       float* __restrict__ txyz, int32_t* __restrict__ grp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    if (txyz != nullptr) {
        const float4 p = nn1_point(xyz, xform, i);
        txyz[3 * (size_t)i] = p.x, txyz[3 * (size_t)i + 1] = p.y, txyz[3 * (size_t)i + 2] = p.z;
    }
    if (grp != nullptr) grp[i] = keep[i] != 0 ? 0 : -1;
}

// query keys on the reference's grid; a query that takes no part sorts behind every one that does
__global__ void nn1_query_keys_kernel(int Q, const float* __restrict__ xyz, DqoNn1Rows rows, const float* __restrict__ xform,
                                      const float* __restrict__ ref_bbox, uint64_t* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    uint64_t code = (1ull << (3 * FINE_BITS)) - 1ull;
    if (nn1_row_group(rows, i) != 0u) {
        const float4 p = nn1_point(xyz, xform, i);
        code = morton_fine_code(p.x, p.y, p.z, ref_bbox);
    }
    keys[i] = (code << FINE_IDX_BITS) | (uint64_t)i;
}

// the sorted query: xyz under the transform, the row index and the group word above it (0: the point is not searched for)
__global__ void nn1_gather_query_kernel(int Q, const float* __restrict__ xyz, DqoNn1Rows rows, const float* __restrict__ xform,
                                        const uint64_t* __restrict__ keys, float4* __restrict__ sorted_q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    const uint32_t src = (uint32_t)keys[i] & NN1_IDX_MASK;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t w = src;
    const uint32_t g1 = nn1_row_group(rows, (int)src);
    if (g1 != 0u) p = nn1_point(xyz, xform, (int)src), w |= g1 << KNN_GROUP_SHIFT;
    p.w = __uint_as_float(w);
    sorted_q[i] = p;
}

// kbest with K = 1; FILTER: only a reference of the lane's own group counts (the sentinel rows carry none)
template <bool FILTER>
__device__ __forceinline__ void nn1_take(const float4 me, const float4 cand, uint32_t my_group, float& best, int& bidx) {
#pragma clang fp contract(off)
    const float dx = cand.x - me.x, dy = cand.y - me.y, dz = cand.z - me.z;
    const float dist = dx * dx + dy * dy + dz * dz;
    const uint32_t w = __float_as_uint(cand.w);
    // (two selects, not a branch: a run's candidates stay in one block, so their wave-uniform loads are merged and issued ahead)
    const bool take = (!FILTER || (w >> KNN_GROUP_SHIFT) == my_group) && dist < best;
    best = take ? dist : best, bidx = take ? (int)(w & NN1_IDX_MASK) : bidx;
}

// by_rank (dqo_eval_pcd_grouped; may be NULL): the result in the queries' SORTED order too, {dist2, group id (64: none)} of sorted query q —
// an object's rows are contiguous there, which is what the reduction's fixed summation order is laid over.  dist2 may be NULL then.
template <bool FILTER>
__global__ __launch_bounds__(256) void nn1_scan_kernel(int Q, const float4* __restrict__ sorted_q, const uint64_t* __restrict__ keys_q, int R,
                                                       const float4* __restrict__ sorted_r, const uint64_t* __restrict__ keys_r,
                                                       const float* __restrict__ boxes, const float* __restrict__ sub,
                                                       const float* __restrict__ groups, float* __restrict__ dist2, int32_t* __restrict__ idx,
                                                       float2* __restrict__ by_rank) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const float4 me = q < Q ? sorted_q[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t my_w = __float_as_uint(me.w);
    const uint32_t my_group = q < Q ? my_w >> KNN_GROUP_SHIFT : 0u;  // id + 1
    const bool live = my_group != 0u;
    const unsigned long long my_bit = live ? 1ull << (my_group - 1u) : 0ull;
    float best = FLT_MAX;
    int bidx = -1, rank = 0;
    if (live) {  // the first reference key not below the query's code, and the two references either side of it: candidates like any other
        const uint64_t key = (keys_q[q] >> FINE_IDX_BITS) << FINE_IDX_BITS;
        int lo = 0, hi = R;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys_r[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        rank = lo;
        for (int i = max(0, rank - 2); i <= min(R - 1, rank + 1); i++) nn1_take<FILTER>(me, sorted_r[i], my_group, best, bidx);
    }
    const int nb = (R + KNN_BOX - 1) / KNN_BOX, ng = (nb + 63) / 64;
    // a record (wave-uniform address) is opened if a lane cannot exclude it — FILTER: a lane of a group the record holds
    auto wanted = [&](const float* rec) {
        bool mine = true;
        if (FILTER) {
            const unsigned long long held = knn_record_groups(rec);
            if (held == 0ull) return false;
            mine = (held & my_bit) != 0ull;
        }
        const float d = dist_box_point(rec, me);
        return __ballot(live && mine && !(d > best)) != 0;
    };
    auto scan_box = [&](int b) {  // (b wave-uniform: the records and the candidates come by wave-uniform loads)
        if (!wanted(boxes + 8 * (size_t)b)) return;
        const int lo = b * KNN_BOX, hi = min(R, lo + KNN_BOX);
        for (int r0 = lo; r0 < hi; r0 += KNN_SUB) {
            if (!wanted(sub + 8 * (size_t)(r0 / KNN_SUB))) continue;
            // every lane takes every candidate, asked for the run or not (a candidate like any other; a lane without a query is not
            // written).  A full run has a constant trip count: its wave-uniform loads are issued several at a time
            if (r0 + KNN_SUB <= hi) {
#pragma unroll 8
                for (int i = 0; i < KNN_SUB; i++) nn1_take<FILTER>(me, sorted_r[r0 + i], my_group, best, bidx);
            } else {
                for (int i = r0; i < hi; i++) nn1_take<FILTER>(me, sorted_r[i], my_group, best, bidx);
            }
        }
    };
    if (__ballot(live) != 0) {
        // queries that take no part sort last, so lane 0 of a wave with a live lane is live: the box its rank falls into first
        const int home = min(nb - 1, __builtin_amdgcn_readfirstlane(rank) / KNN_BOX);
        scan_box(home);
        for (int g = 0; g < ng; g++) {
            if (!wanted(groups + 8 * (size_t)g)) continue;
            const int b1 = min(nb, (g + 1) * 64);
            for (int b = g * 64; b < b1; b++)
                if (b != home) scan_box(b);
        }
    }
    if (q < Q) {
        const uint32_t dst = my_w & NN1_IDX_MASK;
        const float d = live && bidx >= 0 ? best : FLT_MAX;
        if (dist2 != nullptr) dist2[dst] = d;
        if (idx != nullptr) idx[dst] = live ? bidx : -1;
        if (by_rank != nullptr) by_rank[q] = make_float2(d, __uint_as_float(live ? my_group - 1u : 64u));
    }
}

__global__ void nn1_fill_kernel(int Q, float* __restrict__ dist2, int32_t* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    dist2[i] = FLT_MAX;
    if (idx != nullptr) idx[i] = -1;
}

struct Nn1Ws {
    KnnWs r, q;
    float* txyz;    // [R][3] the reference rows under ref_xform
    int32_t* grp;   // [R] 0 = kept, -1 = dropped
    size_t total;
};
inline Nn1Ws nn1_ws(void* base, int Q, int R) {
    Nn1Ws w;
    DqoCarver k(base);
    w.r = knn_ws(k.take_raw(knn_ws(nullptr, R).total), R);  // (a set's layout is one part of its own size)
    w.q = knn_ws(k.take_raw(knn_ws(nullptr, Q).total), Q);
    w.txyz = k.take<float>(12 * (size_t)R);
    w.grp = k.take<int32_t>(4 * (size_t)R);
    w.total = k.total();
    return w;
}

}  // namespace

static size_t dqo_knn3_ws_bytes(int P) { return knn_ws(nullptr, P).total; }

// Stable sort of w.keys[0, P) by the Morton code.  The code sits in bits 32..61 of the key: four stable 8-bit passes; the second key buffer
// is `sorted` (16 B per point, written by the gather only after the sort); an even number of passes leaves the result in w.keys.
// (fine codes: 39 bits above the 25-bit index — five passes; an even pass count leaves the result in w.keys, so a sixth pass
// sorts by the top byte once more: a stable sort of sorted keys by a prefix of the key moves nothing but the buffer)
// by_group (dqo_nn1_grouped's queries, fine codes only): that sixth pass sorts by the rows' group ids instead — by object, and within an
// object by code, since every pass is stable.
static int knn_radix_sort(int P, const KnnWs& w, bool fine, hipStream_t s, const int32_t* by_group = nullptr) {
    const int nblk = (P + RDX_BLK - 1) / RDX_BLK;
    uint64_t* a = w.keys;
    uint64_t* b = reinterpret_cast<uint64_t*>(w.sorted);
    const int n_pass = fine ? 6 : 4, shift0 = fine ? FINE_IDX_BITS : 32;
    for (int pass = 0; pass < n_pass; pass++) {
        const int shift = pass < 5 ? shift0 + 8 * pass : 56;
        const bool grp = by_group != nullptr && pass == 5;
        const auto hist = grp ? radix_hist_kernel<true> : radix_hist_kernel<false>;
        const auto scatter = grp ? radix_scatter_kernel<true> : radix_scatter_kernel<false>;
        DQO_LAUNCH("radix_hist_kernel", hist, dim3(nblk), dim3(RDX_T), s, P, a, shift, w.hist, nblk, by_group);
        DQO_LAUNCH("radix_scan_kernel", radix_scan_kernel, dim3(256), dim3(256), s, w.hist, nblk, w.hist + (size_t)256 * nblk);
        DQO_LAUNCH("radix_scatter_kernel", scatter, dim3(nblk), dim3(RDX_T), s, P, a, b, shift, w.hist, nblk, w.hist + (size_t)256 * nblk,
                   by_group);
        std::swap(a, b);
    }
    return DQO_OK;
}

// bounding box -> Morton keys -> sort -> gather into Morton order (-> boxes)
// fine: morton_fine_kernel's 39-bit codes (the query search's reference set) instead of the reference's 30-bit ones
// gather = false (dqo_mesh_nearest, whose sorted rows are its own three float4 per face): the sorted keys only, w.sorted left as the sort's scratch
static int knn_build(int P, const float* xyz, const KnnWs& w, bool with_boxes, hipStream_t s, bool fine = false, const int32_t* group = nullptr,
                     bool gather = true) {
    fine = fine && P < (1 << FINE_IDX_BITS);
    const int P2 = next_pow2(P < SORT_RUN ? SORT_RUN : P);
    {   // (the partial boxes live at the start of the key array: P2 >= 4096 keys = 32 KB, and the keys are written after the fold)
        const int nb = std::min(BBOX_BLOCKS_MAX, (P + 1023) / 1024);
        float* partial = reinterpret_cast<float*>(w.keys);
        DQO_LAUNCH("bbox_kernel", bbox_kernel, dim3(nb), dim3(1024), s, P, xyz, partial, group);
        DQO_LAUNCH("bbox_fold_kernel", bbox_fold_kernel, dim3(1), dim3(512), s, nb, partial, w.bbox);
    }
    if (fine) DQO_LAUNCH("morton_kernel", morton_fine_kernel, dim3((P2 + 255) / 256), dim3(256), s, P, P2, xyz, w.bbox, w.keys, group);
    else DQO_LAUNCH("morton_kernel", morton_kernel, dim3((P2 + 255) / 256), dim3(256), s, P, P2, xyz, w.bbox, w.keys);
    const int rc = knn_radix_sort(P, w, fine, s);
    if (rc) return rc;
    if (!gather) return DQO_OK;
    DQO_LAUNCH("gather_sorted_kernel", gather_sorted_kernel, dim3((P + 255) / 256), dim3(256), s, P, xyz, w.keys, w.sorted,
               fine ? ((1ull << FINE_IDX_BITS) - 1ull) : 0xffffffffull, group);
    if (with_boxes) {
        const int nb = (P + KNN_BOX - 1) / KNN_BOX;
        DQO_LAUNCH("box_minmax_kernel", box_minmax_kernel, dim3(nb), dim3(256), s, P, w.sorted, w.boxes, group != nullptr ? 1 : 0);
    }
    return DQO_OK;
}

static int dqo_launch_knn3(int P, const float* xyz, float* mean_d2, int32_t* idx3, void* ws, size_t ws_bytes, hipStream_t s) {
    (void)ws_bytes;
    KnnWs w = knn_ws(ws, P);
    int rc = knn_build(P, xyz, w, true, s);
    if (rc) return rc;
    const int ns = (P + KNN_SUB - 1) / KNN_SUB;
    DQO_LAUNCH("sub_minmax_kernel", sub_minmax_kernel, dim3((ns * 64 + 255) / 256), dim3(256), s, P, w.sorted, w.sub);
    DQO_LAUNCH("knn_scan_kernel", knn_scan_kernel, dim3((P + 255) / 256), dim3(256), s, P, w.sorted, w.boxes, w.sub, mean_d2, idx3);
    return DQO_OK;
}

// the reference set of a query search: knn_build on the fine grid, then the two further pruning levels (runs of 64 points, runs of 64 boxes)
static int knn_build_ref(int R, const float* xyz, const KnnWs& w, hipStream_t s, const int32_t* group) {
    const int rc = knn_build(R, xyz, w, true, s, true, group);
    if (rc) return rc;
    const int ns = (R + KNN_SUB - 1) / KNN_SUB, nb = (R + KNN_BOX - 1) / KNN_BOX, ng = (nb + 63) / 64;
    DQO_LAUNCH("sub_minmax_kernel", sub_minmax_kernel, dim3((ns * 64 + 255) / 256), dim3(256), s, R, w.sorted, w.sub);
    DQO_LAUNCH("group_minmax_kernel", group_minmax_kernel, dim3((ng * 64 + 255) / 256), dim3(256), s, nb, w.boxes, w.groups);
    return DQO_OK;
}

static size_t dqo_knn3_query_ws_bytes(int Q, int R) { return knn_ws(nullptr, Q).total + knn_ws(nullptr, R).total; }

static int dqo_launch_knn3_query(int Q, const float* q_xyz, int R, const float* r_xyz, float* dist2, int32_t* idx3, void* ws, size_t ws_bytes,
                                 hipStream_t s, float bound2, const int32_t* q_group, const int32_t* r_group, const float* group_box) {
    (void)ws_bytes;
    KnnWs wr = knn_ws(ws, R);
    const int rc = knn_build_ref(R, r_xyz, wr, s, r_group);
    if (rc) return rc;
    const auto scan = q_group != nullptr ? knn_query_wave_kernel<true> : knn_query_wave_kernel<false>;
    DQO_LAUNCH("knn_query_wave_kernel", scan, dim3(((size_t)Q * 64 + 255) / 256), dim3(256), s, Q, q_xyz, R, wr.sorted, wr.boxes, wr.sub,
               wr.groups, dist2, idx3, bound2, q_group, group_box);
    return DQO_OK;
}

// the index word of a sorted point carries FINE_IDX_BITS index bits
bool dqo_nn1_size_ok(int32_t n) { return n >= 0 && n < (1 << FINE_IDX_BITS); }

size_t dqo_nn1_ws_bytes(int Q, int R) { return nn1_ws(nullptr, Q < 1 ? 1 : Q, R < 1 ? 1 : R).total; }

// The workspace's group column holds a reference keep mask as ids; the caller's own ids are read in place.  Q, R >= 1 when by_rank is
// asked for.
int dqo_launch_nn1(int Q, const float* q_xyz, DqoNn1Rows q_rows, int R, const float* r_xyz, DqoNn1Rows r_rows, const float* q_xform,
                   const float* r_xform, float* dist2, int32_t* idx, float2* by_rank, void* ws, hipStream_t s) {
    if (Q == 0) return DQO_OK;
    if (R == 0) {
        DQO_LAUNCH("nn1_fill_kernel", nn1_fill_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, dist2, idx);
        return DQO_OK;
    }
    const Nn1Ws w = nn1_ws(ws, Q, R);
    const float* ref = r_xyz;
    const int32_t* grp = r_rows.ids;
    if (r_rows.keep != nullptr || r_xform != nullptr) {
        DQO_LAUNCH("nn1_prepare_ref_kernel", nn1_prepare_ref_kernel, dim3((R + 255) / 256), dim3(256), s, R, r_xyz, r_rows.keep, r_xform,
                   r_xform != nullptr ? w.txyz : nullptr, r_rows.keep != nullptr ? w.grp : nullptr);
        if (r_xform != nullptr) ref = w.txyz;
        if (r_rows.keep != nullptr) grp = w.grp;
    }
    int rc = knn_build_ref(R, ref, w.r, s, grp);
    if (rc) return rc;
    DQO_LAUNCH("nn1_query_keys_kernel", nn1_query_keys_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, q_xyz, q_rows, q_xform, w.r.bbox,
               w.q.keys);
    rc = knn_radix_sort(Q, w.q, true, s, q_rows.ids);  // (by object only when there are objects: a keep mask's dropped rows sort last by their code)
    if (rc) return rc;
    DQO_LAUNCH("nn1_gather_query_kernel", nn1_gather_query_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, q_xyz, q_rows, q_xform, w.q.keys,
               w.q.sorted);
    const auto scan = grp != nullptr ? nn1_scan_kernel<true> : nn1_scan_kernel<false>;
    DQO_LAUNCH("nn1_scan_kernel", scan, dim3((Q + 255) / 256), dim3(256), s, Q, w.q.sorted, w.q.keys, R, w.r.sorted, w.r.keys, w.r.boxes, w.r.sub,
               w.r.groups, dist2, idx, by_rank);
    return DQO_OK;
}

// ---- dqo_mesh_nearest: the nearest FACE of a mesh for every query, the exact point-to-triangle distance ----------------------------------
// dqo_nn1's walk with three changes: the references are triangles (sorted along the fine Morton grid of their centroids, gathered as three
// float4: corner a with the face index in .w — -1 for a face that is not valid —, corner b, corner c), the pruning records (runs of 64
// faces, boxes of 1024, groups of 64 boxes; the same 8-float format) are taken over the faces' CORNERS, and the candidate step is the
// point-triangle distance of include/dqo_raster.h: E(p, f), Ericson's seven-region walk one float rounding at a time, clamped from below
// by the face's own bounding box: D(p, f) = fmaxf(E(p, f), B(p, aabb(f))), B = dist_box_point.
// WHY THE CLAMP MAKES PRUNING EXACT.  nn1_scan_kernel skips a record when B(record) > best.  B is monotone under box enclosure IN FLOAT:
// per axis, a point outside the outer box lies outside the inner one on the same side, the two differences are rounded monotonically and
// the smaller of them is taken, squares and sums round monotonically.  A record's box encloses the boxes of its faces (min / max are
// exact), so B(record) <= B(aabb(f)) <= D(p, f) for every face under it: a skipped record holds no face with D < best, and the result is
// the minimum of D over ALL valid faces, bit for bit, whatever the order.  E alone does not have this property: its rounding error
// relative to d^2 grows without bound as d -> 0 (x is a rounded point of the triangle, p - x cancels), so a face in a skipped record could
// have E below B(record).  The clamp only ever raises E by E's own rounding error: in real arithmetic B(aabb(f)) <= d^2.
// Faces that are not valid (row behind the count, an index outside the vertices, n.n not finite or not above 0) go through knn_build's
// sentinel path (group -1: outside the grid's bounding box, sorted last), are gathered with face word -1, left out of every record and
// never taken.  No float atomic; the header's counts are integer atomics on words the first launch cleared.
#pragma clang fp contract(off)
namespace {

struct Tri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
};

__device__ __forceinline__ float mn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// the validity rule's third statement: n = ab x ac, n.n finite and above 0
__device__ __forceinline__ bool mn_has_area(const Tri t) {
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az, acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float nn = mn_dot(nx, ny, nz, nx, ny, nz);
    return nn > 0.0f && nn < __int_as_float(0x7f800000);
}

// E(p, f) and its closest point x (include/dqo_raster.h states the walk; Ericson, Real-Time Collision Detection, 5.1.5)
__device__ __forceinline__ float mn_closest(float px, float py, float pz, const Tri t, float& xx, float& xy, float& xz) {
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az, acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float d1 = mn_dot(abx, aby, abz, apx, apy, apz), d2 = mn_dot(acx, acy, acz, apx, apy, apz);
    const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const float d3 = mn_dot(abx, aby, abz, bpx, bpy, bpz), d4 = mn_dot(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    const float d5 = mn_dot(abx, aby, abz, cpx, cpy, cpz), d6 = mn_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e = d4 - d3, g = d5 - d6;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        xx = t.ax, xy = t.ay, xz = t.az;
    } else if (d3 >= 0.0f && d4 <= d3) {
        xx = t.bx, xy = t.by, xz = t.bz;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        xx = t.ax + v * abx, xy = t.ay + v * aby, xz = t.az + v * abz;
    } else if (d6 >= 0.0f && d5 <= d6) {
        xx = t.cx, xy = t.cy, xz = t.cz;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        xx = t.ax + w * acx, xy = t.ay + w * acy, xz = t.az + w * acz;
    } else if (va <= 0.0f && e >= 0.0f && g >= 0.0f) {
        const float w = e / (e + g);
        xx = t.bx + w * (t.cx - t.bx), xy = t.by + w * (t.cy - t.by), xz = t.bz + w * (t.cz - t.bz);
    } else {
        const float den = 1.0f / ((va + vb) + vc);
        const float v = vb * den, w = vc * den;
        xx = (t.ax + abx * v) + acx * w, xy = (t.ay + aby * v) + acy * w, xz = (t.az + abz * v) + acz * w;
    }
    const float rx = px - xx, ry = py - xy, rz = pz - xz;
    float E = mn_dot(rx, ry, rz, rx, ry, rz);
    if (!(E - E == 0.0f)) {  // not finite (0 / 0 in a sliver's edge branch): the face stands for its corner a
        E = mn_dot(apx, apy, apz, apx, apy, apz);
        xx = t.ax, xy = t.ay, xz = t.az;
    }
    return E;
}

// D(p, f) = fmaxf(E(p, f), B(p, aabb(f)))
__device__ __forceinline__ float mn_dist(const float4 me, const Tri t, float& xx, float& xy, float& xz) {
    const float E = mn_closest(me.x, me.y, me.z, t, xx, xy, xz);
    float bx[6];
    bx[0] = fminf(fminf(t.ax, t.bx), t.cx), bx[1] = fminf(fminf(t.ay, t.by), t.cy), bx[2] = fminf(fminf(t.az, t.bz), t.cz);
    bx[3] = fmaxf(fmaxf(t.ax, t.bx), t.cx), bx[4] = fmaxf(fmaxf(t.ay, t.by), t.cy), bx[5] = fmaxf(fmaxf(t.az, t.bz), t.cz);
    return fmaxf(E, dist_box_point(bx, me));
}

// face f's corners under the mesh transform, as every kernel here loads them; false: a row behind the count or a bad index
__device__ __forceinline__ bool mn_load(const float* __restrict__ vertices, const int32_t* __restrict__ faces, const float* __restrict__ xform,
                                        uint32_t f, uint32_t V, Tri& t) {
    int32_t a, b, c;
    if (!mo_face(faces, f, V, a, b, c)) return false;
    const float4 pa = nn1_point(vertices, xform, a), pb = nn1_point(vertices, xform, b), pc = nn1_point(vertices, xform, c);
    t.ax = pa.x, t.ay = pa.y, t.az = pa.z, t.bx = pb.x, t.by = pb.y, t.bz = pb.z, t.cx = pc.x, t.cy = pc.y, t.cz = pc.z;
    return true;
}

enum { MN_FACES = 0, MN_VALID = 1, MN_BAD_INDEX = 2, MN_DEGENERATE = 3, MN_QUERIES = 4 };

__global__ void mn_clear_kernel(int32_t* __restrict__ header) {
    if (threadIdx.x < 8) header[threadIdx.x] = 0;
}

// per face of the capacity: its centroid (the point knn_build sorts it by) and its group id, 0 = valid, -1 = not; the header's counts
__global__ __launch_bounds__(256) void mn_face_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                      const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t cap_f,
                                                      const float* __restrict__ xform, float* __restrict__ centroid, int32_t* __restrict__ grp,
                                                      int32_t* __restrict__ header) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    int kind = -1;  // -1: behind the count, else one of the header's words
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (f < F) {
        Tri t;
        if (!mn_load(vertices, faces, xform, f, V, t)) kind = MN_BAD_INDEX;
        else if (!mn_has_area(t)) kind = MN_DEGENERATE;
        else {
            kind = MN_VALID;
            cx = ((t.ax + t.bx) + t.cx) / 3.0f, cy = ((t.ay + t.by) + t.cy) / 3.0f, cz = ((t.az + t.bz) + t.cz) / 3.0f;
        }
    }
    if (f < cap_f) {
        centroid[3 * (size_t)f] = cx, centroid[3 * (size_t)f + 1] = cy, centroid[3 * (size_t)f + 2] = cz;
        grp[f] = kind == MN_VALID ? 0 : -1;
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long below = __ballot(kind >= 0), valid = __ballot(kind == MN_VALID), bad = __ballot(kind == MN_BAD_INDEX),
                             deg = __ballot(kind == MN_DEGENERATE);
    if (lane == 0 && below != 0ull) {
        atomicAdd(&header[MN_FACES], __popcll(below));
        if (valid != 0ull) atomicAdd(&header[MN_VALID], __popcll(valid));
        if (bad != 0ull) atomicAdd(&header[MN_BAD_INDEX], __popcll(bad));
        if (deg != 0ull) atomicAdd(&header[MN_DEGENERATE], __popcll(deg));
    }
}

// the faces in Morton order: three float4 per face; a face that is not valid (grp -1) becomes a far sentinel with face word -1
__global__ void mn_gather_kernel(uint32_t cap_f, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                 const int32_t* __restrict__ counts, uint32_t cap_v, const float* __restrict__ xform,
                                 const int32_t* __restrict__ grp, const uint64_t* __restrict__ keys, float4* __restrict__ tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap_f) return;
    const uint32_t src = (uint32_t)keys[i] & NN1_IDX_MASK;
    Tri t;
    const bool ok = grp[src] == 0 && mn_load(vertices, faces, xform, src, mo_count(counts, 0, cap_v), t);
    if (!ok) t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 1e18f;
    tris[3 * (size_t)i] = make_float4(t.ax, t.ay, t.az, __int_as_float(ok ? (int)src : -1));
    tris[3 * (size_t)i + 1] = make_float4(t.bx, t.by, t.bz, 0.f);
    tris[3 * (size_t)i + 2] = make_float4(t.cx, t.cy, t.cz, 0.f);
}

// the run (64 faces, one wave) and box (1024 faces, the block) records over the CORNERS of the valid faces; a record without one keeps
// {FLT_MAX, -FLT_MAX}: its box distance is +inf and nothing opens it.  Group words 0 (the scan is the unfiltered one).
__global__ __launch_bounds__(KNN_BOX) void mn_records_kernel(int F, const float4* __restrict__ tris, float* __restrict__ boxes,
                                                              float* __restrict__ sub) {
    __shared__ float s[6][KNN_BOX / KNN_SUB];
    const int i = blockIdx.x * KNN_BOX + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (i < F) {
        const float4 a = tris[3 * (size_t)i], b = tris[3 * (size_t)i + 1], c = tris[3 * (size_t)i + 2];
        if (__float_as_int(a.w) >= 0) {
            mn[0] = fminf(fminf(a.x, b.x), c.x), mn[1] = fminf(fminf(a.y, b.y), c.y), mn[2] = fminf(fminf(a.z, b.z), c.z);
            mx[0] = fmaxf(fmaxf(a.x, b.x), c.x), mx[1] = fmaxf(fmaxf(a.y, b.y), c.y), mx[2] = fmaxf(fmaxf(a.z, b.z), c.z);
        }
    }
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    const int run = blockIdx.x * (KNN_BOX / KNN_SUB) + wave;
    if (run * KNN_SUB < F && lane < 8)
        sub[8 * (size_t)run + lane] = lane == 0 ? mn[0] : lane == 1 ? mn[1] : lane == 2 ? mn[2] : lane == 3 ? mx[0] : lane == 4 ? mx[1]
                                                                                                                  : lane == 5 ? mx[2] : 0.f;
    if (lane == 0)
        for (int a = 0; a < 3; a++) s[a][wave] = mn[a], s[3 + a][wave] = mx[a];
    __syncthreads();
    if (threadIdx.x < 8) {
        float r = 0.f;
        if (threadIdx.x < 6) {
            r = s[threadIdx.x][0];
            for (int w = 1; w < KNN_BOX / KNN_SUB; w++) r = threadIdx.x < 3 ? fminf(r, s[threadIdx.x][w]) : fmaxf(r, s[threadIdx.x][w]);
        }
        boxes[8 * (size_t)blockIdx.x + threadIdx.x] = r;
    }
}

__device__ __forceinline__ Tri mn_tri(const float4* __restrict__ tris, int i, int& face) {
    const float4 a = tris[3 * (size_t)i], b = tris[3 * (size_t)i + 1], c = tris[3 * (size_t)i + 2];  // (wave-uniform address)
    face = __float_as_int(a.w);
    return Tri{a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
}

// D and a two-select take; a sentinel (face word -1) is never taken
__device__ __forceinline__ void mn_take(const float4 me, const float4* __restrict__ tris, int i, float& best, int& bface) {
    int face;
    const Tri t = mn_tri(tris, i, face);
    float xx, xy, xz;
    const float D = mn_dist(me, t, xx, xy, xz);
    const bool take = face >= 0 && D < best;
    best = take ? D : best, bface = take ? face : bface;
}

// nn1_scan_kernel<false>'s walk over the faces: one lane per sorted query, a record opened by the wave's ballot, a run's faces by
// wave-uniform loads, the faces around the query's rank first (a start bound), then the home box, then every group that cannot be excluded.
__global__ __launch_bounds__(256) void mn_scan_kernel(int Q, const float4* __restrict__ sorted_q, const uint64_t* __restrict__ keys_q, int F,
                                                      const float4* __restrict__ tris, const uint64_t* __restrict__ keys_f,
                                                      const float* __restrict__ boxes, const float* __restrict__ sub,
                                                      const float* __restrict__ groups, const float* __restrict__ vertices,
                                                      const int32_t* __restrict__ faces, const int32_t* __restrict__ counts, uint32_t cap_v,
                                                      const float* __restrict__ xform, float* __restrict__ dist2, int32_t* __restrict__ face_out,
                                                      float* __restrict__ closest, int32_t* __restrict__ header) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const float4 me = q < Q ? sorted_q[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t my_w = __float_as_uint(me.w);
    const bool live = q < Q && (my_w >> KNN_GROUP_SHIFT) != 0u;
    float best = FLT_MAX;
    int bface = -1, rank = 0;
    if (live) {
        const uint64_t key = (keys_q[q] >> FINE_IDX_BITS) << FINE_IDX_BITS;
        int lo = 0, hi = F;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys_f[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        rank = lo;
        for (int i = max(0, rank - 2); i <= min(F - 1, rank + 1); i++) mn_take(me, tris, i, best, bface);
    }
    const int nb = (F + KNN_BOX - 1) / KNN_BOX, ng = (nb + 63) / 64;
    auto wanted = [&](const float* rec) { return __ballot(live && !(dist_box_point(rec, me) > best)) != 0; };
    auto scan_box = [&](int b) {
        if (!wanted(boxes + 8 * (size_t)b)) return;
        const int lo = b * KNN_BOX, hi = min(F, lo + KNN_BOX);
        for (int r0 = lo; r0 < hi; r0 += KNN_SUB) {
            if (!wanted(sub + 8 * (size_t)(r0 / KNN_SUB))) continue;
            const int r1 = min(hi, r0 + KNN_SUB);
            for (int i = r0; i < r1; i++) mn_take(me, tris, i, best, bface);
        }
    };
    const unsigned long long lives = __ballot(live);
    if (lives != 0ull) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&header[MN_QUERIES], __popcll(lives));
        // queries that take no part sort last, so lane 0 of a wave with a live lane is live: the box its rank falls into first
        const int home = min(nb - 1, __builtin_amdgcn_readfirstlane(rank) / KNN_BOX);
        scan_box(home);
        for (int g = 0; g < ng; g++) {
            if (!wanted(groups + 8 * (size_t)g)) continue;
            const int b1 = min(nb, (g + 1) * 64);
            for (int b = g * 64; b < b1; b++)
                if (b != home) scan_box(b);
        }
    }
    if (q < Q) {
        const uint32_t dst = my_w & NN1_IDX_MASK;
        const bool found = live && bface >= 0;
        dist2[dst] = found ? best : FLT_MAX;
        if (face_out != nullptr) face_out[dst] = found ? bface : -1;
        if (closest != nullptr && found) {  // E's x for the returned face, once
            Tri t;
            mn_load(vertices, faces, xform, (uint32_t)bface, mo_count(counts, 0, cap_v), t);
            float xx, xy, xz;
            mn_closest(me.x, me.y, me.z, t, xx, xy, xz);
            closest[3 * (size_t)dst] = xx, closest[3 * (size_t)dst + 1] = xy, closest[3 * (size_t)dst + 2] = xz;
        }
    }
}

struct MnWs {
    KnnWs f, q;
    float* centroid;  // [cap_f][3]
    int32_t* grp;     // [cap_f] 0 = a valid face, -1 = not
    float4* tris;     // [cap_f][3] the faces in Morton order
    size_t total;
};
inline MnWs mn_ws(void* base, int Q, int cap_f) {
    MnWs w;
    DqoCarver k(base);
    w.f = knn_ws(k.take_raw(knn_ws(nullptr, cap_f).total), cap_f);
    w.q = knn_ws(k.take_raw(knn_ws(nullptr, Q).total), Q);
    w.centroid = k.take<float>(12 * (size_t)cap_f);
    w.grp = k.take<int32_t>(4 * (size_t)cap_f);
    w.tris = k.take<float4>(48 * (size_t)cap_f);
    w.total = k.total();
    return w;
}

}  // namespace

// Q and cap_faces carry dqo_nn1's index bits; cap_vertices is the mesh operand's
bool dqo_mesh_nearest_size_ok(int32_t Q, int32_t cap_v, int32_t cap_f) {
    return Q >= 1 && cap_f >= 1 && dqo_nn1_size_ok(Q) && dqo_nn1_size_ok(cap_f) && cap_v >= 1 && cap_v < MO_MAX;
}

size_t dqo_mesh_nearest_ws_bytes(int Q, int cap_v, int cap_f) {
    (void)cap_v;
    return mn_ws(nullptr, Q, cap_f).total;
}

int dqo_launch_mesh_nearest(int Q, const float* q_xyz, const uint8_t* q_keep, const float* q_xform, const float* vertices, const int32_t* faces,
                            const int32_t* counts, int cap_v, int cap_f, const float* mesh_xform, float* dist2, int32_t* face, float* closest,
                            int32_t* header, void* ws, hipStream_t s) {
    const MnWs w = mn_ws(ws, Q, cap_f);
    DQO_LAUNCH("mn_clear_kernel", mn_clear_kernel, dim3(1), dim3(64), s, header);
    DQO_LAUNCH("mn_face_kernel", mn_face_kernel, dim3((cap_f + 255) / 256), dim3(256), s, vertices, faces, counts, (uint32_t)cap_v,
               (uint32_t)cap_f, mesh_xform, w.centroid, w.grp, header);
    int rc = knn_build(cap_f, w.centroid, w.f, false, s, true, w.grp, false);  // (the keys only: mn_gather_kernel makes the sorted rows)
    if (rc) return rc;
    DQO_LAUNCH("mn_gather_kernel", mn_gather_kernel, dim3((cap_f + 255) / 256), dim3(256), s, (uint32_t)cap_f, vertices, faces, counts,
               (uint32_t)cap_v, mesh_xform, w.grp, w.f.keys, w.tris);
    const int nb = (cap_f + KNN_BOX - 1) / KNN_BOX, ng = (nb + 63) / 64;
    DQO_LAUNCH("mn_records_kernel", mn_records_kernel, dim3(nb), dim3(KNN_BOX), s, cap_f, w.tris, w.f.boxes, w.f.sub);
    DQO_LAUNCH("group_minmax_kernel", group_minmax_kernel, dim3((ng * 64 + 255) / 256), dim3(256), s, nb, w.f.boxes, w.f.groups);
    const DqoNn1Rows q_rows = {q_keep, nullptr};
    DQO_LAUNCH("nn1_query_keys_kernel", nn1_query_keys_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, q_xyz, q_rows, q_xform, w.f.bbox, w.q.keys);
    rc = knn_radix_sort(Q, w.q, true, s);
    if (rc) return rc;
    DQO_LAUNCH("nn1_gather_query_kernel", nn1_gather_query_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, q_xyz, q_rows, q_xform, w.q.keys,
               w.q.sorted);
    DQO_LAUNCH("mn_scan_kernel", mn_scan_kernel, dim3((Q + 255) / 256), dim3(256), s, Q, w.q.sorted, w.q.keys, cap_f, w.tris, w.f.keys, w.f.boxes,
               w.f.sub, w.f.groups, vertices, faces, counts, (uint32_t)cap_v, mesh_xform, dist2, face, closest, header);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_mesh_nearest_workspace_bytes(int32_t Q, int32_t cap_vertices, int32_t cap_faces) {
    return dqo_mesh_nearest_size_ok(Q, cap_vertices, cap_faces) ? dqo_mesh_nearest_ws_bytes(Q, cap_vertices, cap_faces) : 0;
}

DQO_API int dqo_mesh_nearest(int32_t Q, const float* query_xyz, const uint8_t* query_keep, const float* query_xform, const float* vertices,
                             const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces, const float* mesh_xform,
                             float* dist2, int32_t* face, float* closest, int32_t* header, void* workspace, size_t workspace_bytes,
                             void* hipStream) {
    DQO_CHECK_ARG(dqo_mesh_nearest_size_ok(Q, cap_vertices, cap_faces),
                  "bad size: %d queries, %d vertices, %d faces of capacity: queries and faces in [1, 2^25 - 1], vertices in [1, 2^28)", Q,
                  cap_vertices, cap_faces);
    DQO_CHECK_ARG(query_xyz && dist2, "null query / output");
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(header != counts, "header must not be the mesh's counts: the first launch clears it before the counts are read");
    DQO_CHECK_WS("mesh nearest", workspace, workspace_bytes, dqo_mesh_nearest_ws_bytes(Q, cap_vertices, cap_faces));
    return dqo_launch_mesh_nearest(Q, query_xyz, query_keep, query_xform, vertices, faces, counts, cap_vertices, cap_faces, mesh_xform, dist2,
                                   face, closest, header, workspace, (hipStream_t)hipStream);
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
    DQO_CHECK_WS("knn query", ws, ws_bytes, dqo_knn3_query_ws_bytes(Q, R));
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
    DQO_CHECK_ARG(R < (1 << FINE_IDX_BITS), "the grouped search carries the group id in the index word: at most 2^25 - 1 reference points");
    return knn3_query(Q, q_xyz, R, r_xyz, max_dist, dist2, idx3, ws, ws_bytes, stream, q_group, r_group, group_box);
}

DQO_API size_t dqo_knn3_workspace_bytes(int32_t P) { return dqo_knn3_ws_bytes(P < 0 ? 0 : P); }

DQO_API int dqo_knn3(int32_t P, const float* xyz, float* mean_d2, int32_t* idx3, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(xyz && mean_d2 && idx3, "null pointer");
    DQO_CHECK_WS("knn", ws, ws_bytes, dqo_knn3_ws_bytes(P));
    return dqo_launch_knn3(P, xyz, mean_d2, idx3, ws, ws_bytes, (hipStream_t)stream);
}

DQO_API size_t dqo_nn1_workspace_bytes(int32_t Q, int32_t R) { return dqo_nn1_size_ok(Q) && dqo_nn1_size_ok(R) ? dqo_nn1_ws_bytes(Q, R) : 0; }

// dqo_nn1 and dqo_nn1_grouped: one set of checks, one search; by_ids: the rows are given by group ids, which then must be there
static int nn1(bool by_ids, int32_t Q, const float* q_xyz, DqoNn1Rows q_rows, int32_t R, const float* r_xyz, DqoNn1Rows r_rows,
               const float* q_xform, const float* r_xform, float* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(dqo_nn1_size_ok(Q) && dqo_nn1_size_ok(R), "bad size: at most 2^25 - 1 rows per set");
    if (Q == 0) return DQO_OK;
    DQO_CHECK_ARG(q_xyz && dist2, "null query / output");
    DQO_CHECK_ARG(R == 0 || r_xyz, "null reference set");
    DQO_CHECK_ARG(!by_ids || (q_rows.ids && (R == 0 || r_rows.ids)), "null group ids");
    if (by_ids) DQO_CHECK_WS("nn1 grouped", ws, ws_bytes, dqo_nn1_ws_bytes(Q, R));
    else DQO_CHECK_WS("nn1", ws, ws_bytes, dqo_nn1_ws_bytes(Q, R));
    return dqo_launch_nn1(Q, q_xyz, q_rows, R, r_xyz, r_rows, q_xform, r_xform, dist2, idx, nullptr, ws, (hipStream_t)stream);
}

DQO_API int dqo_nn1(int32_t Q, const float* q_xyz, const uint8_t* q_keep, int32_t R, const float* r_xyz, const uint8_t* r_keep,
                    const float* q_xform, const float* r_xform, float* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    return nn1(false, Q, q_xyz, {q_keep, nullptr}, R, r_xyz, {r_keep, nullptr}, q_xform, r_xform, dist2, idx, ws, ws_bytes, stream);
}

DQO_API size_t dqo_nn1_grouped_workspace_bytes(int32_t Q, int32_t R) { return dqo_nn1_workspace_bytes(Q, R); }

DQO_API int dqo_nn1_grouped(int32_t Q, const float* q_xyz, const int32_t* q_group, int32_t R, const float* r_xyz, const int32_t* r_group,
                            const float* q_xform, const float* r_xform, float* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    return nn1(true, Q, q_xyz, {nullptr, q_group}, R, r_xyz, {nullptr, r_group}, q_xform, r_xform, dist2, idx, ws, ws_bytes, stream);
}

}  // extern "C"
