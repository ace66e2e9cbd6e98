// Geometry evaluation for gfx950, the ground truth's point set: trimesh.sample.sample_surface(mesh_gt, sample_nums) of eval_pcd
// (SLAM/eval.py:247) — face areas, their cumulative table, one draw located in the table per sample, two draws folded back into the
// triangle — on the device, from the mesh's vertex and face tensors.  include/dqo_raster.h (dqo_mesh_sample) states the contract.
//
// Two departures from trimesh, both so that the result is a pure function of the arguments: the draws are the seeded key rule of
// dqo_sample_hash.h (draws 4-7; 0-2 are dqo_growth_sample's, 3 is dqo_surfel_densify's) instead of numpy's stream, and the cumulative
// table holds INTEGER quanta of area instead of float sums, so it does not depend on the order the areas are added in.
//
// This file is compiled with -ffp-contract=off.  The statements, one rounding each, in this order (tests/mesh_oracle.py restates them):
//   area     a face with an index outside [0, V) has A = 0 and its vertices are never loaded.  Otherwise the nine floats become doubles,
//            e1 = b - a,  e2 = c - a
//            cx = e1y * e2z - e1z * e2y,  cy = e1z * e2x - e1x * e2z,  cz = e1x * e2y - e1y * e2x
//            A  = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);  a non-finite A becomes 0
//   quanta   amax = the largest A (a max: order-free);  frexp(amax) = (m, x), x = 0 for amax = 0;  e = 61 - bit_length(F) - x
//            q_f = (uint64) floor(ldexp(A_f, e)) < 2^(61 - bit_length(F)): the total stays below 2^61
//   table    cum[f] = q_0 + ... + q_f (uint64),  total = cum[F - 1];  total = 0 (no area): nothing is drawn, keep is all 0
//   draw     k_d = dqo_sample_key(seed_word, dqo_sample_draw_word(seed_word, 4 + d), i, 0xffffffff), d = 0..3, for sample i
//            t = floor(total * (k0 * 2^32 + k1) / 2^64) = __umul64hi(total, key64);  the face is the first f with cum[f] > t (a binary
//            search; a face without quanta is never picked)
//            u = k2 * 2^-32,  v = k3 * 2^-32 (double, exact);  if (u + v > 1.0)  u = 1.0 - u,  v = 1.0 - v
//            p = a + ((b - a) * u + (c - a) * v) per component in double, then rounded once to float
//
// Four launches of 256-thread blocks, a block owning MS_BLOCK = 1024 consecutive faces, thread t faces 4 t .. 4 t + 3 of them:
//   area      A_f into the table's slot f (as a double), the block's max and its two counts as partials; the block that takes the launch's
//             last ticket (dqo_reduce.h) folds the partials, forms e and writes header slots 1-4 and 7
//   quantise  q_f over A_f in place, the block's sum as a partial; the last block turns the sums, in block-index order, into exclusive
//             offsets in place (256 per round, a carried total) and writes the total and header slots 0, 5, 6
//   scan      the block's inclusive prefix of its q on top of its offset: cum, in place
//   sample    one thread per sample
// Integer atomics only (the tickets, which come back at zero: no zero fill per call); nothing is allocated, read back or synchronised.
//
// dqo_mesh_sample_counted is the same four launches on a mesh operand (dqo_mesh_components': capacities and a device pointer to the two
// counts, clamped to [0, capacity]): the kernels are templates on where V and F come from, the workspace and the grids are sized from
// cap_faces and count, a block behind F leaves at once (the tickets are counted over the blocks that have faces), and bit_length(F) is
// formed where e is — on the device.  Every output byte is dqo_mesh_sample's on the sliced mesh; F = 0 has no area (total = 0: keep all 0, nothing is searched).
#include "dqo_common.h"
#include "dqo_reduce.h"
#include "dqo_sample_hash.h"

namespace {

enum {
    MS_THREADS = 256,
    MS_FPT = 4,                       // faces per thread
    MS_BLOCK = MS_THREADS * MS_FPT,   // faces per block: DQO_MESH_SCAN_BLOCK
    MS_STATE_BYTES = 256,             // behind the ticket words: MsState
};
static_assert(MS_BLOCK == DQO_MESH_SCAN_BLOCK, "include/dqo_raster.h and the kernels disagree");

typedef unsigned long long u64;

struct MsState {
    u64 total;   // cum[F - 1]
    int32_t e;   // the quantum exponent
};

struct MsArgs {
    int V, F, count;
    uint32_t nblocks;
    uint32_t seed_word, draw_word[4];
    const float* vertices;
    const int32_t* faces;
    float* points;
    int32_t* face_index;
    uint8_t* keep;
    int32_t* header;
    int32_t* ticket;
    MsState* state;
    u64 *bmax, *bcount, *bsum;  // [nblocks] partials: the max area's bits, bad | degenerate << 32, the quanta (then the offsets)
    u64* cum;                   // [F] A_f as a double, then q_f, then cum[f]
    const int32_t* counts;      // dqo_mesh_sample_counted: the device counts (vertices, faces); V and F above are then the capacities
};

// The vertex (k = 0) or face (k = 1) count of the call.  COUNTED (dqo_mesh_sample_counted): the mesh operand's device word, clamped to
// [0, capacity] (NULL counts: the capacities); otherwise the host's argument, and the kernels are dqo_mesh_sample's own instructions.
template <bool COUNTED>
__device__ __forceinline__ int ms_count(const MsArgs& a, int k) {
    const int cap = k == 0 ? a.V : a.F;
    if (!COUNTED || a.counts == nullptr) return cap;
    const int32_t n = a.counts[k];
    return n <= 0 ? 0 : (n < cap ? n : cap);
}

// The blocks that have faces (one at least, which writes the header).  COUNTED: the grid is sized from the capacity; a block behind
// them leaves at once, takes no ticket and stores no partial — a mesh of half a million faces in buffers of twelve million would
// otherwise pay for 11 000 empty blocks' barriers, fences and tickets in each of three launches (0.62 ms against 0.15, profiles/mesh_eval.txt).
template <bool COUNTED>
__device__ __forceinline__ uint32_t ms_active_blocks(const MsArgs& a, int F) {
    if (!COUNTED) return a.nblocks;
    const uint32_t n = ((uint32_t)F + (uint32_t)MS_BLOCK - 1u) / (uint32_t)MS_BLOCK;
    return n > 0u ? n : 1u;
}

__device__ __forceinline__ u64 ms_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ms_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The block's sum / max of x over its threads, for every thread.  s_wave: 4 words of LDS, free again after the call's last barrier.
template <bool MAX>
__device__ __forceinline__ u64 ms_block_fold(u64 x, u64* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 y = __shfl_xor(x, d, 64);
        x = MAX ? (y > x ? y : x) : x + y;
    }
    __syncthreads();  // (s_wave may still be read by the previous call)
    if (lane == 0) s_wave[wave] = x;
    __syncthreads();
    u64 r = s_wave[0];
#pragma unroll
    for (int w = 1; w < 4; w++) r = MAX ? (s_wave[w] > r ? s_wave[w] : r) : r + s_wave[w];
    return r;
}

__device__ __forceinline__ bool ms_in_range(int32_t i, int V) { return (uint32_t)i < (uint32_t)V; }

__device__ __forceinline__ void ms_vertex(const float* vertices, int32_t i, double out[3]) {
    const float* p = vertices + 3 * (size_t)i;
    out[0] = (double)p[0], out[1] = (double)p[1], out[2] = (double)p[2];
}

// ---- area -------------------------------------------------------------------------------------------------------------------------------
template <bool COUNTED>
__global__ __launch_bounds__(MS_THREADS) void mesh_area_kernel(MsArgs a) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int V = ms_count<COUNTED>(a, 0), F = ms_count<COUNTED>(a, 1);
    const uint32_t nact = ms_active_blocks<COUNTED>(a, F);
    if (COUNTED && blockIdx.x >= nact) return;
    u64 amax = 0ull, bad = 0ull, degenerate = 0ull;
    const int64_t f0 = (int64_t)blockIdx.x * MS_BLOCK + (int64_t)tid * MS_FPT;
#pragma unroll
    for (int j = 0; j < MS_FPT; j++) {
        const int64_t f = f0 + j;
        if (f >= (int64_t)F) break;
        const int32_t ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
        double A = 0.0;
        if (!(ms_in_range(ia, V) && ms_in_range(ib, V) && ms_in_range(ic, V))) {
            bad++;
        } else {
            double pa[3], pb[3], pc[3];
            ms_vertex(a.vertices, ia, pa), ms_vertex(a.vertices, ib, pb), ms_vertex(a.vertices, ic, pc);
            const double e1x = pb[0] - pa[0], e1y = pb[1] - pa[1], e1z = pb[2] - pa[2];
            const double e2x = pc[0] - pa[0], e2y = pc[1] - pa[1], e2z = pc[2] - pa[2];
            const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
            A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
            if (!(A > 0.0 && A < __builtin_huge_val())) A = 0.0, degenerate++;  // (zero, infinite or NaN)
        }
        a.cum[f] = (u64)__double_as_longlong(A);
        const u64 bits = (u64)__double_as_longlong(A);  // (A >= 0: the bits order as the values do)
        amax = bits > amax ? bits : amax;
    }
    amax = ms_block_fold<true>(amax, s_wave);
    const u64 counts = ms_block_fold<false>(bad | (degenerate << 32), s_wave);  // (both below 2^25: no carry between the halves)
    if (tid == 0) ms_st(&a.bmax[blockIdx.x], amax), ms_st(&a.bcount[blockIdx.x], counts);
    if (!dqo_last_block(a.ticket, &s_last, COUNTED ? (int)nact : (int)gridDim.x)) return;
    u64 m = 0ull, c = 0ull;
    for (uint32_t b = (uint32_t)tid; b < nact; b += MS_THREADS) {
        const u64 x = ms_ld(&a.bmax[b]);
        m = x > m ? x : m, c += ms_ld(&a.bcount[b]);
    }
    m = ms_block_fold<true>(m, s_wave), c = ms_block_fold<false>(c, s_wave);
    if (tid == 0) {
        int x = 0;
        const double top = __longlong_as_double((long long)m);
        if (top > 0.0) (void)frexp(top, &x);
        const int e = 61 - (32 - __clz(F)) - x;  // (bit_length(0) = 0: __clz(0) is 32)
        a.state->e = e;
        a.header[1] = F, a.header[2] = (int32_t)(uint32_t)c, a.header[3] = (int32_t)(c >> 32), a.header[4] = e, a.header[7] = 0;
    }
}

// this thread's four table entries of the block (0 behind F)
__device__ __forceinline__ void ms_load4(const MsArgs& a, int F, int64_t f0, u64 x[MS_FPT]) {
#pragma unroll
    for (int j = 0; j < MS_FPT; j++) x[j] = f0 + j < (int64_t)F ? a.cum[f0 + j] : 0ull;
}

// ---- quantise ---------------------------------------------------------------------------------------------------------------------------
template <bool COUNTED>
__global__ __launch_bounds__(MS_THREADS) void mesh_quantise_kernel(MsArgs a) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int F = ms_count<COUNTED>(a, 1);
    const uint32_t nact = ms_active_blocks<COUNTED>(a, F);
    if (COUNTED && blockIdx.x >= nact) return;
    const int e = a.state->e;
    const int64_t f0 = (int64_t)blockIdx.x * MS_BLOCK + (int64_t)tid * MS_FPT;
    u64 x[MS_FPT], sum = 0ull;
    ms_load4(a, F, f0, x);
#pragma unroll
    for (int j = 0; j < MS_FPT; j++) {
        if (f0 + j >= (int64_t)F) break;
        const u64 q = (u64)floor(ldexp(__longlong_as_double((long long)x[j]), e));
        a.cum[f0 + j] = q, sum += q;
    }
    sum = ms_block_fold<false>(sum, s_wave);
    if (tid == 0) ms_st(&a.bsum[blockIdx.x], sum);
    if (!dqo_last_block(a.ticket, &s_last, COUNTED ? (int)nact : (int)gridDim.x)) return;
    // the last block: the blocks' sums -> exclusive offsets, in block-index order
    const u64 carry = dqo_scan_block_counts<u64, 1>(a.bsum, nact, 1, s_wave);
    if (tid == 0) {
        a.state->total = carry;
        a.header[0] = carry != 0ull ? a.count : 0;
        a.header[5] = (int32_t)(uint32_t)carry, a.header[6] = (int32_t)(uint32_t)(carry >> 32);
    }
}

// ---- scan -------------------------------------------------------------------------------------------------------------------------------
template <bool COUNTED>
__global__ __launch_bounds__(MS_THREADS) void mesh_scan_kernel(MsArgs a) {
    __shared__ u64 s_wave[4];
    const int tid = threadIdx.x;
    const int F = ms_count<COUNTED>(a, 1);
    if (COUNTED && blockIdx.x >= ms_active_blocks<COUNTED>(a, F)) return;  // (its offset was never written, and it has no face)
    const int64_t f0 = (int64_t)blockIdx.x * MS_BLOCK + (int64_t)tid * MS_FPT;
    u64 x[MS_FPT], total;
    ms_load4(a, F, f0, x);
    u64 run = a.bsum[blockIdx.x] + dqo_block_exclusive(((x[0] + x[1]) + x[2]) + x[3], total, s_wave);
#pragma unroll
    for (int j = 0; j < MS_FPT; j++) {
        if (f0 + j >= (int64_t)F) break;
        run += x[j];
        a.cum[f0 + j] = run;
    }
}

// ---- sample -----------------------------------------------------------------------------------------------------------------------------
template <bool COUNTED>
__global__ __launch_bounds__(MS_THREADS) void mesh_sample_kernel(MsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= (int64_t)a.count) return;
    const u64 total = a.state->total;
    if (total == 0ull) {  // no area (F = 0 among the reasons): no point, and no search of an empty table
        a.keep[i] = 0;
        return;
    }
    uint32_t k[4];
#pragma unroll
    for (int d = 0; d < 4; d++) k[d] = dqo_sample_key(a.seed_word, a.draw_word[d], (uint32_t)i, 0xffffffffu);
    const u64 t = __umul64hi(total, ((u64)k[0] << 32) | (u64)k[1]);  // < total = cum[F - 1]
    const int V = ms_count<COUNTED>(a, 0), F = ms_count<COUNTED>(a, 1);
    int lo = 0, hi = F - 1;
    while (lo < hi) {  // the first f with cum[f] > t
        const int mid = lo + ((hi - lo) >> 1);
        if (a.cum[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    const int32_t ia = a.faces[3 * (size_t)lo], ib = a.faces[3 * (size_t)lo + 1], ic = a.faces[3 * (size_t)lo + 2];
    if (!(ms_in_range(ia, V) && ms_in_range(ib, V) && ms_in_range(ic, V))) {  // (cannot happen: the face has quanta, so area)
        a.keep[i] = 0;
        return;
    }
    double pa[3], pb[3], pc[3];
    ms_vertex(a.vertices, ia, pa), ms_vertex(a.vertices, ib, pb), ms_vertex(a.vertices, ic, pc);
    double u = (double)k[2] * 0x1p-32, v = (double)k[3] * 0x1p-32;
    if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
#pragma unroll
    for (int d = 0; d < 3; d++) a.points[3 * i + d] = (float)(pa[d] + ((pb[d] - pa[d]) * u + (pc[d] - pa[d]) * v));
    if (a.face_index != nullptr) a.face_index[i] = lo;
    a.keep[i] = 1;
}

inline size_t ms_blocks(int64_t F) { return (size_t)((F + MS_BLOCK - 1) / MS_BLOCK); }
// the ticket words | MsState | bmax | bcount | bsum | cum (the last align_up(8 F, 256) bytes: dqo_eval.mesh_cum_view reads them for the tests).
// Of MsArgs it sets the workspace's pointers and nothing else.  F: the face capacity of the counted form
inline DqoLayout<MsArgs> ms_ws(void* base, int64_t F) {
    MsArgs w = {};
    DqoCarver k(base);
    w.ticket = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.state = k.take_raw<MsState>(MS_STATE_BYTES);
    w.bmax = k.take<u64>(ms_blocks(F) * sizeof(u64));
    w.bcount = k.take<u64>(ms_blocks(F) * sizeof(u64));
    w.bsum = k.take<u64>(ms_blocks(F) * sizeof(u64));
    w.cum = k.take<u64>((size_t)F * sizeof(u64));
    return {w, k.total()};
}

}  // namespace

static size_t dqo_mesh_sample_ws_bytes(int64_t F) { return ms_ws(nullptr, F).total; }

// COUNTED: V and F are the capacities — they size the workspace's parts and the grids — and `counts` holds the counts
template <bool COUNTED>
static int dqo_launch_mesh_sample(int V, const float* vertices, int F, const int32_t* faces, const int32_t* counts, int count, uint64_t seed,
                                  float* points, int32_t* face_index, uint8_t* keep, int32_t* header, void* ws, hipStream_t s) {
    MsArgs a = ms_ws(ws, F).w;
    a.V = V, a.F = F, a.count = count, a.nblocks = (uint32_t)ms_blocks(F), a.counts = counts;
    a.seed_word = dqo_sample_seed_word(seed);
    for (uint32_t d = 0; d < 4; d++) a.draw_word[d] = dqo_sample_draw_word(a.seed_word, 4u + d);
    a.vertices = vertices, a.faces = faces, a.points = points, a.face_index = face_index, a.keep = keep, a.header = header;
    const dim3 grid(a.nblocks), block(MS_THREADS);
    DQO_LAUNCH("mesh_area_kernel", mesh_area_kernel<COUNTED>, grid, block, s, a);
    DQO_LAUNCH("mesh_quantise_kernel", mesh_quantise_kernel<COUNTED>, grid, block, s, a);
    DQO_LAUNCH("mesh_scan_kernel", mesh_scan_kernel<COUNTED>, grid, block, s, a);
    DQO_LAUNCH("mesh_sample_kernel", mesh_sample_kernel<COUNTED>, dim3((unsigned)(((int64_t)count + MS_THREADS - 1) / MS_THREADS)), block, s, a);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// trimesh.sample.sample_surface on the ground-truth mesh (SLAM/eval.py:247).  The face table's and dqo_nn1's row limit
static bool mesh_size_ok(int32_t n) { return n >= 1 && n < (1 << 25); }

DQO_API size_t dqo_mesh_sample_workspace_bytes(int32_t F, int32_t count) {
    return mesh_size_ok(F) && mesh_size_ok(count) ? dqo_mesh_sample_ws_bytes(F) : 0;
}

DQO_API int dqo_mesh_sample(int32_t V, const float* vertices, int32_t F, const int32_t* faces, int32_t count, uint64_t seed, float* points,
                            int32_t* face_index, uint8_t* keep, int32_t* header, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(V >= 1, "bad vertex count %d", V);
    DQO_CHECK_ARG(mesh_size_ok(F), "bad face count %d: 1 to 2^25 - 1 faces", F);
    DQO_CHECK_ARG(mesh_size_ok(count), "bad sample count %d: 1 to 2^25 - 1 samples", count);
    DQO_CHECK_ARG(vertices && faces && points && keep && header, "null pointer");
    DQO_CHECK_WS("mesh sample", ws, ws_bytes, dqo_mesh_sample_ws_bytes(F));
    return dqo_launch_mesh_sample<false>(V, vertices, F, faces, nullptr, count, seed, points, face_index, keep, header, ws, (hipStream_t)stream);
}

// dqo_mesh_sample on a mesh operand (dqo_mesh_components'): the counts stay on the device
DQO_API size_t dqo_mesh_sample_counted_workspace_bytes(int32_t cap_faces, int32_t count) {
    return dqo_mesh_sample_workspace_bytes(cap_faces, count);
}

DQO_API int dqo_mesh_sample_counted(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                                    int32_t count, uint64_t seed, float* points, int32_t* face_index, uint8_t* keep, int32_t* header, void* ws,
                                    size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(cap_vertices >= 1 && cap_vertices < (1 << 28), "bad vertex capacity %d: at least 1 and below 2^28", cap_vertices);
    DQO_CHECK_ARG(mesh_size_ok(cap_faces), "bad face capacity %d: 1 to 2^25 - 1 faces", cap_faces);
    DQO_CHECK_ARG(mesh_size_ok(count), "bad sample count %d: 1 to 2^25 - 1 samples", count);
    DQO_CHECK_ARG(vertices && faces && points && keep && header, "null pointer");
    DQO_CHECK_ARG(header != counts, "header must not be the mesh's counts: every launch reads them, the first two write the header");
    DQO_CHECK_WS("mesh sample", ws, ws_bytes, dqo_mesh_sample_ws_bytes(cap_faces));
    return dqo_launch_mesh_sample<true>(cap_vertices, vertices, cap_faces, faces, counts, count, seed, points, face_index, keep, header, ws,
                                        (hipStream_t)stream);
}

}  // extern "C"
