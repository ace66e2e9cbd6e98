// Map checkpoints for gfx950: the map's structure-of-arrays buffers (spare rows, a per-row cloud flag) to and from the array-of-structures
// vertex table of the reference's PLY files (SLAM/gaussian_pointcloud.py:641-684 save_model_ply, :132-207 load) — an ordered compaction
// plus a transpose, on the device.
//
//   dqo_launch_map_pack     the alive rows with stable == 0 in ascending row index, then the alive rows with stable != 0 in ascending row
//                           index: the row order of the reference's MERGED file (merge_ply, SLAM/utils.py:414-423), so one table is all
//                           three files — its first U rows are path.ply, its last S rows path_stable.ply, the whole path_merge.ply.
//   dqo_launch_map_unpack   the inverse for load: n table rows into rows [first_row, first_row + n) of the buffers.
//
// Columns of a row (dqo_ply.attribute_names): x y z | nx ny nz (zeros, :645) | f_dc_0..2 | f_rest channel-major (shs[:, 1:, :] transposed
// from [K,3] to [3,K]) | opacity | scale_0..2 | rot_0..3 | [confidence]: C = 6 + 3 M + 8 (+ 1).
//
// Pure data movement: every value travels as a uint32, so NaN payloads, -0 and denormals keep their bits.  No float atomics; the only
// integer atomics are the tickets of dqo_reduce.h; the result is a pure function of the inputs.
//
// Pack is two launches.
//   count  one block per 256 rows reads the two flag bytes of a row and stores the block's (u, s) pair; the block that takes the launch's
//          last ticket turns the pairs, in block-index order, into exclusive offsets IN PLACE (256 pairs per round, a carried total) and
//          writes the header {U, S}.  The ticket words come back at zero: no zero fill per call.
//   pack   one block per 64 rows (a quarter of a count block — PK_ROWS rows of C <= 207 floats are at most 53 KiB of LDS, 16 KiB at SH degree 3, so
//          eight blocks, the wave limit, stay resident on a CU's 160 KiB).  The block re-reads the 256 flag pairs of its count block
//          (ballots: its own rows' masks and the popcounts of the quarters before it), loads its rows from every buffer with coalesced
//          loads into an LDS tile at their column positions (row stride C | 1, odd: a row-strided access is conflict-free) and stores
//          the live rows as two contiguous runs of floats, the unstable run and the stable run.  A quarter without a live row loads
//          nothing.  Rows leave and arrive as 4-byte words: a run starts at any multiple of 4 bytes, so wider stores would need a peeled
//          head and tail per run.
// Unpack is one launch: the same trip through LDS in the other direction.
//
// Indices are 64-bit inside the kernels; the entry points nevertheless refuse a table of more than 2^31 - 1 floats (include/dqo_raster.h).
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

enum {
    PK_ROWS = 64,  // rows of a pack / unpack block: one wave's flags
};

typedef unsigned long long u64;

struct PkArgs {
    int P, M, C, Cp, with_conf;
    const uint32_t *xyz, *shs, *opacity, *scaling, *rotation, *confidence;
    const uint8_t *alive, *stable;
    uint32_t* table;
    u64* pairs;  // [count blocks] u | s << 32: the block's counts, then (after the count launch) the counts of the blocks before it
    int32_t* header;
};

struct UnpkArgs {
    int M, Cin, Cp, has_conf;
    int64_t n, first_row;
    const uint32_t* table;
    uint32_t *xyz, *shs, *opacity, *scaling, *rotation, *confidence;
};

__host__ __device__ inline size_t pk_blocks(int64_t P) { return (size_t)((P + 255) / 256); }

// which cloud's file a row goes to: 0 none, 1 unstable, 2 stable
__device__ __forceinline__ int pk_class(const PkArgs& a, int64_t i) {
    if (i >= (int64_t)a.P) return 0;
    if (a.alive != nullptr && a.alive[i] == 0) return 0;
    return (a.stable != nullptr && a.stable[i] != 0) ? 2 : 1;
}

// the table column of float `rem` (= 3 k + channel) of a row's SH block [M,3]
__device__ __forceinline__ int pk_sh_column(int rem, int K) {
    const int k = rem / 3, ch = rem - 3 * k;
    return k == 0 ? 6 + ch : 9 + ch * K + (k - 1);
}

// ---- count ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_pack_count_kernel(PkArgs a, int32_t* ticket) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cls = pk_class(a, (int64_t)blockIdx.x * 256 + tid);
    const u64 mu = __ballot(cls == 1), ms = __ballot(cls == 2);
    if (lane == 0) s_wave[wave] = (u64)__popcll(mu) | ((u64)__popcll(ms) << 32);
    __syncthreads();
    if (tid == 0)  // (relaxed agent-scope store: dqo_last_block, next, releases it)
        __hip_atomic_store(&a.pairs[blockIdx.x], ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(ticket, &s_last)) return;
    // the last block: pairs -> exclusive offsets, in block-index order.  Both halves of a pair stay below 2^31 (P does), so one 64-bit add
    // adds the two counts without a carry between them.
    const u64 carry = dqo_scan_block_counts<u64, 1>(a.pairs, gridDim.x, 1, s_wave);
    if (tid == 0) a.header[0] = (int32_t)(uint32_t)carry, a.header[1] = (int32_t)(carry >> 32);
}

// ---- pack -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_pack_rows_kernel(PkArgs a) {
    extern __shared__ uint32_t s_tile[];  // [PK_ROWS][Cp]
    __shared__ u64 s_mask[8];             // the count block's four unstable masks, then its four stable masks
    __shared__ uint8_t s_list[PK_ROWS];   // the tile rows that leave: the unstable ones in order, then the stable ones
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cb = (int)(blockIdx.x >> 2), sub = (int)(blockIdx.x & 3);
    const int cls = pk_class(a, (int64_t)cb * 256 + tid);
    const u64 bu = __ballot(cls == 1), bs = __ballot(cls == 2);
    if (lane == 0) s_mask[wave] = bu, s_mask[4 + wave] = bs;
    __syncthreads();
    const u64 mu = s_mask[sub], ms = s_mask[4 + sub];
    if ((mu | ms) == 0ull) return;  // (the whole block: no live row in this quarter)
    const int nU = __popcll(mu), nS = __popcll(ms);
    int preU = 0, preS = 0;
    for (int v = 0; v < sub; v++) preU += __popcll(s_mask[v]), preS += __popcll(s_mask[4 + v]);
    if (tid < PK_ROWS) {
        const u64 bit = 1ull << tid;
        if (mu & bit) s_list[__popcll(mu & (bit - 1))] = (uint8_t)tid;
        else if (ms & bit) s_list[nU + __popcll(ms & (bit - 1))] = (uint8_t)tid;
    }
    const int C = a.C, Cp = a.Cp, K = a.M - 1, M3 = 3 * a.M;
    const int64_t row0 = (int64_t)cb * 256 + sub * PK_ROWS;
    const int rows = (int)min((int64_t)PK_ROWS, (int64_t)a.P - row0);  // (>= 1: the quarter has a live row)
    if (tid < rows * 3) {
        const int r = tid / 3, c = tid - 3 * r;
        s_tile[r * Cp + c] = a.xyz[row0 * 3 + tid];
        s_tile[r * Cp + 3 + c] = 0u;  // the normals
        s_tile[r * Cp + 10 + 3 * K + c] = a.scaling[row0 * 3 + tid];
    }
    if (tid < rows * 4) s_tile[(tid >> 2) * Cp + 13 + 3 * K + (tid & 3)] = a.rotation[row0 * 4 + tid];
    if (tid < rows) {
        s_tile[tid * Cp + 9 + 3 * K] = a.opacity[row0 + tid];
        if (a.with_conf) s_tile[tid * Cp + C - 1] = a.confidence != nullptr ? a.confidence[row0 + tid] : 0u;
    }
    {  // the SH block: rows * 3 M consecutive floats; (r, rem) = divmod(j, 3 M) carried from step to step
        const uint32_t* src = a.shs + row0 * M3;
        const int n = rows * M3, dr = 256 / M3, drem = 256 - dr * M3;
        int r = tid / M3, rem = tid - r * M3;
        for (int j = tid; j < n; j += 256) {
            s_tile[r * Cp + pk_sh_column(rem, K)] = src[j];
            r += dr, rem += drem;
            if (rem >= M3) rem -= M3, r++;
        }
    }
    __syncthreads();
    // the two runs
    const u64 off = a.pairs[cb];
    uint32_t* outU = a.table + ((size_t)(uint32_t)off + (size_t)preU) * C;
    uint32_t* outS = a.table + ((size_t)(uint32_t)a.header[0] + (size_t)(off >> 32) + (size_t)preS) * C;
    const int nUC = nU * C, total = (nU + nS) * C, dk = 256 / C, dc = 256 - dk * C;
    int k = tid / C, c = tid - k * C;
    for (int q = tid; q < total; q += 256) {
        const uint32_t v = s_tile[(int)s_list[k] * Cp + c];
        if (q < nUC) outU[q] = v;
        else outS[q - nUC] = v;
        k += dk, c += dc;
        if (c >= C) c -= C, k++;
    }
}

// ---- unpack -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_unpack_rows_kernel(UnpkArgs a) {
    extern __shared__ uint32_t s_tile[];  // [PK_ROWS][Cp]
    const int tid = threadIdx.x;
    const int Cin = a.Cin, Cp = a.Cp, K = a.M - 1, M3 = 3 * a.M;
    const int64_t row0 = (int64_t)blockIdx.x * PK_ROWS;
    const int rows = (int)min((int64_t)PK_ROWS, a.n - row0);
    {
        const uint32_t* src = a.table + row0 * Cin;
        const int n = rows * Cin, dk = 256 / Cin, dc = 256 - dk * Cin;
        int k = tid / Cin, c = tid - k * Cin;
        for (int q = tid; q < n; q += 256) {
            s_tile[k * Cp + c] = src[q];
            k += dk, c += dc;
            if (c >= Cin) c -= Cin, k++;
        }
    }
    __syncthreads();
    const int64_t R0 = a.first_row + row0;
    if (tid < rows * 3) {
        const int r = tid / 3, c = tid - 3 * r;
        a.xyz[R0 * 3 + tid] = s_tile[r * Cp + c];
        a.scaling[R0 * 3 + tid] = s_tile[r * Cp + 10 + 3 * K + c];
    }
    if (tid < rows * 4) a.rotation[R0 * 4 + tid] = s_tile[(tid >> 2) * Cp + 13 + 3 * K + (tid & 3)];
    if (tid < rows) {
        a.opacity[R0 + tid] = s_tile[tid * Cp + 9 + 3 * K];
        if (a.confidence != nullptr) a.confidence[R0 + tid] = a.has_conf ? s_tile[tid * Cp + Cin - 1] : 0u;
    }
    uint32_t* dst = a.shs + R0 * M3;
    const int n = rows * M3, dr = 256 / M3, drem = 256 - dr * M3;
    int r = tid / M3, rem = tid - r * M3;
    for (int j = tid; j < n; j += 256) {
        dst[j] = s_tile[r * Cp + pk_sh_column(rem, K)];
        r += dr, rem += drem;
        if (rem >= M3) rem -= M3, r++;
    }
}

// ---- pack by object: every file of save_model_ply_obj (SLAM/gaussian_pointcloud.py:589-637) in one table ---------------------------------
// The alive rows that have an object, ordered by (stable != 0, object id, row index): 128 classes (cloud, object), class q = 64 cloud +
// object.  header[q] is the class's row count, so the rows of (cloud c, object g) are the slice that starts at the sum of the counts before
// class 64 c + g.  Three launches, no atomics at all, nothing but the table and the header written:
//   count  one block per class walks the map's flag and id columns and stores its class's count (a plain store: nothing to zero);
//   order  one block per class, its start = the counts before it; each of its 16 waves takes a sixteenth of the rows, counts its hits,
//          and then walks them again with ballots — the hits' row indices go, in ascending row order, into WORD 0 OF THE TABLE ROWS THE
//          CLASS WILL FILL: the order list needs no memory of its own, and rows behind the total are not touched;
//   pack   one block per 64 table rows reads their source indices, then a wave gathers a row's C words column by column (the stores are
//          contiguous, the SH loads stay inside the row's 12 M bytes) — word-for-word copies, as map_pack_rows_kernel's.
// 128 blocks each read all P flags and ids (6 bytes a row, from L2 after the first): 2 x 1.5 GB at 2 M rows, a fraction of the copy of
// the table to the host that follows.
enum {
    PKO_CLASSES = 128,
    PKO_WAVES = 16,  // waves of a count / order block
};

__device__ __forceinline__ int pko_class(const PkArgs& a, const int32_t* __restrict__ object, int64_t i) {
    const int cls = pk_class(a, i);
    if (cls == 0) return -1;
    const int g = object[i];
    return g >= 0 && g < 64 ? (cls - 1) * 64 + g : -1;
}

__global__ __launch_bounds__(64 * PKO_WAVES) void map_pack_object_count_kernel(PkArgs a, const int32_t* __restrict__ object) {
    __shared__ int s_n[PKO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mine = (int)blockIdx.x;
    int n = 0;
    for (int64_t i = tid; i < (int64_t)a.P; i += 64 * PKO_WAVES) n += pko_class(a, object, i) == mine ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) s_n[wave] = n;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < PKO_WAVES; w++) t += s_n[w];
        a.header[mine] = t;
    }
}

__global__ __launch_bounds__(64 * PKO_WAVES) void map_pack_object_order_kernel(PkArgs a, const int32_t* __restrict__ object) {
    __shared__ int s_n[PKO_WAVES];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mine = (int)blockIdx.x;
    if (a.header[mine] == 0) return;  // (the whole block)
    if (wave == 0) {  // the rows of the classes before this one
        int v = (lane < mine ? a.header[lane] : 0) + (lane + 64 < mine ? a.header[lane + 64] : 0);
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_base = v;
    }
    const int64_t seg = (((int64_t)a.P + PKO_WAVES - 1) / PKO_WAVES + 63) / 64 * 64;  // rows of a wave: a multiple of 64
    const int64_t lo = seg * wave, hi = min((int64_t)a.P, lo + seg);
    int n = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) n += pko_class(a, object, i) == mine ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) s_n[wave] = n;
    __syncthreads();
    int64_t run = s_base;
    for (int w = 0; w < wave; w++) run += s_n[w];
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool hit = i < hi && pko_class(a, object, i) == mine;
        const u64 m = __ballot(hit);
        if (hit) a.table[(size_t)(run + __popcll(m & ((1ull << lane) - 1ull))) * a.C] = (uint32_t)i;
        run += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void map_pack_object_rows_kernel(PkArgs a) {
    __shared__ int s_part[4];
    __shared__ uint32_t s_src[PK_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        int v = tid < PKO_CLASSES ? a.header[tid] : 0;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_part[wave] = v;
    }
    __syncthreads();
    const int64_t total = (int64_t)s_part[0] + s_part[1], k0 = (int64_t)blockIdx.x * PK_ROWS;
    if (k0 >= total) return;
    const int n = (int)min((int64_t)PK_ROWS, total - k0), C = a.C, K = a.M - 1, M3 = 3 * a.M;
    if (tid < n) s_src[tid] = a.table[(size_t)(k0 + tid) * C];
    __syncthreads();
    for (int r = wave; r < n; r += 4) {
        const size_t src = s_src[r];
        uint32_t* out = a.table + (size_t)(k0 + r) * C;
        for (int c = lane; c < C; c += 64) {
            uint32_t v;
            if (c < 3) v = a.xyz[src * 3 + c];
            else if (c < 6) v = 0u;  // the normals
            else if (c < 9) v = a.shs[src * M3 + (c - 6)];
            else if (c < 9 + 3 * K) {
                const int q = c - 9, ch = q / K, k = q - ch * K + 1;
                v = a.shs[src * M3 + 3 * k + ch];
            } else if (c == 9 + 3 * K) v = a.opacity[src];
            else if (c < 13 + 3 * K) v = a.scaling[src * 3 + (c - 10 - 3 * K)];
            else if (c < 17 + 3 * K) v = a.rotation[src * 4 + (c - 13 - 3 * K)];
            else v = a.confidence != nullptr ? a.confidence[src] : 0u;
            out[c] = v;
        }
    }
}

inline const uint32_t* pk_u32(const float* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* pk_u32(float* p) { return reinterpret_cast<uint32_t*>(p); }

}  // namespace

static size_t dqo_map_pack_ws_bytes(int64_t P) { return DQO_REDUCE_HEAD_WORDS * 4 + dqo_align_up(pk_blocks(P) * sizeof(u64), 256); }

static int dqo_launch_map_pack(int P, int M, int with_conf, const float* xyz, const float* shs, const float* opacity_raw, const float* scaling_raw,
                               const float* rotation_raw, const float* confidence, const uint8_t* alive, const uint8_t* stable, float* table,
                               int32_t* header, void* ws, hipStream_t s) {
    PkArgs a;
    a.P = P, a.M = M, a.C = 6 + 3 * M + 8 + (with_conf ? 1 : 0), a.Cp = a.C | 1, a.with_conf = with_conf ? 1 : 0;
    a.xyz = pk_u32(xyz), a.shs = pk_u32(shs), a.opacity = pk_u32(opacity_raw), a.scaling = pk_u32(scaling_raw);
    a.rotation = pk_u32(rotation_raw), a.confidence = pk_u32(confidence);
    a.alive = alive, a.stable = stable, a.table = pk_u32(table);
    a.pairs = (u64*)((char*)ws + DQO_REDUCE_HEAD_WORDS * 4), a.header = header;
    const unsigned nb = (unsigned)pk_blocks(P);
    DQO_LAUNCH("map_pack_count_kernel", map_pack_count_kernel, dim3(nb), dim3(256), s, a, (int32_t*)ws);
    const unsigned tiles = (unsigned)(((int64_t)P + PK_ROWS - 1) / PK_ROWS);
    // (a count block's four quarters: blocks 4 cb .. 4 cb + 3; the last count block may have fewer)
    DQO_LAUNCH_SMEM("map_pack_rows_kernel", map_pack_rows_kernel, dim3(tiles), dim3(256), (size_t)PK_ROWS * a.Cp * 4, s, a);
    return DQO_OK;
}

static int dqo_launch_map_pack_by_object(int P, int M, int with_conf, const float* xyz, const float* shs, const float* opacity_raw,
                                         const float* scaling_raw, const float* rotation_raw, const float* confidence, const uint8_t* alive,
                                         const uint8_t* stable, const int32_t* object, float* table, int32_t* header, hipStream_t s) {
    PkArgs a;
    a.P = P, a.M = M, a.C = 6 + 3 * M + 8 + (with_conf ? 1 : 0), a.Cp = a.C | 1, a.with_conf = with_conf ? 1 : 0;
    a.xyz = pk_u32(xyz), a.shs = pk_u32(shs), a.opacity = pk_u32(opacity_raw), a.scaling = pk_u32(scaling_raw);
    a.rotation = pk_u32(rotation_raw), a.confidence = pk_u32(confidence);
    a.alive = alive, a.stable = stable, a.table = pk_u32(table);
    a.pairs = nullptr, a.header = header;
    DQO_LAUNCH("map_pack_object_count_kernel", map_pack_object_count_kernel, dim3(PKO_CLASSES), dim3(64 * PKO_WAVES), s, a, object);
    DQO_LAUNCH("map_pack_object_order_kernel", map_pack_object_order_kernel, dim3(PKO_CLASSES), dim3(64 * PKO_WAVES), s, a, object);
    DQO_LAUNCH("map_pack_object_rows_kernel", map_pack_object_rows_kernel, dim3((unsigned)(((int64_t)P + PK_ROWS - 1) / PK_ROWS)), dim3(256), s, a);
    return DQO_OK;
}

static int dqo_launch_map_unpack(int M, int64_t n, int64_t first_row, int has_conf, const float* table, float* xyz, float* shs, float* opacity_raw,
                                 float* scaling_raw, float* rotation_raw, float* confidence, hipStream_t s) {
    UnpkArgs a;
    a.M = M, a.Cin = 6 + 3 * M + 8 + (has_conf ? 1 : 0), a.Cp = a.Cin | 1, a.has_conf = has_conf ? 1 : 0;
    a.n = n, a.first_row = first_row, a.table = pk_u32(table);
    a.xyz = pk_u32(xyz), a.shs = pk_u32(shs), a.opacity = pk_u32(opacity_raw), a.scaling = pk_u32(scaling_raw);
    a.rotation = pk_u32(rotation_raw), a.confidence = pk_u32(confidence);
    DQO_LAUNCH_SMEM("map_unpack_rows_kernel", map_unpack_rows_kernel, dim3((unsigned)((n + PK_ROWS - 1) / PK_ROWS)), dim3(256),
                    (size_t)PK_ROWS * a.Cp * 4, s, a);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// the vertex table of a map checkpoint: at most 2^31 - 1 floats, SH sizes up to 64 coefficients (a tile of 64 rows stays below 64 KiB of LDS)
static bool map_table_size_ok(int64_t rows, int32_t M, int32_t with_conf) {
    return rows >= 1 && M >= 1 && M <= 64 && rows * (int64_t)(6 + 3 * M + 8 + (with_conf ? 1 : 0)) <= (int64_t)0x7fffffff;
}

DQO_API size_t dqo_map_pack_workspace_bytes(int32_t P) { return P >= 1 ? dqo_map_pack_ws_bytes(P) : 0; }

DQO_API int dqo_map_pack_rows(int32_t P, int32_t M, int32_t include_confidence, const float* xyz, const float* shs, const float* opacity_raw,
                              const float* scaling_raw, const float* rotation_raw, const float* confidence, const uint8_t* alive,
                              const uint8_t* stable, float* table, int64_t table_rows, int32_t* header, void* ws, size_t ws_bytes,
                              void* stream) {
    DQO_CHECK_ARG(P >= 1, "bad row count %d", P);
    DQO_CHECK_ARG(M >= 1 && M <= 64, "bad SH size M = %d: 1 to 64 coefficients", M);
    DQO_CHECK_ARG(map_table_size_ok(P, M, include_confidence), "bad size: a table of %d rows exceeds 2^31 - 1 floats", P);
    DQO_CHECK_ARG(xyz && shs && opacity_raw && scaling_raw && rotation_raw && table && header, "null pointer");
    DQO_CHECK_ARG(table_rows >= (int64_t)P, "table capacity %lld rows is below the map's %d rows", (long long)table_rows, P);
    DQO_CHECK_WS("map pack", ws, ws_bytes, dqo_map_pack_ws_bytes(P));
    return dqo_launch_map_pack(P, M, include_confidence != 0, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence, alive, stable, table,
                               header, ws, (hipStream_t)stream);
}

// save_model_ply_obj (SLAM/gaussian_pointcloud.py:589-637; mapper.py:1586-1588): the vertex tables of every per-object file
DQO_API int dqo_map_pack_rows_by_object(int32_t P, int32_t M, int32_t include_confidence, const float* xyz, const float* shs,
                                        const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, const float* confidence,
                                        const uint8_t* alive, const uint8_t* stable, const int32_t* gaussian_object, float* table,
                                        int64_t table_rows, int32_t* header, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(P >= 1, "bad row count %d", P);
    DQO_CHECK_ARG(M >= 1 && M <= 64, "bad SH size M = %d: 1 to 64 coefficients", M);
    DQO_CHECK_ARG(map_table_size_ok(P, M, include_confidence), "bad size: a table of %d rows exceeds 2^31 - 1 floats", P);
    DQO_CHECK_ARG(xyz && shs && opacity_raw && scaling_raw && rotation_raw && table && header, "null pointer");
    DQO_CHECK_ARG(gaussian_object, "null object ids");
    DQO_CHECK_ARG(table_rows >= (int64_t)P, "table capacity %lld rows is below the map's %d rows", (long long)table_rows, P);
    DQO_CHECK_WS("map pack", ws, ws_bytes, dqo_map_pack_ws_bytes(P));
    return dqo_launch_map_pack_by_object(P, M, include_confidence != 0, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence, alive, stable,
                                         gaussian_object, table, header, (hipStream_t)stream);
}

DQO_API int dqo_map_unpack_rows(int32_t P, int32_t M, int32_t n, int32_t first_row, int32_t has_confidence, const float* table, float* xyz,
                                float* shs, float* opacity_raw, float* scaling_raw, float* rotation_raw, float* confidence, void* stream) {
    DQO_CHECK_ARG(P >= 1 && n >= 0 && first_row >= 0 && (int64_t)first_row + n <= (int64_t)P, "bad size: rows [%d, %d + %d) of a map of %d rows",
                  first_row, first_row, n, P);
    DQO_CHECK_ARG(M >= 1 && M <= 64, "bad SH size M = %d: 1 to 64 coefficients", M);
    DQO_CHECK_ARG(map_table_size_ok(P, M, 1), "bad size: a table of %d rows exceeds 2^31 - 1 floats", P);
    if (n == 0) return DQO_OK;
    DQO_CHECK_ARG(table && xyz && shs && opacity_raw && scaling_raw && rotation_raw, "null pointer");
    return dqo_launch_map_unpack(M, n, first_row, has_confidence != 0, table, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence,
                                 (hipStream_t)stream);
}

}  // extern "C"
