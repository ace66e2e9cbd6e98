// Tile binning for gfx950: which (Gaussian, tile) pairs become list entries, and where.  Replaces the per-Gaussian tile
// loops of
//   /root/reference/submodules/diff-gaussian-rasterizer-depth/cuda_rasterizer/forward.cu:344-353 (tiles_touched) and
//   cuda_rasterizer/rasterizer_impl.cu:70-115 (duplicateWithKeys) + the cub scan of :303,
// where one thread walks its Gaussian's whole tile rect: a wave then runs as long as its largest splat and every
// iteration waits for its own atomic.
//
// bin_count_kernel: a block owns 256 consecutive Gaussians, scans their rect areas in LDS and hands out ONE candidate
//   (Gaussian, tile) pair per thread-iteration (binary search in the scanned offsets), so lanes are evenly loaded.  Each
//   candidate takes the output-invariant footprint test of dqo_cull.h ONCE; the survivors are numbered per Gaussian (rect
//   order -> gaussian-major slot = slot_base + k: a fixed order, so the backward's per-Gaussian sum is reproducible) and
//   take their rank inside their tile from the tile histogram's atomic counter.  (tile, rank, Gaussian) goes into the
//   slot-indexed info table.
// tile_scan_kernel (rast_forward.hip) turns the histogram into the tiles' list ranges.
// bin_place_kernel: one thread per slot, no atomics, no decoding: position = range start + rank; writes the sort key and
//   the slot payload.
//
// Device-scope atomics execute memory-side on MI355X; the counters are spread one per 256 bytes (DQO_TSTRIDE) and every
// thread keeps up to four of them in flight.
#include "dqo_common.h"
#include "dqo_cull.h"
#include "dqo_k1_early.h"

namespace {

constexpr int BIN_THREADS = 256;
constexpr int BIN_CHUNK = BIN_THREADS;  // Gaussians per block, one per thread
constexpr int BIN_WINDOW = 16384;       // candidate pairs whose live bits fit the LDS bit array at once
constexpr int BIN_FLIGHT = 4;           // returning atomics in flight per thread
#ifndef BIN_WAVES
#define BIN_WAVES 8  // waves per SIMD the register allocation leaves room for (8: at most 64 VGPRs)
#endif

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// number of set bits of bits[] in the bit range [a, b)
__device__ __forceinline__ uint32_t popcount_range(const uint32_t* bits, uint32_t a, uint32_t b) {
    if (a >= b) return 0;
    uint32_t wa = a >> 5, wb = (b - 1) >> 5;
    const uint32_t ma = ~0u << (a & 31), mb = ~0u >> (31 - ((b - 1) & 31));
    if (wa == wb) return __popc(bits[wa] & ma & mb);
    uint32_t n = __popc(bits[wa] & ma) + __popc(bits[wb] & mb);
    for (uint32_t w = wa + 1; w < wb; w++) n += __popc(bits[w]);
    return n;
}

// block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = block sum.  Two barriers.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t lane, uint32_t wave, uint32_t* total) {
    // wave-level inclusive scan through DPP (four row_shr steps inside the 16-lane rows, then lane 15 / lane 31 broadcast into the rows
    // behind them): six vector instructions instead of six dependent trips through the LDS crossbar (__shfl_up), on the critical path
    // of every block, twice
    uint32_t incl = v;
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);  // row_shr:1 (lanes without a source add 0)
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);  // row_shr:2
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);  // row_shr:4
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);  // row_shr:8  -> inclusive within each row
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
    __syncthreads();  // s_wave free for reuse
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < BIN_THREADS / 64; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) wbase += t;
        tot += t;
    }
    *total = tot;
    return wbase + incl - v;
}

struct Cand {
    int gi, tile;
};

// The raw parameters of the Gaussians for bin_count_kernel<true> (the early part of the per-Gaussian forward at its head, dqo_k1_early.h)
struct DqoK1Raw {
    DqoView v;
    const float *means3D, *scales, *rotations, *opacities;
    const int32_t* gobj;
    int32_t *radii_out, *n_touched_out;
};

// tile_objects: DqoObjectGate.tile_objects or NULL — a candidate whose Gaussian's object (the spare word of its xy record) owns no pixel of
// the tile is dropped like one whose footprint cannot reach the tile
//
// K1: the block first runs the early part of the per-Gaussian forward for its own 256 Gaussians (k1_early: the statements of
// preprocess_kernel, which is then not launched) instead of reading their rect / conic / pixel position back from the tables — only for
// a frame whose tile histogram, flags and per-frame scalars the previous frame's dqo_rast_backward_adam has cleared
// (DqoRastCtx.frame_prezeroed: preprocess_kernel is also the launch that zeroes the histogram in front of this kernel's atomics).

template <bool K1>
__global__ __launch_bounds__(BIN_THREADS, BIN_WAVES) void bin_count_kernel(int P, int gx, const int32_t* __restrict__ tile_mask, DqoGeomLayout g,
                                                                uint32_t* __restrict__ tile_count, uint32_t* __restrict__ tile_flag,
                                                                DqoBinLayout bin, int64_t capacity,
                                                                const unsigned long long* __restrict__ tile_objects, const DqoK1Raw k1,
                                                                const uint8_t* __restrict__ row_flags) {
    constexpr bool PF = false;
#include "bin_count_body.inc"
}
// the parameter form (dqo_rast_*_params): bin_count_kernel<true> with k1.scales / rotations / opacities the raw parameters, activated on load
__global__ __launch_bounds__(BIN_THREADS, BIN_WAVES) void bin_count_pf_kernel(int P, int gx, const int32_t* __restrict__ tile_mask, DqoGeomLayout g,
                                                                   uint32_t* __restrict__ tile_count, uint32_t* __restrict__ tile_flag,
                                                                   DqoBinLayout bin, int64_t capacity,
                                                                   const unsigned long long* __restrict__ tile_objects, const DqoK1Raw k1,
                                                                   const uint8_t* __restrict__ row_flags) {
    constexpr bool K1 = true, PF = true;
#include "bin_count_body.inc"
}

// One thread per instance slot: list position = start of its tile's range + its rank there.
__global__ __launch_bounds__(256) void bin_place_kernel(DqoGeomLayout g, DqoImageLayout img, DqoBinLayout bin, int64_t capacity) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = min((int64_t)g.counters[0], capacity);
    if (slot >= n) return;
    const uint2 info = bin.slot_info[slot];
    const uint32_t gid = bin.slot_gid[slot];
    const uint2 range = img.ranges[info.x];
    const uint32_t pos = range.x + info.y;
    if (pos >= range.y) {  // only when the forward overflowed its capacity (ranges are emptied then)
        bin.rec_valid[slot] = 0u;
        return;
    }
    bin.recs[pos] = make_uint4(gid, __float_as_uint(g.xy_depth[gid].z), (uint32_t)slot, 0u);
    bin.rec_valid[slot] = 0u;  // no partial gradient record of this slot exists yet (backward)
}

}  // namespace

int dqo_launch_bin_count(int P, int gx, const int32_t* tile_mask, const DqoGeomLayout& g, const DqoImageLayout& img, const DqoBinLayout& bin,
                         int64_t capacity, const unsigned long long* tile_objects, hipStream_t s, const uint8_t* row_flags) {
    DqoK1Raw none{};
    DQO_LAUNCH("bin_count_kernel", bin_count_kernel<false>, dim3(dqo_spread_blocks(P)), dim3(BIN_THREADS), s, P, gx, tile_mask, g,
               img.tile_count, img.tile_flag, bin, capacity, tile_objects, none, row_flags);
    return DQO_OK;
}

// ... with the early part of the per-Gaussian forward at the head of every block (no preprocess_kernel launch in front); pf: `in` holds the
// parameter form's raw opacities / scales / rotations (bin_count_pf_kernel)
int dqo_launch_bin_count_k1(const DqoView& v, const DqoRastInputs* in, const DqoRastOutputs* out, const int32_t* gobj, const DqoGeomLayout& g,
                            const DqoImageLayout& img, const DqoBinLayout& bin, int64_t capacity, const unsigned long long* tile_objects,
                            hipStream_t s, bool pf) {
    DqoK1Raw k1;
    k1.v = v, k1.means3D = in->means3D, k1.scales = in->scales, k1.rotations = in->rotations, k1.opacities = in->opacities;
    k1.gobj = gobj, k1.radii_out = out->radii, k1.n_touched_out = out->n_touched;
    if (pf) {
        DQO_LAUNCH("bin_count_pf_kernel", bin_count_pf_kernel, dim3(dqo_spread_blocks(v.P)), dim3(BIN_THREADS), s, v.P, v.gx, in->tile_mask, g,
                   img.tile_count, img.tile_flag, bin, capacity, tile_objects, k1, v.row_flags);
    } else {
        DQO_LAUNCH("bin_count_kernel", bin_count_kernel<true>, dim3(dqo_spread_blocks(v.P)), dim3(BIN_THREADS), s, v.P, v.gx, in->tile_mask, g,
                   img.tile_count, img.tile_flag, bin, capacity, tile_objects, k1, v.row_flags);
    }
    return DQO_OK;
}

int dqo_launch_bin_place(const DqoGeomLayout& g, const DqoImageLayout& img, const DqoBinLayout& bin, int64_t capacity, hipStream_t s) {
    if (capacity <= 0) return DQO_OK;
    DQO_LAUNCH("bin_place_kernel", bin_place_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), s, g, img, bin, capacity);
    return DQO_OK;
}
