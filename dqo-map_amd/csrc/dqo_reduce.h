// A launch that ends with its own fixed-order reduction: every block stores a partial, every block takes an integer ticket, and the block
// that takes the launch's LAST ticket folds the partials in block-index order and writes the result.  One launch, no float atomics, the
// same bits on every run whatever order the blocks ran in, and the ticket words handed back at zero — no zero fill per call, so the entry
// can be captured in a hipGraph.  Users: map_eval.hip (eval_picture_kernel, eval_pcd_kernel, eval_pcd_grouped_kernel: its own partial lines), map_msssim.hip (msssim_level_kernel), map_lpips.hip (lpips_head_kernel), map_lifecycle.hip (the two cloud limits and
// the frame's counts), map_prune.hip (prune_rows_kernel: ticket and counts), map_tilemask.hip (window_masks_kernel: ticket only, its last block selects tiles), map_checkpoint.hip (map_pack_count_kernel: its last block scans
// the blocks' row counts), map_meshsample.hip (mesh_area_kernel: max and counts; mesh_quantise_kernel: its last block scans the blocks'
// quanta), map_tsdf.hip (tsdf_edges_kernel, tsdf_vertices_kernel: their last blocks scan the spans' vertex and face counts),
// map_meshops.hip (mesh_comp_stats / _fcount / _vcount_kernel, mesh_csr_scan_kernel, mesh_simp_number / _keep_kernel: span partials folded
// or scanned), map_meshcull.hip (mesh_cull_fcount / _vcount_kernel: span pairs scanned, tickets over the spans that have items), dqo_adam.h
// (ticket only, unfenced).
//
// Below the double reductions, the integer ends the map operators share (behind whichever last-block ticket their kernel takes):
//   - dqo_block_exclusive, the block-wide exclusive scan: map_densify.hip (the count and emit passes, the first histogram pass's N),
//     map_meshsample.hip (mesh_scan_kernel), and dqo_scan_block_counts;
//   - dqo_scan_block_counts, the last block's turn of the blocks' counts into exclusive offsets in index order: map_sample.hip
//     (sample_rank_kernel, sample_rows_kernel: two interleaved columns), map_densify.hip (densify_count_kernel: eight per thread),
//     map_checkpoint.hip (map_pack_count_kernel), map_meshsample.hip (mesh_quantise_kernel), map_tsdf.hip (tsdf_edges_kernel,
//     tsdf_vertices_kernel);
//   - dqo_line_count / dqo_line_totals, a row pass's counts on 64 lines: map_lifecycle.hip, map_prune.hip.
//
// Deliberately NOT users of the ticket, and not to be "finished" into this header:
//   - dqo_select.h's dqo_single_ticket_last_block (map_sample.hip, map_densify.hip): one uint32 word per kernel, zeroed by the call's
//     first launch, a few hundred to two thousand blocks — a different and simpler contract;
//   - the reductions that finish in a second launch (ICP, the tracker's p2p, SSIM, the loss, the attach loss): folding them into one launch
//     changes the launch count and the summation order, which is a performance change;
//   - everything under rast_*.
//
// All blocks are 256 threads (four waves).
#pragma once
#include "dqo_common.h"

// The ticket words (int32; zero when the workspace is made, zero again after every launch): word 0, and word 16 + 16 * line — one 64-byte
// line each.  Same-address returning atomics are served one at a time memory-side (~11 ns each, profiles/r06_tail_ticket.txt): a single
// word that all blocks of a 500 k-row launch add to is 43 us of queue.  So a block takes a ticket on line blockIdx % lines, and only the
// last block of a line one of word 0's.
enum {
    DQO_REDUCE_LINES = 64,
    DQO_REDUCE_HEAD_WORDS = 16 + 16 * DQO_REDUCE_LINES + 48,  // the ticket words, padded to a multiple of 256 bytes: a workspace's head
};
static_assert(DQO_TICKET_WORDS == 16 + 16 * DQO_REDUCE_LINES, "DqoAdamStep.block_ticket: include/dqo_raster.h and the kernels disagree");
static_assert(DQO_REDUCE_HEAD_WORDS * 4 == DQO_WINDOW_MASKS_SUMS_OFFSET, "the tile sums' place in the workspace is part of the public header");

// Takes the block's ticket (ONE thread of the block calls it); true in the block that took the launch's last one.  The words it used are
// zero again.  No barrier and, by default, no fence: it orders nothing but the tickets themselves.  ORDERED is dqo_last_block's (there).
// `grid`: the blocks that take a ticket — blocks 0 .. grid - 1 of the launch, every one of them exactly once (the launch's own gridDim.x in
// the forms without it; fewer where the blocks behind a device-side count leave at once: map_meshsample.hip's counted form, map_meshcull.hip).
template <bool ORDERED = false>
__device__ __forceinline__ bool dqo_ticket_take(int32_t* ticket, int grid) {
    const int lines = min((int)DQO_REDUCE_LINES, max(1, grid / 16));
    const int l = (int)blockIdx.x % lines;
    const int on_line = (grid - l + lines - 1) / lines;  // blocks b < grid with b % lines == l
    int32_t* const line = ticket + 16 + 16 * l;
    if (atomicAdd(line, 1) != on_line - 1) return false;
    *line = 0;
    if (ORDERED) __threadfence();  // fence 2 of dqo_last_block
    if (atomicAdd(ticket, 1) != lines - 1) return false;
    *ticket = 0;
    return true;
}
template <bool ORDERED = false>
__device__ __forceinline__ bool dqo_ticket_take(int32_t* ticket) {
    return dqo_ticket_take<ORDERED>(ticket, (int)gridDim.x);
}

// Every thread of every block calls it after the block's last store that the last block is to read; true (for every thread of the block)
// in the block that took the launch's last ticket, which may then read what EVERY block of the launch stored before its call.
// Why that holds (the tickets are relaxed atomics; the order comes from the barriers and three agent-scope fences):
//   1. barrier, then thread 0 fences BEFORE its ticket: the barrier puts the stores of all the block's threads before thread 0's fence,
//      the fence releases them to whoever reads a later value of the line's word.
//   2. the last block of a line has read the tickets of all the line's blocks, but a relaxed read acquires nothing and its own fence 1
//      came before that read.  So it fences AGAIN before it takes word 0's ticket: that fence acquires what the line's other blocks
//      released and releases it, with the block's own stores, to the block that takes word 0's last ticket.
//   3. in the last block only thread 0 has read a ticket.  The second barrier hands its answer to the block, and then EVERY thread fences
//      before it reads: a fence orders the accesses of the thread that executes it and of no other, so thread 0's alone would leave the
//      other threads' loads of the partials free to be served from before the last ticket was taken.
__device__ __forceinline__ bool dqo_last_block(int32_t* ticket, int* s_last, int grid) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();  // 1
        *s_last = dqo_ticket_take<true>(ticket, grid);
    }
    __syncthreads();
    if (!*s_last) return false;
    __threadfence();  // 3
    return true;
}
__device__ __forceinline__ bool dqo_last_block(int32_t* ticket, int* s_last) { return dqo_last_block(ticket, s_last, (int)gridDim.x); }

// Exclusive prefix of x over the block's threads in thread order, and the block's total (for every thread): __shfl_up over the wave, the
// four wave totals through LDS.  T: uint32_t or a 64-bit unsigned.  s_wave: 4 words of LDS; the call starts with a barrier, so the
// previous call's reads of them are done.
template <class T>
__device__ __forceinline__ T dqo_block_exclusive(T x, T& total, T* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    __syncthreads();  // (s_wave may still be read by the previous call)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    total = all;
    return before + incl - x;
}

// In the last block, by every thread: the blocks' counts a[0], a[stride], ... (n entries) become their exclusive prefix in index order,
// in place, and every thread gets the total.  A thread takes PER consecutive entries of a round of 256 * PER; the total so far is
// carried from round to round in a register.  Relaxed agent-scope loads and stores: dqo_last_block's fences (or the single-word ticket's,
// dqo_select.h) order the loads behind the other blocks' stores, the kernel boundary orders the next launch's reads behind the stores.
template <class T, int PER>
__device__ __forceinline__ T dqo_scan_block_counts(T* a, size_t n, int stride, T* s_wave) {
    T carry = 0;
    for (size_t base = 0; base < n; base += 256 * PER) {
        const size_t i0 = base + (size_t)threadIdx.x * PER;
        T h[PER], sum = 0, total;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            h[j] = i0 + j < n ? __hip_atomic_load(&a[(i0 + j) * stride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (T)0;
            sum += h[j];
        }
        T run = carry + dqo_block_exclusive(sum, total, s_wave);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if (i0 + j < n) __hip_atomic_store(&a[(i0 + j) * stride], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            run += h[j];
        }
        carry += total;
    }
    return carry;
}

// The counts of a row pass (map_lifecycle.hip, map_prune.hip): acc[DQO_COUNT_LINES][64] int32 behind the workspace's head, word k of a
// line is count k while the launch runs.  Same-address atomics are served one at a time memory-side (above), so a block counts on line
// blockIdx % DQO_COUNT_LINES: one integer atomic per wave and count, ballot + popcount.
enum { DQO_COUNT_LINES = 64 };
__device__ __forceinline__ void dqo_line_count(int32_t* acc, int k, bool pred, int lane) {
    const int n = __popcll(__ballot(pred));
    if (lane == 0 && n > 0) atomicAdd(&acc[(blockIdx.x % DQO_COUNT_LINES) * 64 + k], n);
}

// In the last block, by every thread: wave w adds up counts 2w and 2w + 1 over the lines (lane = line) into stats[k], for the k of
// `which` (a bit mask of the eight counts), and leaves their lines at zero.
__device__ __forceinline__ void dqo_line_totals(int32_t* acc, uint32_t which, int32_t* stats) {
    static_assert(DQO_COUNT_LINES == 64, "one lane per line");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 2 * wave; k < 2 * wave + 2; k++) {
        if (!((which >> k) & 1u)) continue;
        const uint32_t n = dqo_wave_sum_u32((uint32_t)atomicExch(&acc[lane * 64 + k], 0), lane);
        if (lane == 0) stats[k] = (int32_t)n;
    }
}

// The block's sums of every thread's a[0 .. NSUM): lanes by the xor butterfly, then the four waves in order; sum q goes to
// partial[blockIdx.x * STRIDE + q] (relaxed agent-scope stores: dqo_last_block, which the caller calls next, releases them).
// s_stage: 4 * STRIDE doubles of LDS at least, free again after dqo_last_block's first barrier.
template <int NSUM, int STRIDE>
__device__ __forceinline__ void dqo_block_partial(double (&a)[NSUM], double* s_stage, double* partial) {
    static_assert(NSUM <= STRIDE, "a partial line holds the sums");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < NSUM; q++) a[q] = dqo_wave_sum_f64(a[q], lane);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NSUM; q++) s_stage[wave * STRIDE + q] = a[q];
    }
    __syncthreads();
    if (tid < NSUM) {
        double t = 0.0;
        for (int v = 0; v < 4; v++) t += s_stage[v * STRIDE + tid];
        __hip_atomic_store(&partial[(size_t)blockIdx.x * STRIDE + tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// In the last block, by every thread: the partials of the blocks [first, last) added IN BLOCK-INDEX ORDER — staged through LDS STAGE
// blocks at a time (coalesced loads), sum q added by thread q, which gets the total (the other threads get 0).
// s_stage: STAGE * STRIDE doubles of LDS, free again on return.
template <int NSUM, int STRIDE, int STAGE>
__device__ __forceinline__ double dqo_fold_partials(const double* partial, int first, int last, double* s_stage) {
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int base = first; base < last; base += STAGE) {
        const int m = min(STAGE, last - base);
        for (int j = tid; j < m * STRIDE; j += 256)
            s_stage[j] = __hip_atomic_load(&partial[(size_t)base * STRIDE + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tid < NSUM)
            for (int k = 0; k < m; k++) total += s_stage[k * STRIDE + tid];
        __syncthreads();
    }
    return total;
}
