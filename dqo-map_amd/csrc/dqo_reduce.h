// A launch that ends with its own fixed-order reduction: every block stores a partial, every block takes an integer ticket, and the block
// that takes the launch's LAST ticket folds the partials in block-index order and writes the result.  One launch, no float atomics, the
// same bits on every run whatever order the blocks ran in, and the ticket words handed back at zero — no zero fill per call, so the entry
// can be captured in a hipGraph.  Users: map_eval.hip (eval_picture_kernel, eval_pcd_kernel, eval_pcd_grouped_kernel: its own partial lines), map_msssim.hip (msssim_level_kernel), map_lifecycle.hip (the two cloud limits and
// the frame's counts), map_tilemask.hip (window_masks_kernel: ticket only, its last block selects tiles), map_checkpoint.hip (map_pack_count_kernel: its last block scans
// the blocks' row counts), map_meshsample.hip (mesh_area_kernel: max and counts; mesh_quantise_kernel: its last block scans the blocks'
// quanta), dqo_adam.h (ticket only, unfenced).
//
// Deliberately NOT users, and not to be "finished" into this header:
//   - map_sample.hip's sp_last_block: one uint32 word per kernel, zeroed by the call's first launch, a few hundred blocks — a different
//     and simpler contract;
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
template <bool ORDERED = false>
__device__ __forceinline__ bool dqo_ticket_take(int32_t* ticket) {
    const int grid = (int)gridDim.x;
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
__device__ __forceinline__ bool dqo_last_block(int32_t* ticket, int* s_last) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();  // 1
        *s_last = dqo_ticket_take<true>(ticket);
    }
    __syncthreads();
    if (!*s_last) return false;
    __threadfence();  // 3
    return true;
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
