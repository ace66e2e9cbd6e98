// The k-th smallest of a launch's 32-bit keys by a radix select over three digits (11 + 11 + 10 bits), one launch per digit: every block
// counts the digit of its keys that lie in the bucket picked so far in an LDS histogram, adds its non-zero bins to a histogram in memory,
// and the block that takes the launch's last ticket picks the digit's bucket.  Users: map_sample.hip (two draws per launch) and
// map_densify.hip (one).  The caller owns the workspace head — where the histograms, the state words and the tickets lie is part of its
// public workspace size — and passes pointers; it also owns its LDS histogram (the sampler holds two, the densifier keeps one across a
// block's chunks).  map_tilemask.hip's select is another algorithm (8-bit digits, descending, inside one block) and no user.
//
// All blocks are 256 threads (four waves).
#pragma once
#include "dqo_common.h"

enum { DQO_SELECT_BINS = 2048 };

__device__ __forceinline__ uint32_t dqo_ld_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dqo_st_u32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The single-word ticket: one uint32 per kernel, zeroed by the call's first launch (a few hundred to two thousand blocks add to it — no
// need for dqo_reduce.h's 64 lines, and nothing to hand back at zero).  Every thread of every block calls it after the block's last store
// that the last block is to read; true (for every thread) in the block that took the launch's last ticket: it sees what every other
// block wrote before its own.  The barriers and fences are dqo_last_block's 1 and 3 (dqo_reduce.h says why each is needed).
__device__ __forceinline__ bool dqo_single_ticket_last_block(uint32_t* ticket) {
    __shared__ int s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    return true;
}

__device__ __forceinline__ uint32_t dqo_select_digit(uint32_t key, int level) {
    return level == 0 ? key >> 21 : level == 1 ? (key >> 10) & 2047u : key & 1023u;
}
// whether `key` lies in the bucket the levels above `level` picked (prefix: the digits picked so far)
__device__ __forceinline__ bool dqo_select_in_bucket(uint32_t key, uint32_t prefix, int level) {
    return level == 0 ? true : level == 1 ? (key >> 21) == prefix : (key >> 10) == prefix;
}

// one key of the bucket onto the block's LDS histogram s_hist[DQO_SELECT_BINS] (zeroed by the caller, a barrier before the first key)
__device__ __forceinline__ void dqo_select_count(uint32_t* s_hist, uint32_t key, int level) {
    atomicAdd(&s_hist[dqo_select_digit(key, level)], 1u);
}

// the block's LDS histogram onto the one in memory, its non-zero bins only (a barrier behind the block's last key comes first)
__device__ __forceinline__ void dqo_select_flush(const uint32_t* s_hist, uint32_t* hist) {
    for (int i = threadIdx.x; i < DQO_SELECT_BINS; i += 256) {
        const uint32_t v = s_hist[i];
        if (v != 0u) atomicAdd(&hist[i], v);
    }
}

// The last block picks the bucket of the k-th smallest key on this level from the level's histogram: with k = state[1] and the prefix
// state[0], state[0] gets the digit appended and state[1] the rank inside the bucket.  k == 0 leaves both as they are: (0, 0) is
// threshold 0 with nothing taken at it.  All 256 threads call it, eight bins each.
__device__ __forceinline__ void dqo_select_pick(const uint32_t* hist, uint32_t* state, int level) {
    __shared__ uint32_t s_part[256];
    const int tid = threadIdx.x;
    const uint32_t k = dqo_ld_u32(&state[1]), prefix = dqo_ld_u32(&state[0]);
    uint32_t h[8], sum = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) h[j] = dqo_ld_u32(&hist[tid * 8 + j]), sum += h[j];
    __syncthreads();  // (s_part may still be read by the previous call)
    s_part[tid] = sum;
    __syncthreads();
    uint32_t before = 0u;
    for (int t = 0; t < tid; t++) before += s_part[t];
    if (k >= 1u && before < k && k <= before + sum) {  // exactly one thread: the bins are counts of k or more keys in all
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (k <= before + h[j]) {
                dqo_st_u32(&state[0], (prefix << (level == 2 ? 10 : 11)) | (uint32_t)(tid * 8 + j));
                dqo_st_u32(&state[1], k - before);
                break;
            }
            before += h[j];
        }
    }
    __syncthreads();
}
