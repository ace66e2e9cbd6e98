// The two-level integer ticket by which the LAST block of a launch learns that it is the last (map_eval.hip, map_tilemask.hip): what
// the other blocks wrote before their tickets it may then read, so a launch ends with a fixed-order reduction and needs no second one.
#pragma once
#include "dqo_common.h"

enum {
    EV_LINES = 64,                           // ticket lines: word 0, and word 16 + 16 * line
    EV_HEAD_WORDS = 16 + 16 * EV_LINES + 48,  // padded to a multiple of 256 bytes
};
static_assert(EV_HEAD_WORDS * 4 % 256 == 0, "workspace head layout");

// Takes the block's ticket; true (for every thread of the block) in the block that took the last one, which then sees what every other
// block wrote before its ticket.  The words it used are zero again.
__device__ __forceinline__ bool ev_last_block(int32_t* ticket, int* s_last) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const int grid = (int)gridDim.x;
        const int lines = min((int)EV_LINES, max(1, grid / 16));
        const int l = (int)blockIdx.x % lines;
        const int on_line = (grid - l + lines - 1) / lines;  // blocks b < grid with b % lines == l
        int32_t* const line = ticket + 16 + 16 * l;
        bool last = atomicAdd(line, 1) == on_line - 1;
        if (last) {
            *line = 0;
            __threadfence();  // (acquire what the line's other blocks released, release it to the block that takes word 0's last ticket)
            last = atomicAdd(ticket, 1) == lines - 1;
            if (last) *ticket = 0;
        }
        *s_last = last;
    }
    __syncthreads();
    if (!*s_last) return false;
    __threadfence();
    return true;
}
