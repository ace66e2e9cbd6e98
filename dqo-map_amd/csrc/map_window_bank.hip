// The keyframe bank of the mapping loop for gfx950: dqo_window_bank_arm / dqo_window_bank_select (include/dqo_raster.h states the rule).
//
// The reference's last call, global_optimization(is_end=True) (SLAM/slam.py:183, SLAM/multiprocess/mapper.py:1143-1148, 1196-1199), trains
// over all keyframes with a random keyframe per iteration.  A captured iteration reads everything per frame from device buffers, so the
// frame choice need not be a host decision: the select launch at the head of the iteration moves the scheduled keyframe from the bank into
// those buffers.  It replaces the eight device copies FusedMapper.set_frame issues from the host and the host's choice of a graph.
//
// The statements of one select launch, in order (tests/window_bank_oracle.py restates them):
//   1. every block: c = cursor, n, prev_k, prev_m, force          (plain loads: no block changes them before 5.)
//   2. c >= n or c >= args.n                 -> over = 1
//      else (k, m) = schedule[c]; k or m outside [0, K_cap) -> over = 2
//   3. over == 0: the camera group's parts from slot k iff force != 0 or k != prev_k, the mask group's parts from slot m iff force != 0
//      or m != prev_m.  A part is walked by ALL blocks of the launch, grid stride, in units of the widest access source and destination
//      both allow (16, 4 or 1 bytes); the bytes behind the last whole unit go one by one.
//   4. dqo_last_block: every block has read the state and finished its stores before the last block goes on.
//   5. the last block, one thread: over != 0 -> overrun = over, nothing else.  Otherwise: if c > 0 and the render header's overflow word
//      is set, lost[lost_count] = c - 1 and lost_count += 1; then prev_k = k, prev_m = m, force = 0, cursor = c + 1.
// Integer atomics on the ticket words only, no float arithmetic: the same bytes on every run.
//
// What bounds it: the bytes of a keyframe, read once and written once (1200 x 680 with a gate: 17.2 MB each way), over the grid of
// WB_BLOCKS blocks; a launch whose slots did not change reads seven words per block and takes its ticket.
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

#ifndef WB_BLOCKS
#define WB_BLOCKS 1024  // the grid's upper bound
#endif
#ifndef WB_PER
#define WB_PER 4  // units a thread has in flight
#endif
enum { WB_PARTS = 10, WB_CAMERA_PARTS = 8 };
static_assert(DQO_WINDOW_BANK_STATE_WORDS == DQO_REDUCE_HEAD_WORDS, "the bank's state is a last-block head: include/dqo_raster.h and dqo_reduce.h disagree");
static_assert(DQO_WINDOW_BANK_LOST_COUNT < DQO_WINDOW_BANK_STATE_WORDS, "the state words lie in the head's padding");

// one part of a slot: `bytes` at bank + slot * stride + offset go to dst (bank == nullptr: the part is not there)
struct WbPart {
    const char* bank;
    char* dst;
    size_t stride, offset, bytes;
};
struct WbLaunch {
    WbPart part[WB_PARTS];  // [0, WB_CAMERA_PARTS): the camera group (slot k); the rest: the mask group (slot m)
    int K_cap, n;
    const int32_t* schedule;
    int32_t* state;
    int32_t* lost;
    const DqoRastHeader* header;
};

// A state or schedule word: a plain load.  Earlier launches and copies wrote these words (the kernel boundary makes them visible) and this
// launch changes them in its last block only, behind every block's ticket, which a block takes after it has USED the values.  (Agent-scope
// atomic loads of the same few words by every wave of the launch are served one after the other: 16 us for a launch that copies nothing.)
__device__ __forceinline__ int32_t wb_load(const int32_t* p) { return *p; }

template <class T>
__device__ __forceinline__ void wb_copy_units(const char* __restrict__ src, char* __restrict__ dst, size_t bytes) {
    constexpr size_t CHUNK = 256 * WB_PER;  // units a block takes at a time: WB_PER per thread, 256 apart
    const size_t units = bytes / sizeof(T), step = (size_t)gridDim.x * CHUNK;
    const T* s = reinterpret_cast<const T*>(src);
    T* d = reinterpret_cast<T*>(dst);
    for (size_t u = (size_t)blockIdx.x * CHUNK + threadIdx.x; u < units; u += step) {
        if (u + (CHUNK - 256) < units) {  // all WB_PER loads in flight before the first store
            T v[WB_PER];
#pragma unroll
            for (int j = 0; j < WB_PER; j++) v[j] = s[u + 256 * j];
#pragma unroll
            for (int j = 0; j < WB_PER; j++) d[u + 256 * j] = v[j];
        } else {
            for (size_t w = u; w < units && w < u + CHUNK; w += 256) d[w] = s[w];
        }
    }
    // what is left behind the last whole unit (fewer than sizeof(T) bytes): block 0, one byte per thread
    const size_t done = units * sizeof(T);
    if (blockIdx.x == 0 && done + threadIdx.x < bytes) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

__global__ __launch_bounds__(256) void window_bank_arm_kernel(int32_t* __restrict__ state, int n) {
    for (int i = threadIdx.x; i < (int)DQO_WINDOW_BANK_STATE_WORDS; i += 256) {
        int32_t v = 0;
        if (i == DQO_WINDOW_BANK_N) v = n;
        if (i == DQO_WINDOW_BANK_PREV_K || i == DQO_WINDOW_BANK_PREV_M) v = -1;
        if (i == DQO_WINDOW_BANK_FORCE) v = 1;
        state[i] = v;
    }
}

__global__ __launch_bounds__(256) void window_bank_select_kernel(WbLaunch a) {
    __shared__ int s_last;
    const int c = wb_load(a.state + DQO_WINDOW_BANK_CURSOR), n = wb_load(a.state + DQO_WINDOW_BANK_N);
    const int prev_k = wb_load(a.state + DQO_WINDOW_BANK_PREV_K), prev_m = wb_load(a.state + DQO_WINDOW_BANK_PREV_M);
    const int force = wb_load(a.state + DQO_WINDOW_BANK_FORCE);
    int over = 0, k = -1, m = -1;
    if (c < 0 || c >= n || c >= a.n) {
        over = 1;
    } else {
        k = wb_load(a.schedule + 2 * (size_t)c), m = wb_load(a.schedule + 2 * (size_t)c + 1);
        if (k < 0 || k >= a.K_cap || m < 0 || m >= a.K_cap) over = 2;
    }
    if (over == 0) {
        const bool camera = force != 0 || k != prev_k, masks = force != 0 || m != prev_m;
#pragma unroll 1
        for (int i = 0; i < WB_PARTS; i++) {
            const WbPart& p = a.part[i];
            const bool cam_part = i < WB_CAMERA_PARTS;
            if (p.bank == nullptr || !(cam_part ? camera : masks)) continue;
            const char* src = p.bank + (size_t)(cam_part ? k : m) * p.stride + p.offset;
            const uintptr_t both = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(p.dst);
            if ((both & 15u) == 0) {
                wb_copy_units<uint4>(src, p.dst, p.bytes);
            } else if ((both & 3u) == 0) {
                wb_copy_units<uint32_t>(src, p.dst, p.bytes);
            } else {
                wb_copy_units<uint8_t>(src, p.dst, p.bytes);
            }
        }
    }
    if (!dqo_last_block(a.state, &s_last)) return;
    if (threadIdx.x != 0) return;
    if (over != 0) {
        a.state[DQO_WINDOW_BANK_OVERRUN] = over;
        return;
    }
    if (c > 0 && a.header != nullptr && __hip_atomic_load(&a.header->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        const int lc = a.state[DQO_WINDOW_BANK_LOST_COUNT];
        if (lc >= 0 && lc < a.n) {  // (at most one entry per position: the list cannot outgrow the schedule)
            a.lost[lc] = c - 1;
            a.state[DQO_WINDOW_BANK_LOST_COUNT] = lc + 1;
        }
    }
    a.state[DQO_WINDOW_BANK_PREV_K] = k;
    a.state[DQO_WINDOW_BANK_PREV_M] = m;
    a.state[DQO_WINDOW_BANK_FORCE] = 0;
    a.state[DQO_WINDOW_BANK_CURSOR] = c + 1;
}

}  // namespace

// ---- entry points (include/dqo_raster.h): argument validation, the call ----
extern "C" {

DQO_API int dqo_window_bank_arm(int32_t* state, int32_t n, void* stream) {
    DQO_CHECK_ARG(state != nullptr, "null state");
    DQO_CHECK_ARG(n >= 0, "bad schedule length %d", n);
    DQO_LAUNCH("window_bank_arm_kernel", window_bank_arm_kernel, dim3(1), dim3(256), (hipStream_t)stream, state, (int)n);
    return DQO_OK;
}

DQO_API int dqo_window_bank_select(const DqoWindowBank* b, void* stream) {
    DQO_CHECK_ARG(b != nullptr, "null arguments");
    DQO_CHECK_ARG(b->K_cap >= 1, "bad K_cap %d", b->K_cap);
    DQO_CHECK_ARG(b->W > 0 && b->H > 0 && (int64_t)b->W * b->H < (1ll << 31) / 3, "bad image size");
    DQO_CHECK_ARG(b->n >= 0, "bad schedule length %d", b->n);
    DQO_CHECK_ARG(b->camera && b->gt_color && b->gt_depth && b->render_mask && b->tile_mask, "null bank part");
    DQO_CHECK_ARG(b->dst_bg && b->dst_viewmatrix && b->dst_projmatrix && b->dst_campos && b->dst_gt_color && b->dst_gt_depth &&
                      b->dst_render_mask && b->dst_tile_mask,
                  "null destination");
    DQO_CHECK_ARG(b->schedule && b->state && b->lost, "null schedule / state / lost");
    const bool gate = b->pixel_object != nullptr;
    DQO_CHECK_ARG((b->tile_objects != nullptr) == gate && (b->dst_pixel_object != nullptr) == gate && (b->dst_tile_objects != nullptr) == gate,
                  "the gate parts (pixel_object, tile_objects) go together, in the bank and in the destination");
    const size_t HW = (size_t)b->W * b->H, T = (size_t)((b->W + DQO_TILE - 1) / DQO_TILE) * ((b->H + DQO_TILE - 1) / DQO_TILE);
    WbLaunch a;
    const char* cam = reinterpret_cast<const char*>(b->camera);
    auto part = [](const void* bank, void* dst, size_t stride, size_t offset, size_t bytes) {
        return WbPart{reinterpret_cast<const char*>(bank), reinterpret_cast<char*>(dst), stride, offset, bytes};
    };
    a.part[0] = part(cam, b->dst_bg, 160, 0, 12);
    a.part[1] = part(cam, b->dst_viewmatrix, 160, 12, 64);
    a.part[2] = part(cam, b->dst_projmatrix, 160, 76, 64);
    a.part[3] = part(cam, b->dst_campos, 160, 140, 12);
    a.part[4] = part(b->gt_color, b->dst_gt_color, 12 * HW, 0, 12 * HW);
    a.part[5] = part(b->gt_depth, b->dst_gt_depth, 4 * HW, 0, 4 * HW);
    a.part[6] = part(b->pixel_object, b->dst_pixel_object, 4 * HW, 0, 4 * HW);
    a.part[7] = part(b->tile_objects, b->dst_tile_objects, 8 * T, 0, 8 * T);
    a.part[8] = part(b->render_mask, b->dst_render_mask, HW, 0, HW);
    a.part[9] = part(b->tile_mask, b->dst_tile_mask, 4 * T, 0, 4 * T);
    a.K_cap = b->K_cap, a.n = b->n;
    a.schedule = b->schedule, a.state = b->state, a.lost = b->lost, a.header = b->render_header;
    // the grid follows the image size alone: one block per chunk of the colour target (256 * WB_PER units of 16 bytes), [16, WB_BLOCKS]
    const size_t chunk = (size_t)4096 * WB_PER;
    const int grid = (int)std::min<size_t>((size_t)WB_BLOCKS, std::max<size_t>(16, (12 * HW + chunk - 1) / chunk));
    DQO_LAUNCH("window_bank_select_kernel", window_bank_select_kernel, dim3(grid), dim3(256), (hipStream_t)stream, a);
    return DQO_OK;
}

}  // extern "C"
