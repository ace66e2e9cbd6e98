// Floater pruning for gfx950: Mapping.to_purne with create_virtual_cameras (SLAM/multiprocess/mapper.py:424-529) on ONE map whose rows
// carry a `stable` flag and a `frame_id` (GaussianPointCloud._frame_ids, SLAM/gaussian_pointcloud.py:52, 230-231, 277-279, 435;
// mapper.py:1451-1460).  The keyframe's camera is turned by +-theta about two axes around the point it looks at, the whole map is rendered
// from the four virtual cameras, and every Gaussian added since the previous keyframe that none of the four views touched leaves the map.
// The reference does it with three host round trips (.cpu() of the centre depth, numpy camera math, .item() of the mask sum) and a
// boolean-mask re-allocation of both clouds; here nothing is read back and every row is rewritten in place.
//
// prune_cameras_kernel (dqo_prune_cameras) — one launch, one lane, double, one rounding per statement, none contracted
// (tests/prune_oracle.py restates them in this order; cos_t / sin_t are the HOST's doubles, so the kernel holds adds and multiplies only):
//     Rw, T        with W2V[a][b] = viewmatrix[b][a] (the raster settings keep the transposed w2c): Rw = W2V[:3,:3], T = W2V[:3,3] — the
//                  reference's camera_R = frame.R.transpose(0, 1) and camera_T = frame.T (:478-479)
//     d            d0 = depth[pixel]; d = (d0 == 0) ? -1 : -d0 (:473-477)
//     focal        z = Rw[:,2]; focal = T + d * z; offset = T - focal — not simplified (:480, 448)
//     R_k, T_k     k = 0..3 with A_k = Ry(+theta), Ry(-theta), Rx(+theta), Rx(-theta) and rotation_matrix's signs (:431-443; Ry = [[c,0,s],
//                  [0,1,0],[-s,0,c]], Rx = [[1,0,0],[0,c,-s],[0,s,c]], the minus angle negates s): R_k = A_k @ Rw, T_k = A_k @ offset + focal
//                  (:452-463), every entry of a product (a0 b0 + a1 b1) + a2 b2
//     viewmatrix_k frame.update(R_k, T_k) (scene/cameras.py:169-183) takes R_k for the camera's R, i.e. W2V_k = [[R_k^T, T_k], [0,0,0,1]]:
//                  viewmatrix_k[:3,:3] = float(R_k) as it stands, viewmatrix_k[3,:3] = float(T_k), the last column (0,0,0,1)
//     projmatrix_k float(viewmatrix_k (double, before its rounding) @ double(projection)), entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 rounded once
//                  (cameras.py:179-183 forms it in float32 from the rounded viewmatrix: the departure map_traj.hip documents)
//     focal        float(focal), for inspection
// campos is not formed: Camera.update never refreshes camera_center, so the reference renders the virtual views with the real camera's
// centre; the caller passes the frame's own campos (it feeds colour only and cannot change a touch count).
// The reference's quirks, ported literally:
//   - `cx, cy = int(frame.cy), int(frame.cx)` then `depth_map[cy, cx]` (:471, 473) reads row int(frame.cx), column int(frame.cy): the
//     caller forms the pixel index, the kernel reads depth[pixel];
//   - camera_T is the w2c translation, used as if it were a position (:478, 480);
//   - update() is handed a w2c rotation where it expects the transposed one (:479, 497).
// The reference restores the frame with the transposed R afterwards (:529); nothing here mutates the caller's camera.
//
// prune_touch_kernel (dqo_prune_touch) — one launch per virtual camera, directly behind its render; one thread per row:
// touched[i] = 1 where n_touched[i] != 0 (`n_touched += render_output["n_touched"]`, :508).  A render that outgrew its capacity
// (DqoRastHeader.overflow != 0) leaves n_touched at zero for EVERY row: such a launch marks nothing and counts an invalid render instead,
// or the frame would delete every Gaussian of the window.
//
// prune_rows_kernel (dqo_prune_rows) — one launch, one thread per row: a row with alive != 0 && lo < frame_id <= hi is in the window
// (:510-515); if every render was valid, a window row with touched == 0 is deleted (:519-527): what map_lifecycle.hip writes into a freed
// row (dqo_map_free_row, dqo_common.h), and frame_id = 0.  Every touched word is cleared as it is read and the last block clears the render counts: the workspace goes back
// ready for the next call.  The counts are integer atomics per wave on 64 lines that the block with the last ticket adds up (dqo_reduce.h).
//
// A row that map_lifecycle.hip frees keeps a stale frame_id (DqoLifecycle does not know the column): no kernel reads frame_id while
// alive == 0, and the growth step that moves a Gaussian into the row overwrites it.
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

// ---- dqo_prune_cameras ----------------------------------------------------------------------------------------------------------

__global__ void prune_cameras_kernel(const float* __restrict__ viewmatrix, const float* __restrict__ projection, const float* __restrict__ depth,
                                     int64_t pixel, double cos_t, double sin_t, float* __restrict__ out_view, float* __restrict__ out_proj,
                                     float* __restrict__ out_focal) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double Rw[9], T[3], Q[16];
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) Rw[3 * a + b] = (double)viewmatrix[4 * b + a];
        T[a] = (double)viewmatrix[12 + a];
    }
    for (int k = 0; k < 16; k++) Q[k] = (double)projection[k];
    const double d0 = (double)depth[pixel];
    const double d = (d0 == 0.0) ? -1.0 : -d0;
    double focal[3], offset[3];
    for (int a = 0; a < 3; a++) {
        const double z = Rw[3 * a + 2];
        focal[a] = T[a] + d * z;
        offset[a] = T[a] - focal[a];
    }
    for (int a = 0; a < 3; a++) out_focal[a] = (float)focal[a];
    const double c = cos_t;
    for (int k = 0; k < 4; k++) {
        const double s = (k & 1) ? -sin_t : sin_t;
        double A[9];
        if (k < 2) {  // rotation_matrix('y', .)
            A[0] = c, A[1] = 0.0, A[2] = s;
            A[3] = 0.0, A[4] = 1.0, A[5] = 0.0;
            A[6] = -s, A[7] = 0.0, A[8] = c;
        } else {  // rotation_matrix('x', .)
            A[0] = 1.0, A[1] = 0.0, A[2] = 0.0;
            A[3] = 0.0, A[4] = c, A[5] = -s;
            A[6] = 0.0, A[7] = s, A[8] = c;
        }
        double V[16];  // the virtual camera's world_view_transform, still in double
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) V[4 * i + j] = (A[3 * i] * Rw[j] + A[3 * i + 1] * Rw[3 + j]) + A[3 * i + 2] * Rw[6 + j];
            V[12 + i] = ((A[3 * i] * offset[0] + A[3 * i + 1] * offset[1]) + A[3 * i + 2] * offset[2]) + focal[i];
            V[4 * i + 3] = 0.0;
        }
        V[15] = 1.0;
        for (int e = 0; e < 16; e++) out_view[16 * k + e] = (float)V[e];
        for (int r = 0; r < 4; r++)
            for (int q = 0; q < 4; q++)
                out_proj[16 * k + 4 * r + q] =
                    (float)(((V[4 * r] * Q[q] + V[4 * r + 1] * Q[4 + q]) + V[4 * r + 2] * Q[8 + q]) + V[4 * r + 3] * Q[12 + q]);
    }
}

// ---- dqo_prune_touch / dqo_prune_rows ---------------------------------------------------------------------------------------------

// words of the workspace's head (int32; zero when the workspace is made, handed back at zero by dqo_prune_rows): the ticket words of
// dqo_reduce.h, the two render counts in free words of word 0's line, and the call's counts spread over DQO_COUNT_LINES lines of 256 bytes
// (same-address atomics are served one at a time memory-side: map_lifecycle.hip measured it)
enum {
    PR_INVALID = 2,  // renders that overflowed their capacity since the last dqo_prune_rows
    PR_VALID = 3,    // renders that marked rows
    PR_ACC = DQO_REDUCE_HEAD_WORDS,  // [DQO_COUNT_LINES][64] word k of a line: count k of the call (stats gets the sums)
    PR_HEAD_WORDS = PR_ACC + DQO_COUNT_LINES * 64,
};
static_assert(PR_VALID < 16 && PR_HEAD_WORDS * 4 % 256 == 0, "workspace head layout");

struct PruneRows {
    int32_t P;
    float* xyz;
    float* opacity_raw;
    float* scaling_raw;
    float* confidence;
    uint8_t* alive;
    uint8_t* row_flags;
    uint8_t* stable;
    int32_t* add_tick;
    int32_t* depth_error_counter;
    int32_t* color_error_counter;
    int32_t* frame_id;
    const float* park;
    int32_t lo, hi;
    int32_t* head;
    uint32_t* touched;
    int32_t* stats;
};

__host__ __device__ inline size_t pr_blocks(int64_t P) { return (size_t)((P + 255) / 256); }

__global__ __launch_bounds__(256) void prune_touch_kernel(int P, const int32_t* __restrict__ n_touched, const DqoRastHeader* __restrict__ header,
                                                          int32_t* __restrict__ head, uint32_t* __restrict__ touched) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = header == nullptr || header->overflow == 0u;  // (an overflowed render: n_touched is zero for every row)
    if (i == 0) atomicAdd(&head[valid ? PR_VALID : PR_INVALID], 1);
    if (!valid || i >= (size_t)P) return;
    if (n_touched[i] != 0) touched[i] = 1u;
}

__global__ __launch_bounds__(256) void prune_rows_kernel(PruneRows a) {
    __shared__ int s_last;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < (size_t)a.P;
    // (agent-scope loads: the last block clears the two words, and no block's read may be served from a scalar cache line)
    const int invalid = __hip_atomic_load(&a.head[PR_INVALID], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int valid = __hip_atomic_load(&a.head[PR_VALID], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool touched = false;
    if (in) {
        const uint32_t t = a.touched[i];
        if (t != 0u) a.touched[i] = 0u;
        touched = t != 0u;
    }
    const bool alive = in && a.alive[i] != 0;
    int fid = 0;
    if (alive) fid = a.frame_id[i];
    const bool window = alive && fid > a.lo && fid <= a.hi;
    const bool del = window && !touched && invalid == 0;
    const bool stable = del && a.stable[i] != 0;
    if (del) dqo_map_free_row(a, i), a.frame_id[i] = 0;
    dqo_line_count(a.head + PR_ACC, 0, window, lane);
    dqo_line_count(a.head + PR_ACC, 1, del && !stable, lane);
    dqo_line_count(a.head + PR_ACC, 2, del && stable, lane);
    dqo_line_count(a.head + PR_ACC, 5, alive && !del, lane);
    if (!dqo_last_block(a.head, &s_last)) return;
    dqo_line_totals(a.head + PR_ACC, 1u << 0 | 1u << 1 | 1u << 2 | 1u << 5, a.stats);  // the counts this kernel took
    if (threadIdx.x == 0) {  // (every block read the two words before it took its ticket)
        a.stats[3] = valid, a.stats[4] = invalid != 0 ? 1 : 0, a.stats[6] = 0, a.stats[7] = 0;
        atomicExch(&a.head[PR_INVALID], 0), atomicExch(&a.head[PR_VALID], 0);
    }
}

}  // namespace

static size_t dqo_prune_ws_bytes(int64_t P) { return PR_HEAD_WORDS * 4 + dqo_align_up((size_t)P * sizeof(uint32_t), 256); }

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_prune_workspace_bytes(int32_t P) { return dqo_prune_ws_bytes(P < 0 ? 0 : P); }

DQO_API int dqo_prune_cameras(int32_t H, int32_t W, const float* viewmatrix, const float* projection, const float* depth, int64_t pixel,
                              double cos_t, double sin_t, float* out_viewmatrix, float* out_projmatrix, float* out_focal, void* stream) {
    DQO_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 31), "bad image size");
    DQO_CHECK_ARG(viewmatrix && projection && depth, "null viewmatrix / projection / depth");
    DQO_CHECK_ARG(out_viewmatrix && out_projmatrix && out_focal, "null output");
    DQO_CHECK_ARG(pixel >= 0 && pixel < (int64_t)H * W, "pixel %lld outside the %d x %d image", (long long)pixel, H, W);
    DQO_LAUNCH("prune_cameras_kernel", prune_cameras_kernel, dim3(1), dim3(64), (hipStream_t)stream, viewmatrix, projection, depth, pixel, cos_t,
               sin_t, out_viewmatrix, out_projmatrix, out_focal);
    return DQO_OK;
}

DQO_API int dqo_prune_touch(int32_t P, const int32_t* n_touched, const DqoRastHeader* render_header, void* workspace, size_t workspace_bytes,
                            void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    if (P == 0) return DQO_OK;
    DQO_CHECK_ARG(n_touched != nullptr, "null n_touched");
    DQO_CHECK_WS("prune", workspace, workspace_bytes, dqo_prune_ws_bytes(P));
    int32_t* head = (int32_t*)workspace;
    DQO_LAUNCH("prune_touch_kernel", prune_touch_kernel, dim3((unsigned)pr_blocks(P)), dim3(256), (hipStream_t)stream, P, n_touched, render_header,
               head, (uint32_t*)(head + PR_HEAD_WORDS));
    return DQO_OK;
}

DQO_API int dqo_prune_rows(int32_t P, float* xyz, float* opacity_raw, float* scaling_raw, float* confidence, uint8_t* alive, uint8_t* row_flags,
                           uint8_t* stable, int32_t* add_tick, int32_t* depth_error_counter, int32_t* color_error_counter, int32_t* frame_id,
                           const float* park, int32_t lo, int32_t hi, void* workspace, size_t workspace_bytes, int32_t* stats, void* stream) {
    DQO_CHECK_ARG(P >= 0, "bad P");
    DQO_CHECK_ARG(lo <= hi, "bad window (%d, %d]", lo, hi);
    DQO_CHECK_ARG(stats != nullptr, "null stats");
    if (P == 0) return dqo_launch_zero_words(reinterpret_cast<uint32_t*>(stats), 8, (hipStream_t)stream);
    DQO_CHECK_ARG(xyz && opacity_raw && scaling_raw && confidence && alive && row_flags && stable && add_tick && depth_error_counter &&
                      color_error_counter && frame_id && park, "null per-Gaussian buffer / park");
    DQO_CHECK_WS("prune", workspace, workspace_bytes, dqo_prune_ws_bytes(P));
    PruneRows a;
    a.P = P, a.xyz = xyz, a.opacity_raw = opacity_raw, a.scaling_raw = scaling_raw, a.confidence = confidence, a.alive = alive;
    a.row_flags = row_flags, a.stable = stable, a.add_tick = add_tick, a.depth_error_counter = depth_error_counter;
    a.color_error_counter = color_error_counter, a.frame_id = frame_id, a.park = park, a.lo = lo, a.hi = hi;
    a.head = (int32_t*)workspace, a.touched = (uint32_t*)(a.head + PR_HEAD_WORDS), a.stats = stats;
    DQO_LAUNCH("prune_rows_kernel", prune_rows_kernel, dim3((unsigned)pr_blocks(P)), dim3(256), (hipStream_t)stream, a);
    return DQO_OK;
}

}  // extern "C"
