// Pose corrections on the device for gfx950: dqo_traj_repose (include/dqo_raster.h states the rule).
//
// Mapping.update_poses (SLAM/multiprocess/mapper.py:256-263; slam.py:126-127 before every mapping(), :181-182 before the final
// global_optimization) hands Camera.updatePose (scene/cameras.py:165-183) the corrected world pose of every processed frame and keyframe;
// Tracker.save_traj (tracker.py:399-401) replaces pose_es by the same set, and metric.py:181 / make_mesh.py:199 / metric_obj.py:212 run
// updatePose per dataset frame.  Here the poses live in a trajectory's float64 store and the cameras in tensors captured graphs read in
// place (a window graph's settings, a keyframe bank's camera rows): ONE launch rewrites the store and re-forms every camera.
//
// The statements of a launch (tests/repose_oracle.py restates them):
//   1. count = header[DQO_TRAJ_HEADER_COUNT] clipped to [0, cap];  rows = new_pose ? min(count, n_new) : 0
//   2. pose[r] = new_pose[r] for r < rows: 8-byte words, exact bytes, all threads of the grid in stride
//   3. target t (one lane each): row outside [0, count) -> nothing written; else P = (new_pose && row < n_new) ? new_pose[row] : pose[row]
//      — never a store row that 2. writes — and dqo_traj_camera.h's statements into the target's non-NULL destinations, 4-byte stores
//   4. block 0: skipped = targets whose row is outside [0, count), counted by its 256 threads in stride and summed lanes by butterfly,
//      the four waves in order; one thread: stats = (rows, T - skipped, skipped, 0) and, with a bank state, its FORCE word = 1
// No atomics, no memset, nothing read back: the same bytes on every run, capturable.  pose_gt, flags, kf_metric and the header are not
// arguments: the reference never re-tests a keyframe.
//
// What bounds it: about 200 double operations per target and 128 bytes per rewritten row; a launch of 45 targets is one block.
#include "dqo_common.h"
#include "dqo_traj_camera.h"

namespace {

constexpr int REPOSE_THREADS = 256;
constexpr int REPOSE_MAX_BLOCKS = 1024;  // of the copy's stride; the grid always covers the targets

__global__ __launch_bounds__(REPOSE_THREADS) void traj_repose_kernel(DqoTrajRepose a) {
#pragma clang fp contract(off)
    __shared__ int s_skipped[REPOSE_THREADS / 64];
    const int tid = threadIdx.x;
    const int count = min(max(a.header[DQO_TRAJ_HEADER_COUNT], 0), a.cap);
    const int rows = a.new_pose != nullptr ? min(count, a.n_new) : 0;

    // 2. the store
    if (rows > 0) {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.new_pose);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.pose);
        const size_t words = (size_t)rows * 16, step = (size_t)gridDim.x * REPOSE_THREADS;
        for (size_t u = (size_t)blockIdx.x * REPOSE_THREADS + tid; u < words; u += step) dst[u] = src[u];
    }

    // 3. the cameras
    const int64_t t = (int64_t)blockIdx.x * REPOSE_THREADS + tid;
    if (t < a.T) {
        const DqoReposeTarget g = a.targets[t];
        if (g.row >= 0 && g.row < count) {
            const double* src = (a.new_pose != nullptr && g.row < a.n_new ? a.new_pose : a.pose) + (size_t)g.row * 16;
            double P[16], W[9], Tr[3];
            for (int k = 0; k < 16; k++) P[k] = src[k];
            traj_invert_affine(P, W, Tr);
            traj_store_camera(P, W, Tr, a.projection, g.c2w, g.w2c, g.viewmatrix, a.projection != nullptr ? g.projmatrix : nullptr, g.campos);
        }
    }

    // 4. the counts and the bank's force word
    if (blockIdx.x != 0) return;
    int skipped = 0;
    for (int q = tid; q < a.T; q += REPOSE_THREADS) {
        const int64_t row = a.targets[q].row;
        skipped += (row < 0 || row >= count) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) skipped += __shfl_xor(skipped, off, 64);
    if ((tid & 63) == 0) s_skipped[tid >> 6] = skipped;
    __syncthreads();
    if (tid != 0) return;
    skipped = ((s_skipped[0] + s_skipped[1]) + s_skipped[2]) + s_skipped[3];
    if (a.stats != nullptr) a.stats[0] = rows, a.stats[1] = a.T - skipped, a.stats[2] = skipped, a.stats[3] = 0;
    if (a.bank_state != nullptr) a.bank_state[DQO_WINDOW_BANK_FORCE] = 1;
}

}  // namespace

// ---- entry point (include/dqo_raster.h): argument validation, the call ----
extern "C" {

DQO_API int dqo_traj_repose(const DqoTrajRepose* r, void* stream) {
    DQO_CHECK_ARG(r != nullptr, "null arguments");
    DQO_CHECK_ARG(r->cap >= 1, "bad capacity");
    DQO_CHECK_ARG(r->pose && r->header, "null pointer");
    DQO_CHECK_ARG(r->n_new >= 0, "bad n_new %d", r->n_new);
    DQO_CHECK_ARG(r->T >= 0, "bad target count %d", r->T);
    DQO_CHECK_ARG(r->T == 0 || r->targets != nullptr, "targets without a table");
    DQO_CHECK_ARG(!(r->flags & DQO_REPOSE_HAS_PROJMATRIX) || r->projection != nullptr, "projmatrix without a projection");
    const size_t words = r->new_pose ? (size_t)std::min(r->cap, r->n_new) * 16 : 0;
    const size_t per_block = (size_t)REPOSE_THREADS * 4;  // four words of the copy per thread
    const int copy_blocks = (int)std::min<size_t>((size_t)REPOSE_MAX_BLOCKS, (words + per_block - 1) / per_block);
    const int grid = std::max(1, std::max(copy_blocks, (int)(((int64_t)r->T + REPOSE_THREADS - 1) / REPOSE_THREADS)));
    DQO_LAUNCH("traj_repose_kernel", traj_repose_kernel, dim3(grid), dim3(REPOSE_THREADS), (hipStream_t)stream, *r);
    return DQO_OK;
}

}  // extern "C"
