// The trajectory on the device for gfx950: what Tracker.tracking does between the tracker's answer and the mapper's input
// (SLAM/multiprocess/tracker.py:307-339), the mapper's keyframe test (SLAM/multiprocess/mapper.py:734-773) and the tracking metric
// (Tracker.eval_total_ate, tracker.py:341-346, 426-430; eval_ate, SLAM/utils.py:486-532), none of which reads anything back.
//
// traj_append_kernel (dqo_traj_append) — one small launch per frame; row i = header[0], which the launch advances itself.  One lane,
// double, one rounding per statement, none contracted (tests/traj_oracle.py restates them in this order):
//     pose[i]      relative mode, i > 0: pose[i-1] @ double(rel), entry (r, c) = ((a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c) + a_r3 b_3c
//                  (tracker.py:324, numpy's float64 @ of a float32 matrix); i == 0: the initial pose (identity without one; :318);
//                  absolute mode: the given world pose (:313, :322)
//     w2c, camera  dqo_traj_camera.h's statements (shared with traj_repose_kernel of map_repose.hip): the cofactor inverse of the affine
//                  pose; c2w, viewmatrix, projmatrix, campos rounded once each from the doubles
//     keyframe     on the rows i == 0 || (i + 1) % gaussian_update_frame == 0, with Wk, Tk / Wc, Tc the w2c of the last keyframe row / of
//                  this row (mapper.py:749-757, SLAM/utils.py:42-54): d_j = (Wk[0][j] Wc[0][j] + Wk[1][j] Wc[1][j]) + Wk[2][j] Wc[2][j],
//                  cos = (((d_0 + d_1) + d_2) - 1) / 2 NOT clamped, theta = acos(cos) * (180 / pi), e = Tk - Tc,
//                  l2 = sqrt((e0 e0 + e1 e1) + e2 e2); keyframe iff theta > theta_thres || l2 > trans_thres (NaN compares false)
//
// track_world_maps_kernel (dqo_track_world_maps) — transform_map of the vertex and the normal map (tracker.py:332-337, SLAM/utils.py:56-63)
// in one pixel launch, float32: out = ((r0 x + r1 y) + r2 z) + t per component, the normals without t (get_rot, utils.py:30-33).
//
// eval_ate_kernel (dqo_eval_ate) — the whole ATE curve in one launch: one block per prefix, three passes over its points in double,
// Horn's quaternion for the rotation.  Lanes by butterfly, the four waves in order, no atomics: a curve is the same bytes on every run.
#include "dqo_common.h"
#include "dqo_traj_camera.h"

namespace {

constexpr int TRAJ_THREADS = 256;

// ---- dqo_traj_append ------------------------------------------------------------------------------------------------------------

__global__ void traj_append_kernel(int cap, double* __restrict__ pose, double* __restrict__ pose_gt, int32_t* __restrict__ flags,
                                   double* __restrict__ kf_metric, int32_t* __restrict__ header, const float* __restrict__ rel,
                                   const double* __restrict__ abs_pose, const double* __restrict__ init_pose, const double* __restrict__ gt,
                                   const float* __restrict__ projection, float* __restrict__ c2w, float* __restrict__ viewmatrix,
                                   float* __restrict__ projmatrix, float* __restrict__ campos, int update_frame, double theta_thres,
                                   double trans_thres) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int i = header[DQO_TRAJ_HEADER_COUNT];
    if (i < 0 || i >= cap) {  // a full store: nothing is written but the overflow word
        header[DQO_TRAJ_HEADER_OVERFLOW] = 1;
        return;
    }
    double P[16];
    if (abs_pose) {
        for (int k = 0; k < 16; k++) P[k] = abs_pose[k];
    } else if (i == 0) {
        for (int k = 0; k < 16; k++) P[k] = init_pose ? init_pose[k] : (k % 5 == 0 ? 1.0 : 0.0);
    } else {
        const double* A = pose + (size_t)(i - 1) * 16;
        double B[16];
        for (int k = 0; k < 16; k++) B[k] = (double)rel[k];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++)
                P[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
    }
    for (int k = 0; k < 16; k++) pose[(size_t)i * 16 + k] = P[k];
    if (gt && pose_gt)
        for (int k = 0; k < 16; k++) pose_gt[(size_t)i * 16 + k] = gt[k];

    double W[9], T[3];
    traj_invert_affine(P, W, T);
    traj_store_camera(P, W, T, projection, c2w, nullptr, viewmatrix, projmatrix, campos);

    // check_keyframe on the rows where the mapper calls it
    int flag = 0;
    double theta = 0.0, l2 = 0.0;
    if (update_frame > 0 && (i == 0 || (i + 1) % update_frame == 0)) {
        flag = DQO_TRAJ_TESTED;
        const int k = header[DQO_TRAJ_HEADER_LAST_KEYFRAME];
        if (k < 0 || k >= i) {  // the first tested row enters the keyframe list and reports "not a keyframe" (mapper.py:736-748)
            flag |= DQO_TRAJ_LISTED;
            header[DQO_TRAJ_HEADER_LAST_KEYFRAME] = i;
        } else {
            double Wk[9], Tk[3];
            traj_invert_affine(pose + (size_t)k * 16, Wk, Tk);
            const double d0 = (Wk[0] * W[0] + Wk[3] * W[3]) + Wk[6] * W[6];
            const double d1 = (Wk[1] * W[1] + Wk[4] * W[4]) + Wk[7] * W[7];
            const double d2 = (Wk[2] * W[2] + Wk[5] * W[5]) + Wk[8] * W[8];
            const double cs = (((d0 + d1) + d2) - 1.0) / 2.0;
            theta = acos(cs) * (180.0 / 3.14159265358979323846);
            const double e0 = Tk[0] - T[0], e1 = Tk[1] - T[1], e2 = Tk[2] - T[2];
            l2 = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
            if (theta > theta_thres || l2 > trans_thres) {
                flag |= DQO_TRAJ_KEYFRAME | DQO_TRAJ_LISTED;
                header[DQO_TRAJ_HEADER_LAST_KEYFRAME] = i;
            }
        }
    }
    flags[i] = flag;
    kf_metric[2 * (size_t)i] = theta, kf_metric[2 * (size_t)i + 1] = l2;
    header[DQO_TRAJ_HEADER_COUNT] = i + 1;
}

// ---- dqo_track_world_maps -------------------------------------------------------------------------------------------------------

constexpr int WM_PIXELS = 4;                                  // pixels per thread: 12 floats, three 16-byte accesses
constexpr int WM_CHUNK = TRAJ_THREADS * WM_PIXELS * 3;        // floats of a map a block holds at a time

// One map's chunk [base, base + WM_CHUNK) of n3 floats: into LDS with lane-consecutive accesses (16 bytes per lane where VEC: the map's
// address is 16-byte aligned, and base is a multiple of 4), four pixels per thread transformed in LDS, out the way it came in.  src may
// be dst: a block reads its whole chunk before it writes any of it, and no other block touches the chunk.
template <bool VEC, bool TRANSLATE>
__device__ __forceinline__ void wm_chunk(const float* src, float* dst, int64_t base, int64_t n3, const float* R, const float* t, float* s) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int64_t left = n3 - base;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int q = k * TRAJ_THREADS + tid;
            if (4 * (int64_t)q + 3 < left) {
                *reinterpret_cast<float4*>(s + 4 * q) = *reinterpret_cast<const float4*>(src + base + 4 * q);
            } else {
                for (int j = 0; j < 4; j++)
                    if (4 * (int64_t)q + j < left) s[4 * q + j] = src[base + 4 * q + j];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int f = k * TRAJ_THREADS + tid;
            if (f < left) s[f] = src[base + f];
        }
    }
    __syncthreads();
    float* p = s + 12 * tid;  // the thread's four pixels (only the ones below `left` are stored)
#pragma unroll
    for (int j = 0; j < WM_PIXELS; j++) {
        const float x = p[3 * j], y = p[3 * j + 1], z = p[3 * j + 2];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = (R[3 * c] * x + R[3 * c + 1] * y) + R[3 * c + 2] * z;
            p[3 * j + c] = TRANSLATE ? v + t[c] : v;
        }
    }
    __syncthreads();
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int q = k * TRAJ_THREADS + tid;
            if (4 * (int64_t)q + 3 < left) {
                *reinterpret_cast<float4*>(dst + base + 4 * q) = *reinterpret_cast<const float4*>(s + 4 * q);
            } else {
                for (int j = 0; j < 4; j++)
                    if (4 * (int64_t)q + j < left) dst[base + 4 * q + j] = s[4 * q + j];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int f = k * TRAJ_THREADS + tid;
            if (f < left) dst[base + f] = s[f];
        }
    }
    __syncthreads();  // the next chunk reuses s
}

template <bool VEC>
__global__ __launch_bounds__(TRAJ_THREADS) void track_world_maps_kernel(int64_t n3, const float* vertex_c, const float* normal_c,
                                                                        const float* __restrict__ c2w, float* vertex_w, float* normal_w) {
    __shared__ __attribute__((aligned(16))) float s[WM_CHUNK];
    float R[9], t[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) R[3 * a + b] = c2w[4 * a + b];
        t[a] = c2w[4 * a + 3];
    }
    for (int64_t base = (int64_t)blockIdx.x * WM_CHUNK; base < n3; base += (int64_t)gridDim.x * WM_CHUNK) {
        wm_chunk<VEC, true>(vertex_c, vertex_w, base, n3, R, t, s);
        if (normal_c) wm_chunk<VEC, false>(normal_c, normal_w, base, n3, R, t, s);
    }
}

// ---- dqo_eval_ate ---------------------------------------------------------------------------------------------------------------

// every thread's a[0 .. NSUM) summed over the block: lanes by the xor butterfly, then the four waves in order; every thread gets the sums
template <int NSUM>
__device__ __forceinline__ void ate_block_sum(double (&a)[NSUM], double* s_red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < NSUM; q++) a[q] = dqo_wave_sum_f64(a[q], lane);
    __syncthreads();  // s_red is free again (the previous sums were read)
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NSUM; q++) s_red[wave * NSUM + q] = a[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NSUM; q++) a[q] = ((s_red[q] + s_red[NSUM + q]) + s_red[2 * NSUM + q]) + s_red[3 * NSUM + q];
}

// The rotation R (3x3 row-major) that takes the zero-centred model onto the zero-centred data in the least-squares sense, from
// S[3 a + b] = sum model_a data_b: Horn's closed form — the unit quaternion is the eigenvector of the largest eigenvalue of the symmetric
// 4x4 N(S), found by cyclic Jacobi in double (as pinv6_jacobi of icp.hip).  Always a proper rotation: what the reference's SVD with
// S[2,2] = -1 yields (SLAM/utils.py:508-512).  Where the optimum is not unique (one point, collinear points, a camera that stands still)
// any eigenvector of the largest eigenvalue gives the same error.
__device__ void ate_horn_rotation(const double* S, double* R) {
#pragma clang fp contract(off)
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[16] = {(Sxx + Syy) + Szz, Syz - Szy,         Szx - Sxz,          Sxy - Syx,
                    Syz - Szy,         (Sxx - Syy) - Szz, Sxy + Syx,          Szx + Sxz,
                    Szx - Sxz,         Sxy + Syx,         (Syy - Sxx) - Szz,  Syz + Szy,
                    Sxy - Syx,         Szx + Sxz,         Syz + Szy,          (Szz - Sxx) - Syy};
    double V[16];
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; p++) {
            diag += A[4 * p + p] * A[4 * p + p];
            for (int q = p + 1; q < 4; q++) off += A[4 * p + q] * A[4 * p + q];
        }
        if (!(off > 1e-34 * diag)) break;  // converged (also ends on A == 0 and on non-finite entries)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[4 * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[4 * q + q] - A[4 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 4; k++) {  // A <- A G (columns p, q)
                    const double akp = A[4 * k + p], akq = A[4 * k + q];
                    A[4 * k + p] = c * akp - sn * akq;
                    A[4 * k + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 4; k++) {  // A <- G^T A (rows p, q)
                    const double apk = A[4 * p + k], aqk = A[4 * q + k];
                    A[4 * p + k] = c * apk - sn * aqk;
                    A[4 * q + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < 4; k++) {  // V <- V G
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = c * vkp - sn * vkq;
                    V[4 * k + q] = sn * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int k = 1; k < 4; k++)
        if (A[4 * k + k] > A[4 * m + m]) m = k;
    double w = V[m], x = V[4 + m], y = V[8 + m], z = V[12 + m];
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    if (!(nrm > 0.0) || !isfinite(nrm)) w = 1.0, x = y = z = 0.0;
    else w /= nrm, x /= nrm, y /= nrm, z /= nrm;
    R[0] = ((w * w + x * x) - y * y) - z * z, R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z), R[4] = ((w * w - x * x) + y * y) - z * z, R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = ((w * w - x * x) - y * y) + z * z;
}

// point j of a stream: (stride doubles between points, cstride between a point's components)
__device__ __forceinline__ void ate_point(const double* __restrict__ p, int64_t stride, int64_t cstride, int j, double* v) {
    const double* q = p + (int64_t)j * stride;
    v[0] = q[0], v[1] = q[cstride], v[2] = q[2 * cstride];
}

__global__ __launch_bounds__(TRAJ_THREADS) void eval_ate_kernel(int N, const double* __restrict__ model, int64_t m_stride, int64_t m_cstride,
                                                                const double* __restrict__ data, int64_t d_stride, int64_t d_cstride,
                                                                double* __restrict__ ate, double* __restrict__ fit, double* __restrict__ fits) {
#pragma clang fp contract(off)
    __shared__ double s_red[4 * 9];
    __shared__ double s_R[9];
    const int tid = threadIdx.x;
    for (int n = (int)blockIdx.x + 1; n <= N; n += (int)gridDim.x) {  // the prefix of length n
        // 1. the two means
        double mean[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < n; j += TRAJ_THREADS) {
            double m[3], d[3];
            ate_point(model, m_stride, m_cstride, j, m), ate_point(data, d_stride, d_cstride, j, d);
            for (int a = 0; a < 3; a++) mean[a] += m[a], mean[3 + a] += d[a];
        }
        ate_block_sum<6>(mean, s_red);
        for (int a = 0; a < 6; a++) mean[a] = mean[a] / (double)n;
        // 2. the sum of outer products of the zero-centred points
        double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < n; j += TRAJ_THREADS) {
            double m[3], d[3];
            ate_point(model, m_stride, m_cstride, j, m), ate_point(data, d_stride, d_cstride, j, d);
            for (int a = 0; a < 3; a++) m[a] = m[a] - mean[a], d[a] = d[a] - mean[3 + a];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) S[3 * a + b] += m[a] * d[b];
        }
        ate_block_sum<9>(S, s_red);
        if (tid == 0) {
            double R[9];
            ate_horn_rotation(S, R);
            for (int k = 0; k < 9; k++) s_R[k] = R[k];
            // the alignment itself: rot, and trans = mean(data) - rot mean(model) (SLAM/utils.py:512-513)
            double* row = fits + (size_t)(n - 1) * 12;
            for (int a = 0; a < 3; a++) {
                for (int b = 0; b < 3; b++) row[3 * a + b] = R[3 * a + b];
                row[9 + a] = mean[3 + a] - ((R[3 * a] * mean[0] + R[3 * a + 1] * mean[1]) + R[3 * a + 2] * mean[2]);
            }
            if (n == N && fit)
                for (int k = 0; k < 12; k++) fit[k] = row[k];
        }
        __syncthreads();
        double R[9];
        for (int k = 0; k < 9; k++) R[k] = s_R[k];
        // 3. the squared lengths of R (m - mean m) - (d - mean d)
        double e2[1] = {0.0};
        for (int j = tid; j < n; j += TRAJ_THREADS) {
            double m[3], d[3];
            ate_point(model, m_stride, m_cstride, j, m), ate_point(data, d_stride, d_cstride, j, d);
            for (int a = 0; a < 3; a++) m[a] = m[a] - mean[a], d[a] = d[a] - mean[3 + a];
            double q = 0.0;
            for (int a = 0; a < 3; a++) {
                const double e = (((R[3 * a] * m[0] + R[3 * a + 1] * m[1]) + R[3 * a + 2] * m[2])) - d[a];
                q += e * e;
            }
            e2[0] += q;
        }
        ate_block_sum<1>(e2, s_red);  // (its first barrier also orders this prefix's reads of s_R before the next prefix's write)
        if (tid == 0) ate[n - 1] = sqrt(e2[0] / (double)n) * 100.0;
    }
}

}  // namespace

static size_t dqo_eval_ate_ws_bytes(int64_t N) { return N < 1 || N > DQO_ATE_MAX_POINTS ? 0 : dqo_align_up((size_t)N * 12 * sizeof(double), 256); }

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API int dqo_traj_append(int32_t cap, double* pose, double* pose_gt, int32_t* flags, double* kf_metric, int32_t* header, const float* rel,
                            const double* abs_pose, const double* init_pose, const double* gt, const float* projection, float* c2w,
                            float* viewmatrix, float* projmatrix, float* campos, int32_t gaussian_update_frame, double theta_thres,
                            double trans_thres, void* stream) {
    DQO_CHECK_ARG(cap >= 1, "bad capacity");
    DQO_CHECK_ARG(pose && flags && kf_metric && header, "null pointer");
    DQO_CHECK_ARG((rel != nullptr) != (abs_pose != nullptr), "one of the relative and the absolute pose");
    DQO_CHECK_ARG(!gt || pose_gt, "a ground-truth pose without a store for it");
    DQO_CHECK_ARG(!projmatrix || projection, "projmatrix without a projection");
    DQO_CHECK_ARG(gaussian_update_frame >= 0, "bad gaussian_update_frame");
    DQO_LAUNCH("traj_append_kernel", traj_append_kernel, dim3(1), dim3(64), (hipStream_t)stream, cap, pose, pose_gt, flags, kf_metric, header, rel,
               abs_pose, init_pose, gt, projection, c2w, viewmatrix, projmatrix, campos, gaussian_update_frame, theta_thres, trans_thres);
    return DQO_OK;
}

DQO_API int dqo_track_world_maps(int32_t H, int32_t W, const float* vertex_c, const float* normal_c, const float* c2w, float* vertex_w,
                                 float* normal_w, void* stream) {
    DQO_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)0x7fffffff / 3, "bad image size");
    DQO_CHECK_ARG(vertex_c && vertex_w && c2w, "null pointer");
    DQO_CHECK_ARG((normal_c != nullptr) == (normal_w != nullptr), "the normal map and its output come together");
    const int64_t n3 = (int64_t)H * W * 3;
    const int grid = (int)((n3 + WM_CHUNK - 1) / WM_CHUNK);
    const bool vec = (((uintptr_t)vertex_c | (uintptr_t)vertex_w | (uintptr_t)normal_c | (uintptr_t)normal_w) & 15) == 0;
    if (vec)
        DQO_LAUNCH("track_world_maps_kernel", track_world_maps_kernel<true>, dim3(grid), dim3(TRAJ_THREADS), (hipStream_t)stream, n3, vertex_c,
                   normal_c, c2w, vertex_w, normal_w);
    else
        DQO_LAUNCH("track_world_maps_kernel", track_world_maps_kernel<false>, dim3(grid), dim3(TRAJ_THREADS), (hipStream_t)stream, n3, vertex_c,
                   normal_c, c2w, vertex_w, normal_w);
    return DQO_OK;
}

DQO_API size_t dqo_eval_ate_workspace_bytes(int32_t N) { return dqo_eval_ate_ws_bytes(N); }

DQO_API int dqo_eval_ate(int32_t N, const double* model, int64_t model_stride, int64_t model_cstride, const double* data, int64_t data_stride,
                         int64_t data_cstride, double* ate, double* fit, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(N >= 1 && N <= DQO_ATE_MAX_POINTS, "bad point count");
    DQO_CHECK_ARG(model && data && ate, "null pointer");
    DQO_CHECK_ARG(model_stride >= 0 && model_cstride >= 0 && data_stride >= 0 && data_cstride >= 0, "bad stride");
    DQO_CHECK_WS("ate", ws, ws_bytes, dqo_eval_ate_ws_bytes(N));
    const int grid = min((int)N, 16384);
    DQO_LAUNCH("eval_ate_kernel", eval_ate_kernel, dim3(grid), dim3(TRAJ_THREADS), (hipStream_t)stream, N, model, model_stride, model_cstride,
               data, data_stride, data_cstride, ate, fit, (double*)ws);
    return DQO_OK;
}

}  // extern "C"
