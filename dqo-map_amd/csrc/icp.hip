// Point-to-plane ICP normal equations for gfx950.
//
// Replaces, per Gauss-Newton iteration of /root/reference/SLAM/icp.py:
//   ICP.compute_residuals_jacobian :51-108 (transform, projective data association through warp_features / grid_sample
//   "nearest" :131-149, masks, residual, Jacobian), ICP.compute_jtj :110-115 and ICP.compute_jtr :117-123
// i.e. ~40 eager torch kernels and three [HW, 6]-sized temporaries, by ONE pass over the two vertex / normal maps that leaves
// J^T J (6x6), J^T r (6) and the number of valid pixels.  dqo_icp_normal_equations leaves the 6x6 solve and the se(3) update
// (icp.py:125-129, 248-312) to the host, as in the reference; dqo_icp_gauss_newton does them on the device in a second launch
// (icp_gauss_newton_kernel), so that the tracker's iterations need no host copy.
//
// Per pixel: p = R v0 + t, n = R n0; (u, v) = projection of p; q, m = vertex1 / normal1 at the nearest pixel to (u, v);
// r = m . (p - q); J = [p x m, m] (rotation first, icp.py:95-100); the pixel counts iff it is in view, both depths are
// positive, |p - q| <= distance_threshold and n . m > normal_threshold.  Sums are accumulated in fp64 per thread and reduced
// in a fixed order (block partials, then one finishing block): bitwise reproducible.
#include "dqo_common.h"

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_NSUM = 28;  // 21 upper-triangular J^T J + 6 J^T r + valid count

struct IcpPose {
    float R[9], t[3];
};

// the body of icp_partial_kernel, shared with icp_partial_kdev_kernel (intrinsics read from device memory)
__device__ __forceinline__ void icp_partial_body(int H, int W, const float* __restrict__ vertex0, const float* __restrict__ vertex1,
                                                 const float* __restrict__ normal0, const float* __restrict__ normal1,
                                                 const float* __restrict__ pose10, float fx, float fy, float cx, float cy, float dist_thr,
                                                 float normal_thr, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double s_red[ICP_THREADS / 64][ICP_NSUM];
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = pose10[4 * i + j];
        t[i] = pose10[4 * i + 3];
    }
    double acc[ICP_NSUM];
#pragma unroll
    for (int i = 0; i < ICP_NSUM; i++) acc[i] = 0.0;
    const int HW = H * W;
    const float hw = (float)(W - 1) / 2.0f, hh = (float)(H - 1) / 2.0f;
    for (int p = blockIdx.x * ICP_THREADS + threadIdx.x; p < HW; p += gridDim.x * ICP_THREADS) {
        const float v0x = vertex0[3 * p], v0y = vertex0[3 * p + 1], v0z = vertex0[3 * p + 2];
        const bool mask0 = v0z > 0.0f;
        // torch's matmul of a 3x3 by a 3-vector in fp32: sum in index order
        const float px = (R[0] * v0x + R[1] * v0y + R[2] * v0z) + t[0];
        const float py = (R[3] * v0x + R[4] * v0y + R[5] * v0z) + t[1];
        const float pz = (R[6] * v0x + R[7] * v0y + R[8] * v0z) + t[2];
        const float n0x = normal0[3 * p], n0y = normal0[3 * p + 1], n0z = normal0[3 * p + 2];
        const float nx = R[0] * n0x + R[1] * n0y + R[2] * n0z;
        const float ny = R[3] * n0x + R[4] * n0y + R[5] * n0z;
        const float nz = R[6] * n0x + R[7] * n0y + R[8] * n0z;
        const float u = (px / pz) * fx + cx, v = (py / pz) * fy + cy;
        const bool inview = (u > 0.f) && (u < (float)(W - 1)) && (v > 0.f) && (v < (float)(H - 1));
        bool ok = mask0 && inview;  // (NaN coordinates fail `inview`)
        float rx = 0.f, J0 = 0.f, J1 = 0.f, J2 = 0.f, J3 = 0.f, J4 = 0.f, J5 = 0.f;
        if (ok) {
            // warp_features -> grid_sample(mode="nearest", padding_mode="border", align_corners=True): normalise, unnormalise,
            // clip, round half to even
            const float un = u / hw - 1.0f, vn = v / hh - 1.0f;
            float gxf = ((un + 1.0f) / 2.0f) * (float)(W - 1), gyf = ((vn + 1.0f) / 2.0f) * (float)(H - 1);
            gxf = fminf((float)(W - 1), fmaxf(gxf, 0.f));
            gyf = fminf((float)(H - 1), fmaxf(gyf, 0.f));
            const int xi = (int)nearbyintf(gxf), yi = (int)nearbyintf(gyf);
            const int q = yi * W + xi;
            const float qx = vertex1[3 * q], qy = vertex1[3 * q + 1], qz = vertex1[3 * q + 2];
            const float mx = normal1[3 * q], my = normal1[3 * q + 1], mz = normal1[3 * q + 2];
            const float dx = px - qx, dy = py - qy, dz = pz - qz;
            const bool mask1 = qz > 0.f;
            const bool ndm = ((nx * mx + ny * my) + nz * mz) > normal_thr;
            const float dn = sqrtf((dx * dx + dy * dy) + dz * dz);
            ok = mask1 && ndm && !(dn > dist_thr);
            if (ok) {
                rx = (mx * dx + my * dy) + mz * dz;
                // J_rot = -(m^T [p]_x) = p x m (icp.py:96-97), J_trs = m
                J0 = -(my * pz - mz * py), J1 = -(-mx * pz + mz * px), J2 = -(mx * py - my * px);
                J3 = mx, J4 = my, J5 = mz;
            }
        }
        if (ok) {
            const double J[6] = {J0, J1, J2, J3, J4, J5};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) acc[k++] += J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; a++) acc[21 + a] += J[a] * (double)rx;
            acc[27] += 1.0;
        }
    }
    // wave reduction, then the block's four waves in order
#pragma unroll
    for (int i = 0; i < ICP_NSUM; i++) {
        double x = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        acc[i] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int i = 0; i < ICP_NSUM; i++) s_red[wave][i] = acc[i];
    __syncthreads();
    if (threadIdx.x < ICP_NSUM) {
        double x = 0.0;
        for (int w = 0; w < ICP_THREADS / 64; w++) x += s_red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * ICP_NSUM + threadIdx.x] = x;
    }
}

__global__ __launch_bounds__(ICP_THREADS) void icp_partial_kernel(int H, int W, const float* __restrict__ vertex0,
                                                                  const float* __restrict__ vertex1, const float* __restrict__ normal0,
                                                                  const float* __restrict__ normal1, const float* __restrict__ pose10,
                                                                  float fx, float fy, float cx, float cy, float dist_thr,
                                                                  float normal_thr, double* __restrict__ partial) {
    icp_partial_body(H, W, vertex0, vertex1, normal0, normal1, pose10, fx, fy, cx, cy, dist_thr, normal_thr, partial);
}

// the same pass with K * k_scale taken from a row-major 3x3 fp32 matrix in device memory (the tracker's per-level `K * downscale`)
__global__ __launch_bounds__(ICP_THREADS) void icp_partial_kdev_kernel(int H, int W, const float* __restrict__ vertex0,
                                                                       const float* __restrict__ vertex1, const float* __restrict__ normal0,
                                                                       const float* __restrict__ normal1, const float* __restrict__ pose10,
                                                                       const float* __restrict__ K, float k_scale, float dist_thr,
                                                                       float normal_thr, double* __restrict__ partial) {
    const DqoIntrinsics k = dqo_load_intrinsics(K, k_scale);
    icp_partial_body(H, W, vertex0, vertex1, normal0, normal1, pose10, k.fx, k.fy, k.cx, k.cy, dist_thr, normal_thr, partial);
}

__global__ void icp_finish_kernel(int nblk, const double* __restrict__ partial, float* __restrict__ JtJ, float* __restrict__ JtR,
                                  int32_t* __restrict__ valid_count) {
    const int i = threadIdx.x;
    if (i >= ICP_NSUM) return;
    double x = 0.0;
    for (int b = 0; b < nblk; b++) x += partial[(size_t)b * ICP_NSUM + i];
    if (i < 21) {
        int k = 0;
        for (int a = 0; a < 6; a++)
            for (int c = a; c < 6; c++, k++)
                if (k == i) JtJ[6 * a + c] = JtJ[6 * c + a] = (float)x;
    } else if (i < 27) {
        JtR[i - 21] = (float)x;
    } else {
        *valid_count = (int32_t)x;
    }
}

// Cholesky of the symmetric 6x6 A (row-major, double) into its lower triangle L; false unless every pivot is positive and finite
__device__ bool chol6(const double* A, double* L) {
    for (int j = 0; j < 6; j++) {
        double d = A[6 * j + j];
        for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        d = sqrt(d);
        L[6 * j + j] = d;
        for (int i = j + 1; i < 6; i++) {
            double x = A[6 * i + j];
            for (int k = 0; k < j; k++) x -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = x / d;
        }
    }
    return true;
}

// Moore-Penrose inverse of the symmetric 6x6 A through a cyclic Jacobi eigendecomposition A = V diag(lambda) V^T; eigenvalues at or
// below numpy.linalg.pinv's cutoff (1e-15 * the largest |lambda|) are dropped, so A == 0 gives 0.  A is overwritten.
__device__ void pinv6_jacobi(double* A, double* V, double* P) {
    for (int i = 0; i < 36; i++) V[i] = (i % 7 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 6; p++) {
            diag += A[6 * p + p] * A[6 * p + p];
            for (int q = p + 1; q < 6; q++) off += A[6 * p + q] * A[6 * p + q];
        }
        if (!(off > 1e-32 * diag)) break;  // converged (also ends on A == 0 and on non-finite entries)
        for (int p = 0; p < 5; p++)
            for (int q = p + 1; q < 6; q++) {
                const double apq = A[6 * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[6 * q + q] - A[6 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 6; k++) {  // A <- A G (columns p, q)
                    const double akp = A[6 * k + p], akq = A[6 * k + q];
                    A[6 * k + p] = c * akp - sn * akq;
                    A[6 * k + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 6; k++) {  // A <- G^T A (rows p, q)
                    const double apk = A[6 * p + k], aqk = A[6 * q + k];
                    A[6 * p + k] = c * apk - sn * aqk;
                    A[6 * q + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < 6; k++) {  // V <- V G
                    const double vkp = V[6 * k + p], vkq = V[6 * k + q];
                    V[6 * k + p] = c * vkp - sn * vkq;
                    V[6 * k + q] = sn * vkp + c * vkq;
                }
            }
    }
    double amax = 0.0;
    for (int k = 0; k < 6; k++) amax = fmax(amax, fabs(A[6 * k + k]));
    const double cutoff = 1e-15 * amax;
    for (int i = 0; i < 36; i++) P[i] = 0.0;
    for (int k = 0; k < 6; k++) {
        const double lam = A[6 * k + k];
        if (!(fabs(lam) > cutoff)) continue;
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) P[6 * i + j] += V[6 * i + k] * (V[6 * j + k] / lam);
    }
}

// One Gauss-Newton update on the device, after icp_partial_kernel (icp.py:33-47, 248-337 as dqo_icp.ICP restates them on the host):
// fold the partials in icp_finish_kernel's order, JtJ / JtR rounded to fp32, H = JtJ + damping * trace(JtJ) * I in fp32 (lev_mar_H),
// xi = -H^-1 JtR in double (Cholesky; a Jacobi pseudo-inverse when H is not positive definite), T = exp_se3(xi) in double,
// pose10 <- float(T) @ pose10 in fp32.  valid_count gets this iteration's count.  One block of 64 threads; thread 0 solves.
__global__ void icp_gauss_newton_kernel(int nblk, const double* __restrict__ partial, float damping, float* __restrict__ pose10,
                                        int32_t* __restrict__ valid_count) {
#pragma clang fp contract(off)
    __shared__ double s_sum[ICP_NSUM];
    __shared__ double s_A[36], s_L[36], s_V[36];
    const int i = threadIdx.x;
    if (i < ICP_NSUM) {
        // icp_finish_kernel's order; unrolled so that the loads of a stretch are in flight together (the adds stay in order)
        double x = 0.0;
#pragma unroll 16
        for (int b = 0; b < nblk; b++) x += partial[(size_t)b * ICP_NSUM + i];
        s_sum[i] = x;
    }
    __syncthreads();
    if (i != 0) return;
    float J[36], r[6];
    for (int a = 0, k = 0; a < 6; a++)
        for (int c = a; c < 6; c++, k++) J[6 * a + c] = J[6 * c + a] = (float)s_sum[k];
    for (int a = 0; a < 6; a++) r[a] = (float)s_sum[21 + a];
    float trace = 0.f;
    for (int a = 0; a < 6; a++) trace = trace + J[7 * a];
    const float eps = trace * damping;
    for (int k = 0; k < 36; k++) s_A[k] = (double)(k % 7 == 0 ? J[k] + eps : J[k]);
    double xi[6];
    if (chol6(s_A, s_L)) {
        double y[6];
        for (int a = 0; a < 6; a++) {  // L y = JtR, then L^T x = y
            double x = (double)r[a];
            for (int k = 0; k < a; k++) x -= s_L[6 * a + k] * y[k];
            y[a] = x / s_L[7 * a];
        }
        for (int a = 5; a >= 0; a--) {
            double x = y[a];
            for (int k = a + 1; k < 6; k++) x -= s_L[6 * k + a] * xi[k];
            xi[a] = x / s_L[7 * a];
        }
        for (int a = 0; a < 6; a++) xi[a] = -xi[a];
    } else {
        pinv6_jacobi(s_A, s_V, s_L);
        for (int a = 0; a < 6; a++) {
            double x = 0.0;
            for (int k = 0; k < 6; k++) x += -s_L[6 * a + k] * (double)r[k];
            xi[a] = x;
        }
    }
    // exp_se3 (icp.py:272-312): rotation first, translation through the left Jacobian
    const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
    const double wh[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double wh2[9];
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) wh2[3 * a + c] = wh[3 * a] * wh[c] + wh[3 * a + 1] * wh[3 + c] + wh[3 * a + 2] * wh[6 + c];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    double ew[9], jl[9];
    for (int k = 0; k < 9; k++) ew[k] = jl[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (th > 1e-8) {
        const double st = sin(th), ct = cos(th), th2 = th * th;
        for (int k = 0; k < 9; k++) {
            ew[k] += wh[k] * st / th + wh2[k] * (1.0 - ct) / th2;
            jl[k] += (1.0 - ct) / th2 * wh[k] + (th - st) / (th2 * th) * wh2[k];
        }
    }
    float T[16];
    for (int a = 0; a < 3; a++) {
        for (int c = 0; c < 3; c++) T[4 * a + c] = (float)ew[3 * a + c];
        T[4 * a + 3] = (float)(jl[3 * a] * xi[3] + jl[3 * a + 1] * xi[4] + jl[3 * a + 2] * xi[5]);
    }
    T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
    float P[16], out[16];
    for (int k = 0; k < 16; k++) P[k] = pose10[k];
    for (int a = 0; a < 4; a++)
        for (int c = 0; c < 4; c++)
            out[4 * a + c] = ((T[4 * a] * P[c] + T[4 * a + 1] * P[4 + c]) + T[4 * a + 2] * P[8 + c]) + T[4 * a + 3] * P[12 + c];
    for (int k = 0; k < 16; k++) pose10[k] = out[k];
    *valid_count = (int32_t)s_sum[27];
}

}  // namespace

static size_t dqo_icp_ws_bytes(void) { return sizeof(double) * ICP_NSUM * 1024; }

static int dqo_launch_icp(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1, const float* pose10,
                          float fx, float fy, float cx, float cy, float dist_thr, float normal_thr, float* JtJ, float* JtR, int32_t* valid_count,
                          void* ws, hipStream_t s) {
    const int HW = H * W;
    const int nblk = min(1024, (HW + ICP_THREADS - 1) / ICP_THREADS);
    double* partial = (double*)ws;
    DQO_LAUNCH("icp_partial_kernel", icp_partial_kernel, dim3(nblk), dim3(ICP_THREADS), s, H, W, vertex0, vertex1, normal0, normal1, pose10, fx,
               fy, cx, cy, dist_thr, normal_thr, partial);
    DQO_LAUNCH("icp_finish_kernel", icp_finish_kernel, dim3(1), dim3(64), s, nblk, partial, JtJ, JtR, valid_count);
    return DQO_OK;
}

static int dqo_launch_icp_gauss_newton(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1,
                                       float* pose10, const float* K, float k_scale, float dist_thr, float normal_thr, float damping,
                                       int32_t* valid_count, void* ws, hipStream_t s) {
    const int HW = H * W;
    const int nblk = min(1024, (HW + ICP_THREADS - 1) / ICP_THREADS);
    double* partial = (double*)ws;
    DQO_LAUNCH("icp_partial_kdev_kernel", icp_partial_kdev_kernel, dim3(nblk), dim3(ICP_THREADS), s, H, W, vertex0, vertex1, normal0, normal1,
               pose10, K, k_scale, dist_thr, normal_thr, partial);
    DQO_LAUNCH("icp_gauss_newton_kernel", icp_gauss_newton_kernel, dim3(1), dim3(64), s, nblk, partial, damping, pose10, valid_count);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_icp_workspace_bytes(void) { return dqo_icp_ws_bytes(); }

DQO_API int dqo_icp_normal_equations(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0,
                                     const float* normal1, const float* pose10, float fx, float fy, float cx, float cy, float dist_thr,
                                     float normal_thr, float* JtJ, float* JtR, int32_t* valid_count, void* ws, size_t ws_bytes,
                                     void* stream) {
    DQO_CHECK_ARG(H > 1 && W > 1 && (int64_t)H * W < (int64_t)0x7fffffff / 3, "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && normal1 && pose10 && JtJ && JtR && valid_count, "null pointer");
    DQO_CHECK_WS("icp", ws, ws_bytes, dqo_icp_ws_bytes());
    return dqo_launch_icp(H, W, vertex0, vertex1, normal0, normal1, pose10, fx, fy, cx, cy, dist_thr, normal_thr, JtJ, JtR, valid_count, ws,
                          (hipStream_t)stream);
}

DQO_API int dqo_icp_gauss_newton(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* normal1,
                                 float* pose10, const float* K, float k_scale, float dist_thr, float normal_thr, float damping,
                                 int32_t* valid_count, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(H > 1 && W > 1 && (int64_t)H * W < (int64_t)0x7fffffff / 3, "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && normal1 && pose10 && K && valid_count, "null pointer");
    DQO_CHECK_WS("icp", ws, ws_bytes, dqo_icp_ws_bytes());
    return dqo_launch_icp_gauss_newton(H, W, vertex0, vertex1, normal0, normal1, pose10, K, k_scale, dist_thr, normal_thr, damping, valid_count,
                                       ws, (hipStream_t)stream);
}

}  // extern "C"
