// Per-frame geometry of DQO-MAP's ICP tracker for gfx950: what /root/reference runs around the normal equations (icp.hip) in
// eager torch, as a handful of stream-ordered launches with no host synchronisation:
//
//   preprocess  Tracker.map_preprocess's geometry (SLAM/multiprocess/tracker.py:135-156): optional bilateralFilter_torch
//               (SLAM/utils.py:607-646), range mask, compute_vertex_map, compute_normal_map, compute_confidence_map
//               (utils.py:65-142) and the invalid-confidence mask.  Two launches: depth + vertex + min / max block partials, then
//               normals / confidence / mask / zeroing (the normal's min / max rule needs the whole map's extremes first).
//   pyramid     ImagePyramids("max") + build_vertex_pyramid + build_normal_pyramid (SLAM/icp.py:340-358, utils.py:542-558) for every
//               level at once: two launches (pooled vertex maps + min / max partials, then normals).
//   fill        IcpTracker.update_last_status (icp.py:403-421): the model depth takes the frame depth where they disagree; in place.
//   p2p loss    point2plane_loss of predict_pose's failure test (icp.py:7-14, 450-457): pixel-aligned, no data association; block
//               partials in fp64, then one finishing wave that also writes success and the last ICP level's valid ratio.
//
// Per-pixel arithmetic is fp32 in the reference's operation order (contraction off); where torch's CPU kernels fuse a multiply-add
// (torch.cross, the 2-norm of 3-vectors) the same fma is written out, so the unfiltered maps reproduce a CPU run of the reference
// (tests/golden/tracking_golden.npz) exactly; torch's GPU kernels may round those steps differently.  The bilateral filter's expf
// is not torch's exp: filtered depths agree to about an ulp.  Min / max are exact; sums are fp64 in a fixed order: every output is
// bitwise reproducible run to run.  The intrinsics K are a row-major 3x3 fp32 matrix in DEVICE memory, read by the kernels: a
// caller's per-frame GPU intrinsic costs no host read.
#include "dqo_common.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_BLOCKS = 1024;      // pixel kernels with block partials stride over at most this many blocks
constexpr int TR_PYR_MAX_BLOCKS = 256;   // ... per pyramid level
constexpr int TR_MAX_LEVELS = 4;

struct TrackLevel {
    int h, w, pool, off, blk0, nblk;  // size, pooling window, first pixel in the packed maps, first block and block count
    float scale;                       // K * scale for this level's vertex map (1 / pool)
};
struct TrackLevels {
    int L;
    TrackLevel lv[TR_MAX_LEVELS];
};

// torch.norm / linalg.vector_norm of a 3-vector (CPU kernel): sqrt(fma(z, z, fma(y, y, x * x)))
__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(__fmaf_rn(z, z, __fmaf_rn(y, y, x * x))); }

// compute_normal_map at (x, y) of a [h, w, 3] vertex map: Sobel with replicate padding in conv2d's tap order, n = cross(dy, dx)
// (torch.cross: fma(a_j, b_k, -(a_k * b_j))), n / (|n| + 1e-8), zero where z <= zmin or z >= zmax
__device__ __forceinline__ void sobel_normal(const float* __restrict__ V, int h, int w, int x, int y, float zmin, float zmax, float n[3]) {
#pragma clang fp contract(off)
    const float z = V[3 * (y * w + x) + 2];
    if (z <= zmin || z >= zmax) {
        n[0] = n[1] = n[2] = 0.f;
        return;
    }
    const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
    const float* r0 = V + 3 * (ym * w);
    const float* r1 = V + 3 * (y * w);
    const float* r2 = V + 3 * (yp * w);
    float dx[3], dy[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a00 = r0[3 * xm + c], a01 = r0[3 * x + c], a02 = r0[3 * xp + c];
        const float a10 = r1[3 * xm + c], a12 = r1[3 * xp + c];
        const float a20 = r2[3 * xm + c], a21 = r2[3 * x + c], a22 = r2[3 * xp + c];
        dx[c] = ((((-a00 + a02) - 2.f * a10) + 2.f * a12) - a20) + a22;
        dy[c] = ((((-a00 - 2.f * a01) - a02) + a20) + 2.f * a21) + a22;
    }
    const float c0 = __fmaf_rn(dy[1], dx[2], -(dy[2] * dx[1]));
    const float c1 = __fmaf_rn(dy[2], dx[0], -(dy[0] * dx[2]));
    const float c2 = __fmaf_rn(dy[0], dx[1], -(dy[1] * dx[0]));
    const float m = norm3(c0, c1, c2) + 1e-8f;
    n[0] = c0 / m, n[1] = c1 / m, n[2] = c2 / m;
}

// F.cosine_similarity(a, b, dim=-1) (eps 1e-8): each vector over max(|v|, eps), then the dot product
__device__ __forceinline__ float cosine3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float na = fmaxf(norm3(ax, ay, az), 1e-8f), nb = fmaxf(norm3(bx, by, bz), 1e-8f);
    return ((ax / na) * (bx / nb) + (ay / na) * (by / nb)) + (az / na) * (bz / nb);
}

// min / max of a block (every thread passes its running values); thread 0 gets the result
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
    __shared__ float s_lo[TR_THREADS / 64], s_hi[TR_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < TR_THREADS / 64; k++) lo = fminf(lo, s_lo[k]), hi = fmaxf(hi, s_hi[k]);
}

// every block folds the n (min, max) partials it needs; min / max are exact, so the order does not matter
__device__ __forceinline__ void fold_minmax(const float* __restrict__ partial, int n, float& zmin, float& zmax) {
    __shared__ float s_res[2];
    float lo = INFINITY, hi = -INFINITY;
    for (int b = threadIdx.x; b < n; b += TR_THREADS) lo = fminf(lo, partial[2 * b]), hi = fmaxf(hi, partial[2 * b + 1]);
    block_minmax(lo, hi);
    if (threadIdx.x == 0) s_res[0] = lo, s_res[1] = hi;
    __syncthreads();
    zmin = s_res[0], zmax = s_res[1];
}

// bilateralFilter_torch(depth, 5, 2, 2): circular footprint, zero padding, zero taps get no weight, 0 / 0 -> 0
__device__ float bilateral5(const float* __restrict__ depth, int H, int W, int x, int y) {
#pragma clang fp contract(off)
    const float d = depth[y * W + x];
    float wsum = 0.f, psum = 0.f;
    for (int i = -5; i <= 5; i++) {
        for (int j = -5; j <= 5; j++) {
            if (i * i + j * j > 25) continue;
            const int yy = y + i, xx = x + j;
            const float nb = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? depth[yy * W + xx] : 0.f;
            const float spatial = -(float)(i * i + j * j) / 8.f;  // -(i^2 + j^2) / (2 sigma_space^2), exact
            const float diff = d - nb;
            const float color = -(diff * diff) / 8.f;
            const float wgt = expf(spatial + color) * (nb != 0.f ? 1.f : 0.f);
            wsum = wsum + wgt;
            psum = psum + wgt * nb;
        }
    }
    return wsum == 0.f ? 0.f : psum / wsum;
}

__global__ __launch_bounds__(TR_THREADS) void track_depth_kernel(int H, int W, const float* __restrict__ depth, int filter, float dmin,
                                                                 float dmax, const float* __restrict__ K, float* __restrict__ dws,
                                                                 float* __restrict__ vws, float* __restrict__ partial) {
#pragma clang fp contract(off)
    const DqoIntrinsics k = dqo_load_intrinsics(K, 1.0f);
    const int HW = H * W;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = blockIdx.x * TR_THREADS + threadIdx.x; p < HW; p += gridDim.x * TR_THREADS) {
        const int y = p / W, x = p - y * W;
        float d = filter ? bilateral5(depth, H, W, x, y) : depth[p];
        d = (d > dmin && d < dmax) ? d : 0.f;
        dws[p] = d;
        vws[3 * p] = (((float)x - k.cx) / k.fx) * d;
        vws[3 * p + 1] = (((float)y - k.cy) / k.fy) * d;
        vws[3 * p + 2] = d;
        lo = fminf(lo, d), hi = fmaxf(hi, d);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = lo, partial[2 * blockIdx.x + 1] = hi;
}

__global__ __launch_bounds__(TR_THREADS) void track_geometry_kernel(int H, int W, const float* __restrict__ K, float conf_thr,
                                                                    const float* __restrict__ dws, const float* __restrict__ vws,
                                                                    const float* __restrict__ partial, int nblk, float* __restrict__ depth_out,
                                                                    float* __restrict__ vertex_out, float* __restrict__ normal_out,
                                                                    float* __restrict__ conf_out, uint8_t* __restrict__ invalid_out) {
#pragma clang fp contract(off)
    const DqoIntrinsics k = dqo_load_intrinsics(K, 1.0f);
    float zmin, zmax;
    fold_minmax(partial, nblk, zmin, zmax);
    const int HW = H * W;
    for (int p = blockIdx.x * TR_THREADS + threadIdx.x; p < HW; p += gridDim.x * TR_THREADS) {
        const int y = p / W, x = p - y * W;
        float n[3];
        sobel_normal(vws, H, W, x, y, zmin, zmax, n);
        // compute_confidence_map: |cos(n, ray / (|ray| + 1e-8))|
        float rx = ((float)x - k.cx) / k.fx, ry = ((float)y - k.cy) / k.fy, rz = 1.f;
        const float rm = norm3(rx, ry, rz) + 1e-8f;
        rx = rx / rm, ry = ry / rm, rz = rz / rm;
        const float conf = fabsf(cosine3(n[0], n[1], n[2], rx, ry, rz));
        const bool invalid = (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) || conf < conf_thr;
        depth_out[p] = invalid ? 0.f : dws[p];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            vertex_out[3 * p + c] = invalid ? 0.f : vws[3 * p + c];
            normal_out[3 * p + c] = invalid ? 0.f : n[c];
        }
        conf_out[p] = invalid ? 0.f : conf;
        invalid_out[p] = invalid ? 1 : 0;
    }
}

__device__ __forceinline__ int level_of_block(const TrackLevels& py) {
    int l = 0;
    while (l + 1 < py.L && (int)blockIdx.x >= py.lv[l + 1].blk0) l++;
    return l;
}

__global__ __launch_bounds__(TR_THREADS) void track_pyr_vertex_kernel(int W, const float* __restrict__ depth, const float* __restrict__ K,
                                                                      TrackLevels py, float* __restrict__ vertex, float* __restrict__ partial) {
#pragma clang fp contract(off)
    const TrackLevel lv = py.lv[level_of_block(py)];
    const DqoIntrinsics in = dqo_load_intrinsics(K, lv.scale);
    const int n = lv.h * lv.w, k = lv.pool;
    float* V = vertex + 3 * (size_t)lv.off;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = ((int)blockIdx.x - lv.blk0) * TR_THREADS + threadIdx.x; p < n; p += lv.nblk * TR_THREADS) {
        const int y = p / lv.w, x = p - y * lv.w;
        // MaxPool2d(k, k): the window's maximum, NaN propagates
        float d = -INFINITY;
        for (int a = 0; a < k; a++)
            for (int b = 0; b < k; b++) {
                const float v = depth[(y * k + a) * W + x * k + b];
                d = (v > d || isnan(v)) ? v : d;
            }
        V[3 * p] = (((float)x - in.cx) / in.fx) * d;
        V[3 * p + 1] = (((float)y - in.cy) / in.fy) * d;
        V[3 * p + 2] = d;
        lo = fminf(lo, d), hi = fmaxf(hi, d);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = lo, partial[2 * blockIdx.x + 1] = hi;
}

__global__ __launch_bounds__(TR_THREADS) void track_pyr_normal_kernel(TrackLevels py, const float* __restrict__ vertex,
                                                                      const float* __restrict__ partial, float* __restrict__ normal) {
    const TrackLevel lv = py.lv[level_of_block(py)];
    float zmin, zmax;
    fold_minmax(partial + 2 * lv.blk0, lv.nblk, zmin, zmax);
    const int n = lv.h * lv.w;
    const float* V = vertex + 3 * (size_t)lv.off;
    float* N = normal + 3 * (size_t)lv.off;
    for (int p = ((int)blockIdx.x - lv.blk0) * TR_THREADS + threadIdx.x; p < n; p += lv.nblk * TR_THREADS) {
        const int y = p / lv.w, x = p - y * lv.w;
        float nn[3];
        sobel_normal(V, lv.h, lv.w, x, y, zmin, zmax, nn);
        N[3 * p] = nn[0], N[3 * p + 1] = nn[1], N[3 * p + 2] = nn[2];
    }
}

__global__ __launch_bounds__(TR_THREADS) void track_fill_kernel(int HW, float* __restrict__ render_depth, const float* __restrict__ frame_depth,
                                                                const float* __restrict__ render_normal, const float* __restrict__ frame_normal,
                                                                float dist_thr, float normal_thr) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= HW) return;
    const float r = render_depth[p], f = frame_depth[p];
    const float c = cosine3(render_normal[3 * p], render_normal[3 * p + 1], render_normal[3 * p + 2], frame_normal[3 * p],
                            frame_normal[3 * p + 1], frame_normal[3 * p + 2]);
    const bool normal_mask = (1.f - c) > normal_thr;
    if (((fabsf(r - f) > dist_thr) || r == 0.f || normal_mask) && f > 0.f) render_depth[p] = f;
}

__global__ __launch_bounds__(TR_THREADS) void track_p2p_partial_kernel(int HW, const float* __restrict__ vertex0, const float* __restrict__ vertex1,
                                                                       const float* __restrict__ normal0, const float* __restrict__ pose10,
                                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double s_red[TR_THREADS / 64];
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = pose10[4 * i + j];
        t[i] = pose10[4 * i + 3];
    }
    double acc = 0.0;
    for (int p = blockIdx.x * TR_THREADS + threadIdx.x; p < HW; p += gridDim.x * TR_THREADS) {
        const float ax = vertex1[3 * p], ay = vertex1[3 * p + 1], az = vertex1[3 * p + 2];
        // v1 @ R^T + t, then ((p1 - v0) * n0).sum(-1), squared
        const float px = (R[0] * ax + R[1] * ay + R[2] * az) + t[0];
        const float py = (R[3] * ax + R[4] * ay + R[5] * az) + t[1];
        const float pz = (R[6] * ax + R[7] * ay + R[8] * az) + t[2];
        const float r = ((px - vertex0[3 * p]) * normal0[3 * p] + (py - vertex0[3 * p + 1]) * normal0[3 * p + 1]) +
                        (pz - vertex0[3 * p + 2]) * normal0[3 * p + 2];
        acc += (double)(r * r);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = 0.0;
        for (int w = 0; w < TR_THREADS / 64; w++) x += s_red[w];
        partial[blockIdx.x] = x;
    }
}

// one wave: lane l sums the partials l, l + 64, ... in order, then a fixed butterfly
__global__ void track_p2p_finish_kernel(int nblk, int H, int W, const double* __restrict__ partial, float fail_thr,
                                        const int32_t* __restrict__ valid_count, float* __restrict__ loss, int32_t* __restrict__ success,
                                        float* __restrict__ valid_ratio) {
    double x = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) x += partial[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if (threadIdx.x != 0) return;
    const float l = (float)(x / ((double)H * (double)W));
    loss[0] = l;
    success[0] = (l > fail_thr) ? 0 : 1;  // icp.py:455-457: only `loss > threshold` fails (a NaN loss passes)
    if (valid_ratio) valid_ratio[0] = ((float)valid_count[0] / (float)H) / (float)W;
}

int blocks_for(int n, int cap) { return max(1, min(cap, (n + TR_THREADS - 1) / TR_THREADS)); }

// level i of `levels` (coarsest first) pools by 2^(levels-1-i); blocks and pixel offsets packed in that order
TrackLevels make_levels(int H, int W, int levels) {
    TrackLevels py{};
    py.L = levels;
    int off = 0, blk = 0;
    for (int i = 0; i < levels; i++) {
        TrackLevel& lv = py.lv[i];
        lv.pool = 1 << (levels - 1 - i);
        lv.h = H / lv.pool, lv.w = W / lv.pool;
        lv.scale = 1.0f / (float)lv.pool;
        lv.off = off, lv.blk0 = blk, lv.nblk = blocks_for(lv.h * lv.w, TR_PYR_MAX_BLOCKS);
        off += lv.h * lv.w, blk += lv.nblk;
    }
    return py;
}

}  // namespace

static size_t dqo_track_preprocess_ws_bytes(int H, int W) {
    const size_t HW = (size_t)H * W;
    return dqo_align_up(HW * 4 * sizeof(float), 256) + 2 * sizeof(float) * TR_MAX_BLOCKS;
}

static int dqo_launch_track_preprocess(int H, int W, const float* depth, const float* K, float min_depth, float max_depth,
                                       float conf_thr, int filter, float* depth_out, float* vertex_out, float* normal_out, float* conf_out,
                                       uint8_t* invalid_out, void* ws, hipStream_t s) {
    const int HW = H * W;
    float* dws = (float*)ws;
    float* vws = dws + HW;
    float* partial = (float*)((char*)ws + dqo_align_up((size_t)HW * 4 * sizeof(float), 256));
    const int nblk = blocks_for(HW, TR_MAX_BLOCKS);
    DQO_LAUNCH("track_depth_kernel", track_depth_kernel, dim3(nblk), dim3(TR_THREADS), s, H, W, depth, filter, min_depth, max_depth, K, dws,
               vws, partial);
    DQO_LAUNCH("track_geometry_kernel", track_geometry_kernel, dim3(nblk), dim3(TR_THREADS), s, H, W, K, conf_thr, dws, vws,
               partial, nblk, depth_out, vertex_out, normal_out, conf_out, invalid_out);
    return DQO_OK;
}

static size_t dqo_track_pyramid_ws_bytes(void) { return 2 * sizeof(float) * TR_PYR_MAX_BLOCKS * TR_MAX_LEVELS; }

static int64_t dqo_track_pyramid_pixel_count(int H, int W, int levels) {
    int64_t n = 0;
    for (int i = 0; i < levels; i++) n += (int64_t)(H >> (levels - 1 - i)) * (W >> (levels - 1 - i));
    return n;
}

static int dqo_launch_track_pyramid(int H, int W, int levels, const float* depth, const float* K, float* vertex, float* normal,
                                    void* ws, hipStream_t s) {
    const TrackLevels py = make_levels(H, W, levels);
    const int nblk = py.lv[levels - 1].blk0 + py.lv[levels - 1].nblk;
    float* partial = (float*)ws;
    DQO_LAUNCH("track_pyr_vertex_kernel", track_pyr_vertex_kernel, dim3(nblk), dim3(TR_THREADS), s, W, depth, K, py, vertex, partial);
    DQO_LAUNCH("track_pyr_normal_kernel", track_pyr_normal_kernel, dim3(nblk), dim3(TR_THREADS), s, py, vertex, partial, normal);
    return DQO_OK;
}

static int dqo_launch_track_fill(int H, int W, float* render_depth, const float* frame_depth, const float* render_normal, const float* frame_normal,
                                 float dist_thr, float normal_thr, hipStream_t s) {
    const int HW = H * W;
    DQO_LAUNCH("track_fill_kernel", track_fill_kernel, dim3((HW + TR_THREADS - 1) / TR_THREADS), dim3(TR_THREADS), s, HW, render_depth,
               frame_depth, render_normal, frame_normal, dist_thr, normal_thr);
    return DQO_OK;
}

static size_t dqo_track_p2p_ws_bytes(void) { return sizeof(double) * TR_MAX_BLOCKS; }

static int dqo_launch_track_p2p(int H, int W, const float* vertex0, const float* vertex1, const float* normal0, const float* pose10, float fail_thr,
                                const int32_t* valid_count, float* loss, int32_t* success, float* valid_ratio, void* ws, hipStream_t s) {
    const int HW = H * W;
    const int nblk = blocks_for(HW, TR_MAX_BLOCKS);
    double* partial = (double*)ws;
    DQO_LAUNCH("track_p2p_partial_kernel", track_p2p_partial_kernel, dim3(nblk), dim3(TR_THREADS), s, HW, vertex0, vertex1, normal0, pose10,
               partial);
    DQO_LAUNCH("track_p2p_finish_kernel", track_p2p_finish_kernel, dim3(1), dim3(64), s, nblk, H, W, partial, fail_thr, valid_count, loss,
               success, valid_ratio);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// image sizes of the tracker entry points: positive, and H * W * 4 floats still indexable with int
static bool track_size_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W < (int64_t)0x7fffffff / 4; }

DQO_API size_t dqo_track_preprocess_workspace_bytes(int32_t H, int32_t W) {
    return track_size_ok(H, W) ? dqo_track_preprocess_ws_bytes(H, W) : 0;
}

DQO_API int dqo_track_preprocess(int32_t H, int32_t W, const float* depth, const float* K, float min_depth, float max_depth, float conf_thr,
                                 int32_t depth_filter, float* depth_out, float* vertex_out, float* normal_out, float* conf_out,
                                 uint8_t* invalid_out, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(depth && K && depth_out && vertex_out && normal_out && conf_out && invalid_out, "null pointer");
    DQO_CHECK_WS("track preprocess", ws, ws_bytes, dqo_track_preprocess_ws_bytes(H, W));
    return dqo_launch_track_preprocess(H, W, depth, K, min_depth, max_depth, conf_thr, depth_filter ? 1 : 0, depth_out, vertex_out,
                                       normal_out, conf_out, invalid_out, ws, (hipStream_t)stream);
}

DQO_API int64_t dqo_track_pyramid_pixels(int32_t H, int32_t W, int32_t levels) {
    if (!track_size_ok(H, W) || levels < 1 || levels > 4) return -1;
    return dqo_track_pyramid_pixel_count(H, W, levels);
}

DQO_API size_t dqo_track_pyramid_workspace_bytes(void) { return dqo_track_pyramid_ws_bytes(); }

DQO_API int dqo_track_pyramid(int32_t H, int32_t W, int32_t levels, const float* depth, const float* K, float* vertex, float* normal, void* ws,
                              size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(levels >= 1 && levels <= 4, "levels must be in [1, 4]");
    DQO_CHECK_ARG(track_size_ok(H, W) && (H >> (levels - 1)) > 0 && (W >> (levels - 1)) > 0, "bad image size for %d levels", levels);
    DQO_CHECK_ARG(depth && K && vertex && normal, "null pointer");
    DQO_CHECK_WS("track pyramid", ws, ws_bytes, dqo_track_pyramid_ws_bytes());
    return dqo_launch_track_pyramid(H, W, levels, depth, K, vertex, normal, ws, (hipStream_t)stream);
}

DQO_API int dqo_track_fill_model_depth(int32_t H, int32_t W, float* render_depth, const float* frame_depth, const float* render_normal,
                                       const float* frame_normal, float dist_thr, float normal_thr, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(render_depth && frame_depth && render_normal && frame_normal, "null pointer");
    return dqo_launch_track_fill(H, W, render_depth, frame_depth, render_normal, frame_normal, dist_thr, normal_thr, (hipStream_t)stream);
}

DQO_API size_t dqo_track_p2p_workspace_bytes(void) { return dqo_track_p2p_ws_bytes(); }

DQO_API int dqo_track_p2p_loss(int32_t H, int32_t W, const float* vertex0, const float* vertex1, const float* normal0, const float* pose10,
                               float fail_thr, const int32_t* valid_count, float* loss, int32_t* success, float* valid_ratio, void* ws,
                               size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(track_size_ok(H, W), "bad image size");
    DQO_CHECK_ARG(vertex0 && vertex1 && normal0 && pose10 && loss && success, "null pointer");
    DQO_CHECK_ARG((valid_count == nullptr) == (valid_ratio == nullptr), "valid_count and valid_ratio go together");
    DQO_CHECK_WS("track p2p", ws, ws_bytes, dqo_track_p2p_ws_bytes());
    return dqo_launch_track_p2p(H, W, vertex0, vertex1, normal0, pose10, fail_thr, valid_count, loss, success, valid_ratio, ws,
                                (hipStream_t)stream);
}

}  // extern "C"
