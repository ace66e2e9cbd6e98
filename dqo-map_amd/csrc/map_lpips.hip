// LPIPS of a rendered frame for gfx950: the "lpips" number eval_picture reports (SLAM/eval.py:28-30, :65-68 —
// LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True) of the clamped images), on weights the caller brings, nothing
// read back.  include/dqo_raster.h states the four steps (dqo_eval_lpips); tests/lpips_oracle.py restates them.  Neither `lpips` nor
// `torchmetrics` exists on this platform: the kernels follow the published sources and are held to that restatement.
//
// Launches: TWELVE per call — C0 P0 C1 P1 C2 C3 C4, then the five heads H0 .. H4.
//
// lpips_conv_kernel: one template for the five convolutions, an implicit GEMM on v_mfma_f32_32x32x2_f32.  M = the output pixels of BOTH
// images (one launch per layer reads every weight once), N = Cout, K = the taps in the packed order k = (kh * KW + kw) * Cin + ci.  A
// 256-thread block owns a 64 x 64 tile of the output (pixels x channels; 128 x 64 in layers 3 and 4), each of its four waves a 32 x 32
// quarter (two there, one above the other) in an accumulator tile of its own (16 registers):
// the f32 MFMA is bit for bit fmaf(a_k, b_k, acc) in ascending k, so an output element is the serial chain the header promises — there
// is no split-K and no two accumulators to add.  K goes by chunks of BK taps: the A chunk (64 pixels x BK taps) is gathered from the
// previous map and the B chunk (BK taps x 64 channels) from the packed weights into registers while the MFMAs of the chunk before run
// out of LDS (k-major, pitch 68 dwords: a half-wave's 32 operand reads are 32 consecutive dwords).  Every Cin behind layer 0 is a
// multiple of 32, so a chunk lies inside one tap and a thread's part of it is one or two float4 of the pixel-major map.  Layer 0
// gathers element by element from the two [3,H,W] images, step 1 folded into the load; its K = 363 ends inside a chunk: the tail's a
// and b are zeros, and fmaf(0, 0, acc) is acc.  Rows beyond M are gathered as zeros and not stored.  Epilogue: + bias, ReLU,
// pixel-major [2][h][w][Cout] — what the next layer's gather and the head's channel walk read contiguously.
// The tile and the chunks (profiles/lpips_1200x680.txt): BK = 16 in layer 0 and 32 behind it is measured — 32 is 4.5-7.5 % faster in
// layers 1..4 (twice the MFMAs between two barriers), 3 % slower in layer 0 (K pads to 384 instead of 368).  The tile is measured too:
// 128 x 64 is 13-21 % slower than 64 x 64 in layers 0..2 (half the blocks, fewer waves to hide the gather) and 4-5 % faster in layers 3
// and 4, whose 6 068 rows at 1200 x 680 are 95 x 4 = 380 blocks of 64 x 64 on 256 CUs — 124 CUs with two, 132 with one — but 192 of
// 128 x 64, one per CU.
//
// lpips_pool_kernel: maxpool 3/2 as a kernel of its own, one thread per float4 of the pooled map, rather than inside the next layer's
// gather: layer 1 reads every pooled pixel for 25 taps and layer 2 for 9, so a fused pool would form each maximum that many times.
//
// lpips_head_kernel: steps 3 and 4 of one layer.  A group of lanes owns a pixel at a time: its lanes form the channels' terms side by
// side into LDS, in double — the two squares, then lin_c (na_c - nb_c)^2 — and the group's first lanes add them up in ascending channel
// order, so every sum is the serial chain of the statement.  The block's sum goes to a partial (dqo_reduce.h), the launch's last block
// folds the partials in block order, forms the layer's mean and writes its slot; layer 4's also adds the five means and writes slots 0,
// 6 and 7.  No float atomics, no zero fill, the ticket words handed back at zero: two calls give the same bytes, and a call is
// capturable in a hipGraph.
#include <algorithm>

#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

enum {
    LP_LAYERS = 5,
    LP_BN = 64,      // output channels of a block's tile
    LP_HEAD_BLOCKS = 256,  // the most blocks of a head's launch: its last block adds their partials one after the other
    LP_PITCH = 68,   // dwords per k row of the B chunk in LDS (a multiple of 4: the rows are stored as float4)
    LP_STRIDE = 8,   // doubles per block partial: one 64-byte line
    LP_STAGE = 64,   // partials staged through LDS at a time by the last block
    LP_SLOTS = 8,
};

struct LpLayer {
    int cin, cout, ks, stride, pad;
};
constexpr LpLayer LP_NET[LP_LAYERS] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};

// float offsets into the packed weights (include/dqo_raster.h lists them)
struct LpWeights {
    size_t w[LP_LAYERS], bias[LP_LAYERS], lin[LP_LAYERS], total;
};
inline LpWeights lp_weights() {
    LpWeights o;
    size_t p = 0;
    for (int l = 0; l < LP_LAYERS; l++) {
        const LpLayer& L = LP_NET[l];
        o.w[l] = p, p += (size_t)L.cin * L.ks * L.ks * L.cout;
        o.bias[l] = p, p += L.cout;
        o.lin[l] = p, p += L.cout;
    }
    o.total = p;
    return o;
}

struct LpWorkspace {
    int32_t* ticket;
    double* means;            // [LP_LAYERS] (8 doubles' room)
    float* feat[LP_LAYERS];   // f_l: [2][h_l][w_l][Cout_l]
    float* pooled[2];         // maxpool3/2 of f_0, f_1: [2][h_{l+1}][w_{l+1}][Cout_l]
    double* partial;          // [LP_HEAD_BLOCKS][LP_STRIDE]
    int h[LP_LAYERS], w[LP_LAYERS];
    size_t total;
};

inline LpWorkspace lp_ws(void* base, int W, int H) {
    LpWorkspace k;
    DqoCarver c(base);
    k.ticket = c.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    k.means = c.take<double>(256);  // = DQO_LPIPS_FEATURES_OFFSET
    k.h[0] = (H - 7) / 4 + 1, k.w[0] = (W - 7) / 4 + 1;
    k.h[1] = (k.h[0] - 3) / 2 + 1, k.w[1] = (k.w[0] - 3) / 2 + 1;
    k.h[2] = k.h[3] = k.h[4] = (k.h[1] - 3) / 2 + 1, k.w[2] = k.w[3] = k.w[4] = (k.w[1] - 3) / 2 + 1;
    for (int l = 0; l < LP_LAYERS; l++) k.feat[l] = c.take<float>(sizeof(float) * 2 * (size_t)k.h[l] * k.w[l] * LP_NET[l].cout);
    for (int l = 0; l < 2; l++) k.pooled[l] = c.take<float>(sizeof(float) * 2 * (size_t)k.h[l + 1] * k.w[l + 1] * LP_NET[l].cout);
    k.partial = c.take<double>((size_t)LP_HEAD_BLOCKS * LP_STRIDE * sizeof(double));
    k.total = c.total();
    return k;
}
static_assert(DQO_REDUCE_HEAD_WORDS * 4 + 256 == DQO_LPIPS_FEATURES_OFFSET, "the feature maps' place in the workspace is part of the public header");

// step 1 of a loaded colour value of channel c: one float rounding per statement (the file is compiled without contraction)
__device__ __forceinline__ float lp_scale_input(float x, int c) {
    x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);  // (a NaN fails both tests and stays)
    x = 2.f * x;
    x = x - 1.f;
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    x = x - shift;
    return x / scale;
}

// One convolution.  src0: the previous map [2][ih][iw][CIN] (FIRST: the first image's [3][ih iw] planes, src1 the second's).
// grid (ceil(2 oh ow / BM), COUT / 64).  BM: the pixels of a block's tile, 64 or 128 (a wave then owns two 32 x 32 quarters, one above
// the other, each in an accumulator tile of its own); BK: the taps of a chunk, 16 or 32.
template <int CIN, int KS, int STRIDE, int PAD, int COUT, bool FIRST, int BM, int BK>
__global__ __launch_bounds__(256) void lpips_conv_kernel(const float* __restrict__ src0, const float* __restrict__ src1, int ih, int iw, int oh,
                                                         int ow, const float* __restrict__ wgt, const float* __restrict__ bias,
                                                         float* __restrict__ dst) {
    constexpr int K = CIN * KS * KS, CHUNKS = (K + BK - 1) / BK;
    constexpr int TPR = 256 / BM;              // threads that share a row of the A chunk
    constexpr int NA = BK / TPR, NB = BK / 16;  // floats of A and float4s of B a thread gathers per chunk
    constexpr int MI = BM / 64, PA = BM + 4;    // accumulator tiles of a wave; dwords per k row of the A chunk in LDS
    static_assert((BM == 64 || BM == 128) && (BK == 16 || BK == 32), "the gather's thread maps");
    static_assert(FIRST || CIN % BK == 0, "a chunk lies inside one tap");
    static_assert(COUT % LP_BN == 0, "no column tail");
    __shared__ __attribute__((aligned(16))) float s_a[BK * PA];
    __shared__ __attribute__((aligned(16))) float s_b[BK * LP_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int npix = oh * ow, M = 2 * npix;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * LP_BN;
    // the A row this thread gathers: FIRST — row tid % BM, taps tid / BM + TPR j of the chunk; else row tid / TPR, taps NA (tid % TPR) + j
    const int ar = FIRST ? (tid % BM) : (tid / TPR), aq = FIRST ? (tid / BM) : (tid % TPR);
    const int am = m0 + ar;
    const bool a_row = am < M;
    const int a_img = a_row ? am / npix : 0, a_p = a_row ? am - a_img * npix : 0;
    const int a_oy = a_p / ow, a_ox = a_p - a_oy * ow;
    const int a_y0 = a_oy * STRIDE - PAD, a_x0 = a_ox * STRIDE - PAD;
    // the B rows: taps tid / 16 + 16 j of the chunk, channels 4 (tid % 16) ..
    const int bk = tid >> 4, bc = (tid & 15) * 4;

    float ra[NA];
    float4 rb[NB];
    auto gather = [&](int chunk) {
        const int k0 = chunk * BK;
        if constexpr (FIRST) {
            const float* __restrict__ img = a_img ? src1 : src0;
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const int k = k0 + aq + TPR * j;
                const int tap = k / CIN, ci = k - tap * CIN, kh = tap / KS, kw = tap - kh * KS;
                const int iy = a_y0 + kh, ix = a_x0 + kw;
                const bool in = a_row && k < K && iy >= 0 && iy < ih && ix >= 0 && ix < iw;
                ra[j] = in ? lp_scale_input(img[((size_t)ci * ih + iy) * iw + ix], ci) : 0.f;
            }
        } else {
            const int tap = k0 / CIN, ci = k0 - tap * CIN + NA * aq, kh = tap / KS, kw = tap - kh * KS;
            const int iy = a_y0 + kh, ix = a_x0 + kw;
            const bool in = a_row && iy >= 0 && iy < ih && ix >= 0 && ix < iw;
            const float4* __restrict__ p = reinterpret_cast<const float4*>(src0 + (((size_t)a_img * ih + iy) * iw + ix) * CIN + ci);
#pragma unroll
            for (int j = 0; j < NA / 4; j++) {
                const float4 v = in ? p[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                ra[4 * j] = v.x, ra[4 * j + 1] = v.y, ra[4 * j + 2] = v.z, ra[4 * j + 3] = v.w;
            }
        }
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int k = k0 + bk + 16 * j;
            rb[j] = k < K ? *reinterpret_cast<const float4*>(wgt + (size_t)k * COUT + n0 + bc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    lp_f32x16 acc[MI];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
    gather(0);
    const int half = lane >> 5, l32 = lane & 31;
    for (int chunk = 0; chunk < CHUNKS; chunk++) {
#pragma unroll
        for (int j = 0; j < NA; j++) s_a[(FIRST ? aq + TPR * j : NA * aq + j) * PA + ar] = ra[j];
#pragma unroll
        for (int j = 0; j < NB; j++) *reinterpret_cast<float4*>(&s_b[(bk + 16 * j) * LP_PITCH + bc]) = rb[j];
        __syncthreads();
        if (chunk + 1 < CHUNKS) gather(chunk + 1);  // (in flight under the MFMAs below)
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++) {
            // lane l holds A[i = l % 32][k = l / 32] and B[k = l / 32][j = l % 32]; the instruction adds k = 0, then k = 1
            const float b = s_b[(2 * kk + half) * LP_PITCH + wn * 32 + l32];
#pragma unroll
            for (int i = 0; i < MI; i++) {
                const float a = s_a[(2 * kk + half) * PA + wm * (BM / 2) + 32 * i + l32];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D of the 32 x 32 forms: column = lane % 32, row = (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
    const int n = n0 + wn * 32 + l32;
    const float bn = bias[n];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + wm * (BM / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m < M) {
                const float v = acc[i][r] + bn;
                dst[(size_t)m * COUT + n] = v < 0.f ? 0.f : v;  // (a NaN stays, as torch's relu leaves it)
            }
        }
}

// dst [2][oh][ow][C] = max_pool2d(src [2][ih][iw][C], 3, 2): floor mode, no padding; a NaN wins, as in torch.  One thread per float4.
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ src, int ih, int iw, int oh, int ow, int C4,
                                                         float* __restrict__ dst) {
    const size_t n = (size_t)2 * oh * ow * C4, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c4 = (int)(i % C4);
    const size_t pix = i / C4;
    const int ox = (int)(pix % ow), oy = (int)((pix / ow) % oh), img = (int)(pix / ((size_t)ow * oh));
    const float4* __restrict__ s = reinterpret_cast<const float4*>(src) + (((size_t)img * ih + 2 * oy) * iw + 2 * ox) * C4 + c4;  // (2 oy + 2 <= ih - 1)
    float4 m = s[0];
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const float4 v = s[((size_t)dy * iw + dx) * C4];
            m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x, m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
            m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z, m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
        }
    reinterpret_cast<float4*>(dst)[i] = m;
}

// t[0] + t[1] + .. + t[C - 1] in that order (C a multiple of 8; eight loads in flight ahead of the chain of adds)
__device__ __forceinline__ double lp_serial_sum(const double* t, int C) {
    double sum = 0.0;
    for (int c = 0; c < C; c += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = t[c + j];
#pragma unroll
        for (int j = 0; j < 8; j++) sum += v[j];
    }
    return sum;
}

// Steps 3 and 4 of layer `layer`: feat [2][npix][C].  A group of G lanes owns a pixel at a time (256 / G pixels a round, the block's
// rounds LP_HEAD_BLOCKS * 256 / G pixels apart): its lanes form the channels' terms side by side into LDS — the squares, then
// lin_c (na_c - nb_c)^2 — and the group's first lanes add them up in ascending channel order, so every sum is the serial chain of the
// statement.  CMAX: the most channels the LDS holds.
template <int G, int CMAX>
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ feat, int npix, int C, const float* __restrict__ lin, int mode,
                                                         int layer, int32_t* ticket, double* partial, double* means,
                                                         const DqoRastHeader* __restrict__ header, float* __restrict__ out) {
    constexpr int GROUPS = 256 / G;
    __shared__ double s_t[GROUPS][2][CMAX + 2];  // (+ 2: the groups' serial readers walk their rows in step, on banks of their own)
    __shared__ double s_stage[LP_STAGE * LP_STRIDE];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, g = tid / G, gl = tid % G;
    double a[1] = {0.0};
    for (int base = (int)blockIdx.x * GROUPS; base < npix; base += (int)gridDim.x * GROUPS) {  // (the same trips for the whole block)
        const int p = base + g;
        const bool live = p < npix;
        const float* __restrict__ fa = feat + (size_t)(live ? p : 0) * C;
        const float* __restrict__ fb = feat + ((size_t)npix + (live ? p : 0)) * C;
        for (int c = gl; c < C; c += G) {
            const double x = (double)fa[c], y = (double)fb[c];
            s_t[g][0][c] = x * x, s_t[g][1][c] = y * y;
        }
        __syncthreads();
        double sum = 0.0;
        if (gl < 2) sum = lp_serial_sum(s_t[g][gl], C);
        const double den = mode == DQO_LPIPS_NORM_LPIPS ? sqrt(sum) + 1e-10 : sqrt(1e-8 + sum);
        const double da = __shfl(den, (lane / G) * G), db = __shfl(den, (lane / G) * G + 1);
        __syncthreads();
        for (int c = gl; c < C; c += G) {
            const double d = (double)fa[c] / da - (double)fb[c] / db;
            s_t[g][0][c] = (double)lin[c] * (d * d);
        }
        __syncthreads();
        if (gl == 0 && live) a[0] += lp_serial_sum(s_t[g][0], C);
        __syncthreads();
    }
    dqo_block_partial<1, LP_STRIDE>(a, s_stage, partial);
    if (!dqo_last_block(ticket, &s_last)) return;
    const double total = dqo_fold_partials<1, LP_STRIDE, LP_STAGE>(partial, 0, (int)gridDim.x, s_stage);
    if (tid != 0) return;
    const double d = total / (double)npix;
    means[layer] = d;
    out[1 + layer] = (float)d;
    if (layer != LP_LAYERS - 1) return;
    const float nan = __int_as_float(0x7fc00000);
    if (header != nullptr && header->overflow != 0u) {  // the render outgrew its context: its images are invalid, and so is the row
#pragma unroll
        for (int q = 0; q < LP_SLOTS; q++) out[q] = nan;
        return;
    }
    // (the earlier layers' means were left by earlier launches of this call)
    out[0] = (float)((((means[0] + means[1]) + means[2]) + means[3]) + d);
    out[6] = nan, out[7] = nan;
}

template <int L, bool FIRST, int BM, int BK>
int lp_conv(const char* name, const float* src0, const float* src1, int ih, int iw, int oh, int ow, const float* weights, float* dst, hipStream_t s) {
    constexpr LpLayer N = LP_NET[L];
    const LpWeights o = lp_weights();
    const int64_t M = (int64_t)2 * oh * ow;
    auto kernel = lpips_conv_kernel<N.cin, N.ks, N.stride, N.pad, N.cout, FIRST, BM, BK>;
    DQO_LAUNCH(name, kernel, dim3((unsigned)((M + BM - 1) / BM), (unsigned)(N.cout / LP_BN)), dim3(256), s, src0, src1, ih, iw, oh, ow,
               weights + o.w[L], weights + o.bias[L], dst);
    return DQO_OK;
}

int lp_pool(const char* name, const float* src, int ih, int iw, int oh, int ow, int C, float* dst, hipStream_t s) {
    const size_t n = (size_t)2 * oh * ow * (C / 4);
    DQO_LAUNCH(name, lpips_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), s, src, ih, iw, oh, ow, C / 4, dst);
    return DQO_OK;
}

}  // namespace

// The pixels of a tile and the taps of a chunk, per layer (see the head comment; a build may override them to repeat the measurement)
#ifndef LP_BM0
#define LP_BM0 64
#endif
#ifndef LP_BM1
#define LP_BM1 64
#endif
#ifndef LP_BM2
#define LP_BM2 64
#endif
#ifndef LP_BM3
#define LP_BM3 128
#endif
#ifndef LP_BM4
#define LP_BM4 128
#endif
#ifndef LP_BK0
#define LP_BK0 16
#endif
#ifndef LP_BK1
#define LP_BK1 32
#endif
#ifndef LP_BK2
#define LP_BK2 32
#endif
#ifndef LP_BK3
#define LP_BK3 32
#endif
#ifndef LP_BK4
#define LP_BK4 32
#endif

#define LP_TRY(expr)                      \
    do {                                  \
        const int rc_ = (expr);           \
        if (rc_ != DQO_OK) return rc_;    \
    } while (0)

static int dqo_launch_lpips(int W, int H, const float* image, const float* gt, const float* weights, int mode, const DqoRastHeader* header,
                            float* out_row, void* ws, hipStream_t s) {
    const LpWorkspace k = lp_ws(ws, W, H);
    const LpWeights o = lp_weights();
    LP_TRY((lp_conv<0, true, LP_BM0, LP_BK0>("lpips_conv0", image, gt, H, W, k.h[0], k.w[0], weights, k.feat[0], s)));
    LP_TRY(lp_pool("lpips_pool0", k.feat[0], k.h[0], k.w[0], k.h[1], k.w[1], LP_NET[0].cout, k.pooled[0], s));
    LP_TRY((lp_conv<1, false, LP_BM1, LP_BK1>("lpips_conv1", k.pooled[0], nullptr, k.h[1], k.w[1], k.h[1], k.w[1], weights, k.feat[1], s)));
    LP_TRY(lp_pool("lpips_pool1", k.feat[1], k.h[1], k.w[1], k.h[2], k.w[2], LP_NET[1].cout, k.pooled[1], s));
    LP_TRY((lp_conv<2, false, LP_BM2, LP_BK2>("lpips_conv2", k.pooled[1], nullptr, k.h[2], k.w[2], k.h[2], k.w[2], weights, k.feat[2], s)));
    LP_TRY((lp_conv<3, false, LP_BM3, LP_BK3>("lpips_conv3", k.feat[2], nullptr, k.h[2], k.w[2], k.h[2], k.w[2], weights, k.feat[3], s)));
    LP_TRY((lp_conv<4, false, LP_BM4, LP_BK4>("lpips_conv4", k.feat[3], nullptr, k.h[2], k.w[2], k.h[2], k.w[2], weights, k.feat[4], s)));
    static const char* const head_names[LP_LAYERS] = {"lpips_head0", "lpips_head1", "lpips_head2", "lpips_head3", "lpips_head4"};
    for (int l = 0; l < LP_LAYERS; l++) {
        const int npix = k.h[l] * k.w[l], C = LP_NET[l].cout;
        // as many pixels a round as the LDS holds rows for: 32 at layer 0 (eight lanes a pixel), 16 at layer 1, 8 behind
        const int groups = l == 0 ? 32 : (l == 1 ? 16 : 8);
        const unsigned blocks = (unsigned)std::min<int64_t>(LP_HEAD_BLOCKS, ((int64_t)npix + groups - 1) / groups);
        auto kernel = l == 0 ? lpips_head_kernel<8, 64> : (l == 1 ? lpips_head_kernel<16, 192> : lpips_head_kernel<32, 384>);
        DQO_LAUNCH(head_names[l], kernel, dim3(blocks), dim3(256), s, k.feat[l], npix, C, weights + o.lin[l], mode, l, k.ticket, k.partial, k.means,
                   header, out_row);
    }
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// every map needs a pixel: both sides >= 31; W * H within dqo_eval_picture's limit
static bool lpips_size_ok(int32_t W, int32_t H) { return W >= 31 && H >= 31 && (int64_t)W * H < (1ll << 31) / 3; }

DQO_API size_t dqo_eval_lpips_weight_floats(int32_t layer) {
    const LpWeights o = lp_weights();
    if (layer < 0 || layer >= LP_LAYERS) return o.total;
    return (layer + 1 < LP_LAYERS ? o.w[layer + 1] : o.total) - o.w[layer];
}

DQO_API size_t dqo_eval_lpips_workspace_bytes(int32_t W, int32_t H) { return lpips_size_ok(W, H) ? lp_ws(nullptr, W, H).total : 0; }

DQO_API int dqo_eval_lpips(int32_t W, int32_t H, const float* image, const float* gt, const float* weights, int32_t norm_mode,
                           const DqoRastHeader* render_header, float* out, int32_t row, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(lpips_size_ok(W, H), "bad image size %d x %d: LPIPS needs both sides >= 31 (every AlexNet map needs a pixel)", W, H);
    DQO_CHECK_ARG(image && gt && weights && out, "null pointer");
    DQO_CHECK_ARG(((uintptr_t)weights & 15) == 0, "weights must be 16-byte aligned");
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    DQO_CHECK_ARG(norm_mode == DQO_LPIPS_NORM_TORCHMETRICS || norm_mode == DQO_LPIPS_NORM_LPIPS, "unknown norm_mode %d", norm_mode);
    DQO_CHECK_WS("lpips", ws, ws_bytes, dqo_eval_lpips_workspace_bytes(W, H));
    return dqo_launch_lpips(W, H, image, gt, weights, norm_mode, render_header, out + (size_t)LP_SLOTS * row, ws, (hipStream_t)stream);
}

}  // extern "C"
