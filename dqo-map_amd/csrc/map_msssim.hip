// MS-SSIM of a rendered frame for gfx950: the "ssim" number eval_picture reports (SLAM/eval.py:19-25, :64 —
// pytorch_msssim.ms_ssim(image[None], gt[None], data_range=1.0, size_average=True)), nothing read back.
//
// Five levels.  A level filters both images, their squares and their product with the separable 11-tap window of utils/loss_utils.py:41-58
// (dqo_ssim_window: the mapping loss's, bit for bit) as a VALID correlation — no padding, [h,w] -> [h-10,w-10] — and takes, per channel,
// the means of
//     cs = (2 s12 + C2) / (s1 + s2 + C2)                               s1 = f(X X) - mu1^2,  s2 = f(Y Y) - mu2^2,  s12 = f(X Y) - mu1 mu2
//     ss = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) * cs              mu1 = f(X),  mu2 = f(Y),  C1 = 0.01^2,  C2 = 0.03^2
// Between levels both images are replaced by avg_pool2d(kernel_size = 2, padding = (h % 2, w % 2)): an odd side shifts the 2 x 2 grid by one
// and puts a zero into the first row / column, the divisor is always 4.  The value: per channel the product over the levels of
// max(mean, 0) ** weight — the cs mean at levels 0..3, the ss mean at level 4 — and the mean of the three channels.
//
// Launches: NINE per call, level kernel and pool kernel in turn (L0 P1 L1 P2 L2 P3 L3 P4 L4).  The pooled levels 1..4 are materialised in
// the workspace by a pool kernel of their own — one thread per output pixel, ((top-left + top-right) + bottom-left) + bottom-right, then
// * 0.25f — rather than by a pool fused into the next level's load: the halo tiles of a level overlap, so a fused pool would form every
// pooled pixel up to 2.6 times or need an owner rule for the write, to save four launches of a few microseconds.
//
// msssim_level_kernel: a 256-thread block owns a run of 16 x 16 tiles of one channel's filtered grid (ms_level: one tile at the small
// levels); per tile it stages the 26 x 26 halo tile of both images in LDS and forms the five window sums in one horizontal and one vertical sweep (two barriers), float32 as the reference's library.
// LDS layout (ds_read_b32 / ds_write_b32 bank = dword address mod 32, conflicts inside a 32-lane half): a half is two rows of sixteen
// columns in both sweeps, so a row pitch of 16 mod 32 dwords makes its 32 addresses 32 banks — 48 for the halo tiles (26 columns
// used), 16 for the horizontal sums.  17.9 KB + 4 KB of reduction stage per block: the LDS admits seven blocks per CU, the registers
// (84 VGPRs) five waves per SIMD — more than the four blocks a CU is meant to hold either way.
// cs and ss of a pixel are formed one float32 rounding per statement (never contracted: identical images then give numerator ==
// denominator bit for bit, cs = ss = 1.0f, as in the reference) and added into DOUBLE sums through dqo_reduce.h: lanes by the xor
// butterfly, the block's waves in order, the launch's last block folds the partials of each channel in block-index order and leaves
// the level's six means in the workspace.  Level 4's last block forms the 15 factors, the three products of powers and their mean in
// double, rounds each once to float32 and writes the row.  No float atomics, no zero fill, the ticket words handed back at zero: two
// calls give the same bytes, and a call is capturable in a hipGraph.
#include <algorithm>

#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

enum {
    MS_T = 16,              // tile of the filtered grid
    MS_IN = MS_T + 10,      // halo tile (valid correlation: the window reaches ten inputs beyond the tile's last output)
    MS_PITCH = 48,          // dwords per halo row in LDS (16 mod 32: see above)
    MS_LEVELS = 5,
    MS_BLOCKS = 512,        // blocks of a level's launch, about (ms_level)
    MS_SUMS = 2,            // cs | ss
    MS_STRIDE = 8,          // doubles per block partial: one 64-byte line
    MS_STAGE = 64,          // partials staged through LDS at a time by the last block
    MS_MEANS = 8,           // doubles per level in the workspace: cs r, ss r, cs g, ss g, cs b, ss b, -, -
    MS_SLOTS = 20,
};

struct MsWorkspace {
    int32_t* ticket;
    double* means;    // [MS_LEVELS][MS_MEANS]
    double* partial;  // [blocks of the level with the most][MS_STRIDE]
    float* pooled[MS_LEVELS];  // level l >= 1: [2][3][h_l w_l] (render planes, then target planes)
    size_t total;
};

inline int ms_next(int s) { return s / 2 + s % 2; }

// A level's launch.  The last block adds the blocks' partials one after the other, about 40 ns each (one tile per block at 1200 x 680:
// 12 800 partials over the five levels, 497 us of 524 us per call were that sum).  So a block takes `run` tiles side by side, sized for
// about MS_BLOCKS blocks per level — two per CU; the sums of its tiles stay in the threads' registers.
struct MsLevel {
    int tiles_x, run, groups_x, groups, blocks;
};
inline MsLevel ms_level(int w, int h) {
    MsLevel L;
    L.tiles_x = (w - 10 + MS_T - 1) / MS_T;
    const int tiles_y = (h - 10 + MS_T - 1) / MS_T;
    const int64_t tiles3 = (int64_t)3 * L.tiles_x * tiles_y;
    L.run = (int)std::min<int64_t>(L.tiles_x, std::max<int64_t>(1, (tiles3 + MS_BLOCKS - 1) / MS_BLOCKS));
    L.groups_x = (L.tiles_x + L.run - 1) / L.run;
    L.groups = L.groups_x * tiles_y;
    L.blocks = 3 * L.groups;
    return L;
}

inline MsWorkspace ms_ws(void* base, int W, int H) {
    MsWorkspace w;
    DqoCarver k(base);
    w.ticket = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.means = k.take<double>(MS_LEVELS * MS_MEANS * sizeof(double));
    int blocks = 0, lw = W, lh = H;
    for (int l = 0; l < MS_LEVELS; l++, lw = ms_next(lw), lh = ms_next(lh)) blocks = std::max(blocks, ms_level(lw, lh).blocks);
    w.partial = k.take<double>((size_t)blocks * MS_STRIDE * sizeof(double));
    w.pooled[0] = nullptr;
    lw = W, lh = H;
    for (int l = 1; l < MS_LEVELS; l++) {
        lw = ms_next(lw), lh = ms_next(lh);
        w.pooled[l] = k.take<float>(sizeof(float) * 6 * (size_t)lw * lh);
    }
    w.total = k.total();
    return w;
}

// dst [2][3][oh ow] = avg_pool2d(src, 2, padding = (h % 2, w % 2)), count_include_pad: output (oy, ox) averages rows 2 oy - h % 2, + 1 and
// columns 2 ox - w % 2, + 1; index -1 is a zero.  blockIdx.y: the plane (0..2 of src_x, 3..5 of src_y).
__global__ __launch_bounds__(256) void msssim_pool_kernel(int w, int h, const float* __restrict__ src_x, const float* __restrict__ src_y,
                                                          int ow, int oh, float* __restrict__ dst) {
    const size_t on = (size_t)ow * oh, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= on) return;
    const int plane = blockIdx.y;
    const float* __restrict__ src = (plane < 3 ? src_x + (size_t)plane * w * h : src_y + (size_t)(plane - 3) * w * h);
    const int oy = (int)(i / ow), ox = (int)(i - (size_t)oy * ow);
    const int iy = 2 * oy - (h & 1), ix = 2 * ox - (w & 1);  // (iy + 1 <= h - 1 and ix + 1 <= w - 1 for every output: oh = h / 2 + h % 2)
    const float* r1 = src + (size_t)(iy + 1) * w + (ix + 1);  // the window's bottom-right input: always inside
    const float a00 = (iy >= 0 && ix >= 0) ? r1[-w - 1] : 0.f, a01 = iy >= 0 ? r1[-w] : 0.f, a10 = ix >= 0 ? r1[-1] : 0.f, a11 = r1[0];
    dst[(size_t)plane * on + i] = (((a00 + a01) + a10) + a11) * 0.25f;
}

// cs and ss of a filtered pixel, one float32 rounding per statement
__device__ __forceinline__ void ms_pixel(float mu1, float mu2, float e11, float e22, float e12, float& cs, float& ss) {
#pragma clang fp contract(off)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = e11 - mu1s, s2 = e22 - mu2s, s12 = e12 - mu12;
    const float two_s12 = 2.f * s12, two_mu12 = 2.f * mu12;
    const float s_sum = s1 + s2, mu_sum = mu1s + mu2s;
    cs = (two_s12 + C2) / (s_sum + C2);
    const float lum = (two_mu12 + C1) / (mu_sum + C1);
    ss = lum * cs;
}

// One level: x, y [3][h w] planes.  Block b: channel b / groups, group b % groups of the channel's filtered grid, row-major; a group is
// `run` tiles side by side (the last of a tile row may be shorter), taken left to right.
__global__ __launch_bounds__(256) void msssim_level_kernel(int w, int h, const float* __restrict__ x, const float* __restrict__ y,
                                                           DqoSsimWindow win, int level, int tiles_x, int run, int groups_x, int groups,
                                                           int32_t* ticket, double* partial, double* means,
                                                           const DqoRastHeader* __restrict__ header, float* __restrict__ out) {
    __shared__ float s_a[MS_IN][MS_PITCH], s_b[MS_IN][MS_PITCH];
    __shared__ float s_h5[5][MS_IN][MS_T];  // horizontal sums of x, y, x^2, y^2, x y
    __shared__ double s_stage[MS_STAGE * MS_STRIDE];
    __shared__ double s_mean[6];
    __shared__ int s_last;
    const int tid = threadIdx.x, tx = tid & (MS_T - 1), ty = tid / MS_T;
    const int ch = (int)blockIdx.x / groups, g = (int)blockIdx.x - ch * groups;
    const int y0 = (g / groups_x) * MS_T, t0 = (g % groups_x) * run, t1 = min(t0 + run, tiles_x);
    const float* __restrict__ px = x + (size_t)ch * w * h;
    const float* __restrict__ py = y + (size_t)ch * w * h;
    double a[MS_SUMS] = {0.0, 0.0};
    // (no barrier closes a round: the next round's loads overwrite s_a / s_b, last read before this round's second barrier, and its
    // horizontal sweep writes s_h5 behind its own first barrier, which every thread reaches after its vertical sweep)
    for (int t = t0; t < t1; t++) {
        const int x0 = t * MS_T;
        for (int i = tid; i < MS_IN * MS_IN; i += 256) {  // (beyond the image: zeros, which only outputs beyond the filtered grid read)
            const int r = i / MS_IN, c = i - r * MS_IN;
            const int gx = x0 + c, gy = y0 + r;
            const bool in = gx < w && gy < h;
            s_a[r][c] = in ? px[(size_t)gy * w + gx] : 0.f;
            s_b[r][c] = in ? py[(size_t)gy * w + gx] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < MS_IN * MS_T; i += 256) {
            const int r = i / MS_T, c = i - r * MS_T;
            float h1 = 0.f, h2 = 0.f, h11 = 0.f, h22 = 0.f, h12 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float u = s_a[r][c + k], v = s_b[r][c + k], wk = win.g[k];
                h1 += wk * u, h2 += wk * v, h11 += wk * (u * u), h22 += wk * (v * v), h12 += wk * (u * v);
            }
            s_h5[0][r][c] = h1, s_h5[1][r][c] = h2, s_h5[2][r][c] = h11, s_h5[3][r][c] = h22, s_h5[4][r][c] = h12;
        }
        __syncthreads();
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float wk = win.g[k];
            mu1 += wk * s_h5[0][ty + k][tx], mu2 += wk * s_h5[1][ty + k][tx], e11 += wk * s_h5[2][ty + k][tx],
                e22 += wk * s_h5[3][ty + k][tx], e12 += wk * s_h5[4][ty + k][tx];
        }
        if (x0 + tx < w - 10 && y0 + ty < h - 10) {
            float cs, ss;
            ms_pixel(mu1, mu2, e11, e22, e12, cs, ss);
            a[0] += (double)cs, a[1] += (double)ss;
        }
    }
    dqo_block_partial<MS_SUMS, MS_STRIDE>(a, s_stage, partial);
    if (!dqo_last_block(ticket, &s_last)) return;
    const double n = (double)(w - 10) * (double)(h - 10);
    for (int c = 0; c < 3; c++) {
        const double total = dqo_fold_partials<MS_SUMS, MS_STRIDE, MS_STAGE>(partial, c * groups, (c + 1) * groups, s_stage);
        if (tid < MS_SUMS) s_mean[2 * c + tid] = total / n;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int q = 0; q < 6; q++) means[level * MS_MEANS + q] = s_mean[q];
    if (level != MS_LEVELS - 1) return;
    const float nan = __int_as_float(0x7fc00000);
    if (header != nullptr && header->overflow != 0u) {  // the render outgrew its context: its images are invalid, and so is the row
#pragma unroll
        for (int q = 0; q < MS_SLOTS; q++) out[q] = nan;
        return;
    }
    // pytorch_msssim's weights, float32 widened
    const double wt[MS_LEVELS] = {(double)0.0448f, (double)0.2856f, (double)0.3001f, (double)0.2363f, (double)0.1333f};
    double ms[3] = {1.0, 1.0, 1.0};
    for (int l = 0; l < MS_LEVELS; l++)
        for (int c = 0; c < 3; c++) {
            // the earlier levels' means were left by earlier launches of this call; a NaN mean stays NaN (fmax would drop it)
            const double m = l == MS_LEVELS - 1 ? s_mean[2 * c + 1] : means[l * MS_MEANS + 2 * c];
            const double f = m < 0.0 ? 0.0 : m;
            out[4 + 3 * l + c] = (float)f;
            ms[c] *= pow(f, wt[l]);
        }
    out[0] = (float)(((ms[0] + ms[1]) + ms[2]) / 3.0);
    out[1] = (float)ms[0], out[2] = (float)ms[1], out[3] = (float)ms[2];
    out[19] = nan;
}

}  // namespace

static size_t dqo_msssim_ws_bytes(int W, int H) { return ms_ws(nullptr, W, H).total; }

static int dqo_launch_msssim(int W, int H, const float* render, const float* gt_color, const DqoRastHeader* header, float* out_row, void* ws,
                             hipStream_t s) {
    const MsWorkspace k = ms_ws(ws, W, H);
    const DqoSsimWindow win = dqo_ssim_window();
    const float *x = render, *y = gt_color;
    int w = W, h = H;
    for (int l = 0; l < MS_LEVELS; l++) {
        const MsLevel L = ms_level(w, h);
        DQO_LAUNCH("msssim_level_kernel", msssim_level_kernel, dim3((unsigned)L.blocks), dim3(256), s, w, h, x, y, win, l, L.tiles_x, L.run,
                   L.groups_x, L.groups, k.ticket, k.partial, k.means, header, out_row);
        if (l == MS_LEVELS - 1) break;
        const int ow = ms_next(w), oh = ms_next(h);
        const size_t on = (size_t)ow * oh;
        DQO_LAUNCH("msssim_pool_kernel", msssim_pool_kernel, dim3((unsigned)((on + 255) / 256), 6), dim3(256), s, w, h, x, y, ow, oh, k.pooled[l + 1]);
        x = k.pooled[l + 1], y = x + 3 * on;
        w = ow, h = oh;
    }
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// eval_picture's "ssim" (SLAM/eval.py:19-25, :64): pytorch_msssim's ms_ssim, which asserts min(H, W) > (11 - 1) * 2^4
static bool msssim_size_ok(int32_t W, int32_t H) { return W > 160 && H > 160 && (int64_t)W * H < (1ll << 31) / 3; }

DQO_API size_t dqo_eval_ms_ssim_workspace_bytes(int32_t W, int32_t H) { return msssim_size_ok(W, H) ? dqo_msssim_ws_bytes(W, H) : 0; }

DQO_API int dqo_eval_ms_ssim(int32_t W, int32_t H, const float* render, const float* gt_color, const DqoRastHeader* render_header, float* out,
                             int32_t row, void* ws, size_t ws_bytes, void* stream) {
    DQO_CHECK_ARG(msssim_size_ok(W, H), "bad image size %d x %d: MS-SSIM needs both sides > 160 (five levels of an 11-tap window)", W, H);
    DQO_CHECK_ARG(render && gt_color && out, "null pointer");
    DQO_CHECK_ARG(row >= 0, "bad row %d", row);
    DQO_CHECK_WS("ms_ssim", ws, ws_bytes, dqo_msssim_ws_bytes(W, H));
    return dqo_launch_msssim(W, H, render, gt_color, render_header, out + (size_t)20 * row, ws, (hipStream_t)stream);
}

}  // extern "C"
