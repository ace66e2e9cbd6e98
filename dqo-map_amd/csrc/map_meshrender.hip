// Mesh depth for gfx950: a triangle mesh rasterised to depth in K views — the render that the Depth L1 number of the dense-SLAM
// evaluation protocols (the NICE-SLAM lineage) compares pixel by pixel, and a depth for dqo_mesh_cull's occlusion test where no sensor
// depth exists.  No rasterising library exists on this platform, so include/dqo_raster.h (dqo_mesh_render_depth) defines the rule and
// tests/mesh_render_oracle.py restates it in numpy.  The operand, the counts and the views are dqo_mesh_cull's (dqo_mesh_operand.h,
// map_meshcull.hip): rows behind the counts are never read, grids are sized from the capacities.
//
// This file is compiled with -ffp-contract=off.  Per valid face f < F with corners i = 0, 1, 2 (vertex ids v_i) and used view k:
//   float32, one rounding per operation, left to right, `/` the correctly rounded one — dqo_mesh_cull's own statements:
//     pc_i,r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3]            m = w2c[k], row major
//     in front: pc_i,z > near.  No corner in front: skipped; some but not all: dropped at the near plane and counted (no clipping)
//     x_i = (pc_i,x * fx) / pc_i,z + cx;  y_i likewise with fy, cy              (pixel centres at integer coordinates)
//     box: lo = ceil(min x_i), below 0 -> 0; hi = floor(max x_i), above W - 1 -> W - 1 (float32), the same in y; not lo <= hi: skipped
//   double, from the widened floats, one rounding per operation:
//     edge (i, j), (p, q) = (i, j) if v_i < v_j else (j, i):  E = (x_q - x_p) * (Y - y_p) - (y_q - y_p) * (X - x_p);  e_ij = E if p is i
//     else -E — two faces that share an edge compute opposite values, so no pixel centre falls between them
//     A = e_01 at (x_2, y_2).  A repeated vertex id or A == 0: degenerate, counted, skipped
//     covered: A > 0 and e_01, e_12, e_20 all >= 0, or A < 0 and all <= 0 (inclusive; both sides of a face are rendered)
//     n = (P_1 - P_0) x (P_2 - P_0), P_i = pc_i;  r_x = (X - cx) / fx, r_y = (Y - cy) / fy
//     nr = (n_x * r_x + n_y * r_y) + n_z, nr == 0: no hit;  z = ((n_x * P_0,x + n_y * P_0,y) + n_z * P_0,z) / nr
//     z below min pc_i,z -> that, above max pc_i,z -> that;  d = (float)z;  a hit iff d > near && d <= depth_trunc
//   key = (uint64)(bits of d) << 32 | f; a pixel keeps the MINIMUM key: the nearest face, the lower face id at equal depth — whatever
//   order the faces arrive in.
//
// dqo_mesh_render_depth — three launches of 256-thread blocks, whatever the data:
//   clear      keys = all ones (16-byte stores), header = 0, the used views as one bit each (view_keep's bytes are read here only);
//   rasterise  the hot path, F x n_views.  A grid over (256 faces, MR_CHUNK = 32 views): a lane holds its face's nine corner floats in
//              VGPRs across the chunk; the chunk's word, the view's index and its twelve matrix words are wave-uniform scalar loads.
//              A pair whose clipped box has at most MR_SMALL_MAX pixels is walked by its own lane.  A larger one is flagged: after the
//              lanes' own walks a ballot finds the flagged lanes, and for each the WHOLE wave takes the face — its floats broadcast by
//              v_readlane, the set-up recomputed by every lane (the same bits), the box strode in 8 x 8 pixel tiles, a lane a pixel —
//              so no lane walks a wall-sized triangle alone.  Both paths call one pixel function.  Per hit: one 64-bit no-return
//              integer min atomic, which the wave does not wait for.  (A plain load of the pixel's key in front of it, to skip the
//              atomic where it cannot win, was measured and is not here: the wave has to wait for the load, and the rasterise launch
//              took 1.81 ms with it against 0.97 ms without on the volume's mesh, 310 ms against 155 ms on two wall-sized triangles
//              — profiles/mesh_render.txt.)  The counts: registers across the chunk, one integer add per wave and count on one of
//              DQO_COUNT_LINES lines;
//   resolve    depth, face_index from the keys, MR_RES_BLOCKS blocks at most striding the pixels (with a block, and so a ticket with
//              its barriers and fence, per 1024 pixels this launch took 3.1 ms on 81.6 M pixels; so: 0.23 ms, the bytes alone 0.12);
//              the hits counted; the last block (dqo_reduce.h) sums the lines into header[1..6], leaves them at zero, counts the
//              used views' bits -> header[0].
// Integer atomics only (min, whose result does not depend on the order; adds; the tickets, which come back at zero); nothing is
// allocated, set by a memset, read back or synchronised: the entry can be captured in a hipGraph.
//
// dqo_mesh_render_depth_clip — the same three launches with the rasterise kernel's CLIP instantiation (the plain entry launches the
// other one, whose code the flag leaves as it was: 118 VGPRs, no scratch; CLIP: 186 VGPRs, no scratch).  A pair with 1 or 2 corners in
// front is not dropped: homogeneous rasterisation, no clip polygon (include/dqo_raster.h states it; tests/mesh_clip_oracle.py restates it)
//     an edge with both endpoints in front keeps the 2-D form above; any other edge: c = P_p x P_q, E = (c_x * r_x + c_y * r_y) + c_z
//     A = P_0 . (P_1 x P_2);  covered and the depth as above — the test d > near IS the clip
//     box (mr_cross_box): the projected corners in front and the edges' crossings of z = near, in double, a pixel of margin; with
//     near == 0 a crossing is a point at infinity and opens its side to the image border
//   and takes the same two paths by its box: its own lane, or — the wall-sized ones — the whole wave.
#include <algorithm>

#include "dqo_common.h"
#include "dqo_mesh_operand.h"
#include "dqo_reduce.h"

namespace {

typedef unsigned long long u64;

enum {
    MR_CHUNK = 32,       // views per block of the rasterise launch: one word of used-view bits
    MR_MAX_VIEWS = 65535,
    MR_BITS_BYTES = (MR_MAX_VIEWS / MR_CHUNK + 1) * 4,  // 2048 words: a multiple of 256 bytes
    MR_SMALL_MAX = 64,   // pixels of a clipped box that one lane walks alone (include/dqo_raster.h names it: header[5] depends on it)
    MR_CLEAR_PAIRS = 4,  // 16-byte stores per thread of the clear launch
    MR_RES_PIX = 4,      // pixels per thread and round of the resolve launch
    MR_RES_BLOCKS = 2048,  // its blocks at most: eight to a CU
    MR_MAX_SIDE = 1 << 24,  // W - 1 and H - 1 are exact float32
};
static_assert(MR_BITS_BYTES % 256 == 0, "the workspace's parts are multiples of 256 bytes");
// header words that are sums of the count lines (dqo_line_totals: word k of a line is header[k])
enum { MR_BAD = 1, MR_RAST = 2, MR_NEAR = 3, MR_DEGEN = 4, MR_COOP = 5, MR_HITS = 6 };
constexpr uint32_t MR_SUMMED = 1u << MR_BAD | 1u << MR_RAST | 1u << MR_NEAR | 1u << MR_DEGEN | 1u << MR_COOP | 1u << MR_HITS;
constexpr u64 MR_NO_HIT = ~0ull;

struct MrWork {
    int32_t* head;       // the ticket words
    int32_t* acc;        // [DQO_COUNT_LINES][64] word k of a line: count k of the call
    uint32_t* viewbits;  // [chunks of n_views] bit j of word c: view 32 c + j is used
    u64* keys;           // [n_views * H * W], rounded up to 256 bytes
};

struct MrCamera {
    int W, H;
    float fx, fy, cx, cy, near, depth_trunc;
};

// one edge function: E = dx * (Y - yp) - dy * (X - xp), e = fwd ? E : -E
struct MrEdge {
    double xp, yp, dx, dy;
    bool fwd;
};
// what a (face, view) pair's pixels need, in double from the float32 corners
struct MrSetup {
    MrEdge e[3];
    double A, nx, ny, nz, np0, zmin, zmax, cx, cy, fx, fy;
};

__device__ __forceinline__ MrEdge mr_edge(float xi, float yi, float xj, float yj, bool i_first) {
    MrEdge e;
    const double xp = i_first ? (double)xi : (double)xj, yp = i_first ? (double)yi : (double)yj;
    const double xq = i_first ? (double)xj : (double)xi, yq = i_first ? (double)yj : (double)yi;
    e.xp = xp, e.yp = yp, e.dx = xq - xp, e.dy = yq - yp, e.fwd = i_first;
    return e;
}
__device__ __forceinline__ double mr_edge_at(const MrEdge& e, double X, double Y) {
#pragma clang fp contract(off)
    const double E = e.dx * (Y - e.yp) - e.dy * (X - e.xp);
    return e.fwd ? E : -E;
}

// the 3-D form of an edge that has an endpoint not in front: c = P_p x P_q in (xp, yp, dx);  E = (c_x * r_x + c_y * r_y) + c_z, r the pixel's ray
__device__ __forceinline__ double mr_edge3_at(const MrEdge& e, double rx, double ry) {
#pragma clang fp contract(off)
    const double E = (e.xp * rx + e.yp * ry) + e.dx;
    return e.fwd ? E : -E;
}

// x, y: the projected corners; P: pc of the corners (P[3 i + r]); order: bit 0: v_0 < v_1, bit 1: v_1 < v_2, bit 2: v_2 < v_0
__device__ __forceinline__ MrSetup mr_setup(const float (&x)[3], const float (&y)[3], const float (&P)[9], uint32_t order, const MrCamera& cam) {
#pragma clang fp contract(off)
    MrSetup s;
    s.e[0] = mr_edge(x[0], y[0], x[1], y[1], (order & 1u) != 0u);
    s.e[1] = mr_edge(x[1], y[1], x[2], y[2], (order & 2u) != 0u);
    s.e[2] = mr_edge(x[2], y[2], x[0], y[0], (order & 4u) != 0u);
    s.A = mr_edge_at(s.e[0], (double)x[2], (double)y[2]);
    const double ax = (double)P[3] - (double)P[0], ay = (double)P[4] - (double)P[1], az = (double)P[5] - (double)P[2];
    const double bx = (double)P[6] - (double)P[0], by = (double)P[7] - (double)P[1], bz = (double)P[8] - (double)P[2];
    s.nx = ay * bz - az * by, s.ny = az * bx - ax * bz, s.nz = ax * by - ay * bx;
    s.np0 = (s.nx * (double)P[0] + s.ny * (double)P[1]) + s.nz * (double)P[2];
    float zmin = P[2], zmax = P[2];
    if (P[5] < zmin) zmin = P[5];
    if (P[8] < zmin) zmin = P[8];
    if (P[5] > zmax) zmax = P[5];
    if (P[8] > zmax) zmax = P[8];
    s.zmin = (double)zmin, s.zmax = (double)zmax;
    s.cx = (double)cam.cx, s.cy = (double)cam.cy, s.fx = (double)cam.fx, s.fy = (double)cam.fy;
    return s;
}

// The set-up of a pair that CROSSES the near plane (dqo_mesh_render_depth_clip): front = bit i: corner i is in front.  An edge with both
// endpoints in front keeps the 2-D form on its projected corners (x, y of a corner that is not in front are never read); any other edge
// takes the 3-D form on (p, q), the endpoints ordered by vertex id as in mr_setup; A = the triple product P_0 . (P_1 x P_2).  The
// plane, np0 and the z range are mr_setup's.
__device__ __forceinline__ MrSetup mr_setup_cross(const float (&x)[3], const float (&y)[3], const float (&P)[9], uint32_t order, uint32_t front,
                                                  const MrCamera& cam) {
#pragma clang fp contract(off)
    MrSetup s = mr_setup(x, y, P, order, cam);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3;
        if ((front >> i & 1u) != 0u && (front >> j & 1u) != 0u) continue;
        const bool i_first = (order >> i & 1u) != 0u;
        const int p = i_first ? i : j, q = i_first ? j : i;
        const double px = (double)P[3 * p], py = (double)P[3 * p + 1], pz = (double)P[3 * p + 2];
        const double qx = (double)P[3 * q], qy = (double)P[3 * q + 1], qz = (double)P[3 * q + 2];
        s.e[i].xp = py * qz - pz * qy, s.e[i].yp = pz * qx - px * qz, s.e[i].dx = px * qy - py * qx, s.e[i].dy = 0.0;
    }
    const double tx = (double)P[4] * (double)P[8] - (double)P[5] * (double)P[7];
    const double ty = (double)P[5] * (double)P[6] - (double)P[3] * (double)P[8];
    const double tz = (double)P[3] * (double)P[7] - (double)P[4] * (double)P[6];
    s.A = ((double)P[0] * tx + (double)P[1] * ty) + (double)P[2] * tz;
    return s;
}

// THE pixel function of both paths: pixel (X, Y) of view plane `keys` against face f.  (X, Y) lies inside the image: the box is clipped.
// CROSS: the pair crosses the near plane (s is mr_setup_cross's, front its corners in front); the depth test below is what clips it.
template <bool CROSS>
__device__ __forceinline__ void mr_pixel(const MrSetup& s, uint32_t front, int X, int Y, uint32_t f, const MrCamera& cam, u64* __restrict__ keys) {
#pragma clang fp contract(off)
    const double Xd = (double)X, Yd = (double)Y;
    double e0, e1, e2, rx, ry;
    if (CROSS) {
        rx = (Xd - s.cx) / s.fx, ry = (Yd - s.cy) / s.fy;
        e0 = (front & 3u) == 3u ? mr_edge_at(s.e[0], Xd, Yd) : mr_edge3_at(s.e[0], rx, ry);
        e1 = (front & 6u) == 6u ? mr_edge_at(s.e[1], Xd, Yd) : mr_edge3_at(s.e[1], rx, ry);
        e2 = (front & 5u) == 5u ? mr_edge_at(s.e[2], Xd, Yd) : mr_edge3_at(s.e[2], rx, ry);
    } else e0 = mr_edge_at(s.e[0], Xd, Yd), e1 = mr_edge_at(s.e[1], Xd, Yd), e2 = mr_edge_at(s.e[2], Xd, Yd);
    const bool covered = (s.A > 0.0 && e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (s.A < 0.0 && e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!covered) return;
    if (!CROSS) rx = (Xd - s.cx) / s.fx, ry = (Yd - s.cy) / s.fy;
    const double nr = (s.nx * rx + s.ny * ry) + s.nz;
    if (nr == 0.0) return;
    double z = s.np0 / nr;
    if (z < s.zmin) z = s.zmin;
    if (z > s.zmax) z = s.zmax;
    const float d = (float)z;
    if (!(d > cam.near && d <= cam.depth_trunc)) return;
    const u64 key = (u64)__float_as_uint(d) << 32 | (u64)f;
    (void)__hip_atomic_fetch_min(keys + ((size_t)Y * (size_t)cam.W + (size_t)X), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void mesh_render_clear_kernel(uint32_t n_views, const uint8_t* __restrict__ view_keep, size_t key_pairs, MrWork w,
                                                                int32_t* __restrict__ header) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 8) header[i] = 0;
    if (i < (n_views + (uint32_t)MR_CHUNK - 1u) / (uint32_t)MR_CHUNK) {
        uint32_t bits = 0u;
        for (uint32_t j = 0; j < (uint32_t)MR_CHUNK; j++) {
            const uint32_t k = (uint32_t)i * (uint32_t)MR_CHUNK + j;
            if (k < n_views && (view_keep == nullptr || view_keep[k] != 0)) bits |= 1u << j;
        }
        w.viewbits[i] = bits;
    }
    ulonglong2* const pairs = reinterpret_cast<ulonglong2*>(w.keys);  // (the part is 256-byte aligned and rounded up to 256 bytes)
#pragma unroll
    for (int j = 0; j < MR_CLEAR_PAIRS; j++) {
        const size_t p = ((size_t)blockIdx.x * MR_CLEAR_PAIRS + j) * 256 + threadIdx.x;
        if (p < key_pairs) pairs[p] = make_ulonglong2(MR_NO_HIT, MR_NO_HIT);
    }
}

__device__ __forceinline__ float mr_lane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// The box of a pair that crosses the near plane, in double: the hull of what can be covered is spanned by the projected corners in
// front (x, y: the float32 ones, widened) and by the two points where an edge from a corner in front (a) to one that is not (b) meets
// z = near,
//     t = (near - z_a) / (z_b - z_a);  q = P_a + t * (P_b - P_a) in x and y;  u = (q_x * fx) / near + cx;  v likewise with fy, cy
// — with near == 0 a crossing is a point at infinity: u is +inf or -inf by the sign of q_x (the side opens to the image border) or a
// NaN (q_x == 0), which the comparisons leave out.  lo = ceil(min) - 1, below 0 -> 0; hi = floor(max) + 1, above W - 1 -> W - 1: a
// pixel of margin, since the float32 corners and the 3-D edges do not meet in exactly one point.  False unless lo <= hi on both axes.
__device__ __forceinline__ bool mr_cross_box(const float (&x)[3], const float (&y)[3], const float (&P)[9], uint32_t front, const MrCamera& cam,
                                             int& bx0, int& bx1, int& by0, int& by1) {
#pragma clang fp contract(off)
    const double inf = __builtin_huge_val(), near = (double)cam.near;
    double xmin = inf, xmax = -inf, ymin = inf, ymax = -inf;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if ((front >> i & 1u) == 0u) continue;
        const double u = (double)x[i], v = (double)y[i];
        if (u < xmin) xmin = u;
        if (u > xmax) xmax = u;
        if (v < ymin) ymin = v;
        if (v > ymax) ymax = v;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3;
        if ((front >> i & 1u) == (front >> j & 1u)) continue;
        const int a = (front >> i & 1u) != 0u ? i : j, b = a == i ? j : i;
        const double za = (double)P[3 * a + 2], t = (near - za) / ((double)P[3 * b + 2] - za);
        const double qx = (double)P[3 * a] + t * ((double)P[3 * b] - (double)P[3 * a]);
        const double qy = (double)P[3 * a + 1] + t * ((double)P[3 * b + 1] - (double)P[3 * a + 1]);
        const double u = (qx * (double)cam.fx) / near + (double)cam.cx, v = (qy * (double)cam.fy) / near + (double)cam.cy;
        if (u < xmin) xmin = u;
        if (u > xmax) xmax = u;
        if (v < ymin) ymin = v;
        if (v > ymax) ymax = v;
    }
    double x0 = ceil(xmin) - 1.0, x1 = floor(xmax) + 1.0, y0 = ceil(ymin) - 1.0, y1 = floor(ymax) + 1.0;
    if (x0 < 0.0) x0 = 0.0;
    if (y0 < 0.0) y0 = 0.0;
    if (x1 > (double)(cam.W - 1)) x1 = (double)(cam.W - 1);
    if (y1 > (double)(cam.H - 1)) y1 = (double)(cam.H - 1);
    if (!(x0 <= x1 && y0 <= y1)) return false;  // (false for a NaN; all four lie inside [0, W - 1] x [0, H - 1] here)
    bx0 = (int)x0, bx1 = (int)x1, by0 = (int)y0, by1 = (int)y1;
    return true;
}

// a flagged pair's box by the whole wave, in 8 x 8 pixel tiles, a lane a pixel
template <bool CROSS>
__device__ __forceinline__ void mr_wave_walk(const MrSetup& s, uint32_t front, int x0, int x1, int y0, int y1, int lane, uint32_t f,
                                             const MrCamera& cam, u64* __restrict__ keys) {
    const int lx = lane & 7, ly = lane >> 3;
    for (int ty = y0; ty <= y1; ty += 8)
        for (int tx = x0; tx <= x1; tx += 8) {
            const int X = tx + lx, Y = ty + ly;
            if (X <= x1 && Y <= y1) mr_pixel<CROSS>(s, front, X, Y, f, cam, keys);
        }
}

// CLIP: dqo_mesh_render_depth_clip's rule — a pair that crosses the near plane is rasterised (mr_setup_cross, mr_cross_box), not dropped
template <bool CLIP>
__global__ __launch_bounds__(256) void mesh_render_raster_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t cap_f,
                                                                 const float* __restrict__ w2c, MrCamera cam, MrWork w) {
#pragma clang fp contract(off)
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    if (blockIdx.x * 256u >= F) return;  // (block-uniform)
    uint32_t bits = w.viewbits[blockIdx.y];  // (wave-uniform: a scalar load)
    const int lane = threadIdx.x & 63;
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    int32_t ia = 0, ib = 0, ic = 0;
    const bool live = f < F;
    const bool ok = live && mo_face(faces, f, V, ia, ib, ic);
    int32_t* const line = w.acc + ((blockIdx.x + blockIdx.y) % (uint32_t)DQO_COUNT_LINES) * 64u;
    if (blockIdx.y == 0u) {  // a face's bad index is counted once, by the first chunk's block
        const int n = __popcll(__ballot(live && !ok));
        if (lane == 0 && n > 0) atomicAdd(&line[MR_BAD], n);
    }
    if (bits == 0u) return;
    float c[9];
#pragma unroll
    for (int q = 0; q < 9; q++) c[q] = 0.0f;
    if (ok) {
        const int32_t id[3] = {ia, ib, ic};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int r = 0; r < 3; r++) c[3 * i + r] = vertices[3 * (size_t)id[i] + r];
    }
    const bool repeated = ia == ib || ib == ic || ia == ic;
    const uint32_t order = (ia < ib ? 1u : 0u) | (ib < ic ? 2u : 0u) | (ic < ia ? 4u : 0u);
    const float wmax = (float)(cam.W - 1), hmax = (float)(cam.H - 1);
    const size_t plane = (size_t)cam.W * (size_t)cam.H;
    uint32_t n_rast = 0u, n_near = 0u, n_degen = 0u, n_coop = 0u;
    while (bits != 0u) {  // (wave-uniform)
        const uint32_t k = blockIdx.y * (uint32_t)MR_CHUNK + (uint32_t)(__ffs((int)bits) - 1);
        bits &= bits - 1u;
        const float* __restrict__ m = w2c + 16 * (size_t)k;  // (a wave-uniform address: twelve words by scalar loads)
        u64* const keys = w.keys + (size_t)k * plane;
        float P[9], x[3] = {0.0f, 0.0f, 0.0f}, y[3] = {0.0f, 0.0f, 0.0f};
        int front = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float vx = c[3 * i], vy = c[3 * i + 1], vz = c[3 * i + 2];
            P[3 * i] = ((m[0] * vx + m[1] * vy) + m[2] * vz) + m[3];
            P[3 * i + 1] = ((m[4] * vx + m[5] * vy) + m[6] * vz) + m[7];
            P[3 * i + 2] = ((m[8] * vx + m[9] * vy) + m[10] * vz) + m[11];
            front += P[3 * i + 2] > cam.near ? 1 : 0;
        }
        bool large = false;
        int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
        uint32_t cross = 7u;  // (CLIP) the corners in front of a flagged pair that crosses the near plane; 7: it does not
        if (ok && front > 0) {
            if (front < 3) {
                n_near++;
                if (CLIP) {
                    uint32_t fm = 0u;
#pragma unroll
                    for (int i = 0; i < 3; i++)
                        if (P[3 * i + 2] > cam.near) {
                            fm |= 1u << i;
                            x[i] = (P[3 * i] * cam.fx) / P[3 * i + 2] + cam.cx;
                            y[i] = (P[3 * i + 1] * cam.fy) / P[3 * i + 2] + cam.cy;
                        }
                    if (mr_cross_box(x, y, P, fm, cam, bx0, bx1, by0, by1)) {
                        const MrSetup s = mr_setup_cross(x, y, P, order, fm, cam);
                        if (repeated || s.A == 0.0) n_degen++;
                        else {
                            n_rast++;
                            const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
                            large = bw > MR_SMALL_MAX || bh > MR_SMALL_MAX || bw * bh > MR_SMALL_MAX;
                            if (!large) {
                                for (int Y = by0; Y <= by1; Y++)
                                    for (int X = bx0; X <= bx1; X++) mr_pixel<true>(s, fm, X, Y, f, cam, keys);
                            } else n_coop++, cross = fm;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    x[i] = (P[3 * i] * cam.fx) / P[3 * i + 2] + cam.cx;
                    y[i] = (P[3 * i + 1] * cam.fy) / P[3 * i + 2] + cam.cy;
                }
                float xmin = x[0], xmax = x[0], ymin = y[0], ymax = y[0];
                if (x[1] < xmin) xmin = x[1];
                if (x[2] < xmin) xmin = x[2];
                if (x[1] > xmax) xmax = x[1];
                if (x[2] > xmax) xmax = x[2];
                if (y[1] < ymin) ymin = y[1];
                if (y[2] < ymin) ymin = y[2];
                if (y[1] > ymax) ymax = y[1];
                if (y[2] > ymax) ymax = y[2];
                float x0f = ceilf(xmin), x1f = floorf(xmax), y0f = ceilf(ymin), y1f = floorf(ymax);
                if (x0f < 0.0f) x0f = 0.0f;
                if (y0f < 0.0f) y0f = 0.0f;
                if (x1f > wmax) x1f = wmax;
                if (y1f > hmax) y1f = hmax;
                if (x0f <= x1f && y0f <= y1f) {  // (false for a NaN; all four lie inside [0, W - 1] x [0, H - 1] here)
                    const MrSetup s = mr_setup(x, y, P, order, cam);
                    if (repeated || s.A == 0.0) n_degen++;
                    else {
                        n_rast++;
                        bx0 = (int)x0f, bx1 = (int)x1f, by0 = (int)y0f, by1 = (int)y1f;
                        const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
                        large = bw > MR_SMALL_MAX || bh > MR_SMALL_MAX || bw * bh > MR_SMALL_MAX;
                        if (!large) {
                            for (int Y = by0; Y <= by1; Y++)
                                for (int X = bx0; X <= bx1; X++) mr_pixel<false>(s, 7u, X, Y, f, cam, keys);
                        } else n_coop++;
                    }
                }
            }
        }
        // the flagged pairs, each by the whole wave: the lane's floats broadcast, the set-up recomputed (the same bits in every lane)
        u64 todo = __ballot(large);
        while (todo != 0ull) {  // (wave-uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            float qx[3], qy[3], qP[9];
#pragma unroll
            for (int i = 0; i < 3; i++) qx[i] = mr_lane_f(x[i], src), qy[i] = mr_lane_f(y[i], src);
#pragma unroll
            for (int q = 0; q < 9; q++) qP[q] = mr_lane_f(P[q], src);
            const uint32_t qorder = (uint32_t)__builtin_amdgcn_readlane((int)order, src);
            const int qx0 = __builtin_amdgcn_readlane(bx0, src), qx1 = __builtin_amdgcn_readlane(bx1, src);
            const int qy0 = __builtin_amdgcn_readlane(by0, src), qy1 = __builtin_amdgcn_readlane(by1, src);
            const uint32_t qf = f - (uint32_t)lane + (uint32_t)src;
            const uint32_t qcross = CLIP ? (uint32_t)__builtin_amdgcn_readlane((int)cross, src) : 7u;
            if (CLIP && qcross != 7u) {  // (wave-uniform)
                const MrSetup s = mr_setup_cross(qx, qy, qP, qorder, qcross, cam);
                mr_wave_walk<true>(s, qcross, qx0, qx1, qy0, qy1, lane, qf, cam, keys);
            } else {
                const MrSetup s = mr_setup(qx, qy, qP, qorder, cam);
                mr_wave_walk<false>(s, 7u, qx0, qx1, qy0, qy1, lane, qf, cam, keys);
            }
        }
    }
    n_rast = dqo_wave_sum_u32(n_rast, lane), n_near = dqo_wave_sum_u32(n_near, lane);
    n_degen = dqo_wave_sum_u32(n_degen, lane), n_coop = dqo_wave_sum_u32(n_coop, lane);
    if (lane == 0) {
        if (n_rast > 0u) atomicAdd(&line[MR_RAST], (int32_t)n_rast);
        if (n_near > 0u) atomicAdd(&line[MR_NEAR], (int32_t)n_near);
        if (n_degen > 0u) atomicAdd(&line[MR_DEGEN], (int32_t)n_degen);
        if (n_coop > 0u) atomicAdd(&line[MR_COOP], (int32_t)n_coop);
    }
}

__global__ __launch_bounds__(256) void mesh_render_resolve_kernel(size_t pixels, uint32_t n_views, MrWork w, float* __restrict__ depth,
                                                                  int32_t* __restrict__ face_index, int32_t* __restrict__ header) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63;
    uint32_t hits = 0u;
    for (size_t base = (size_t)blockIdx.x * (256 * MR_RES_PIX); base < pixels; base += (size_t)gridDim.x * (256 * MR_RES_PIX)) {
#pragma unroll
        for (int j = 0; j < MR_RES_PIX; j++) {
            const size_t i = base + (size_t)j * 256 + threadIdx.x;
            if (i < pixels) {
                const u64 key = w.keys[i];
                const bool hit = key != MR_NO_HIT;
                depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
                if (face_index != nullptr) face_index[i] = hit ? (int32_t)(uint32_t)key : -1;
                hits += hit ? 1u : 0u;
            }
        }
    }
    hits = dqo_wave_sum_u32(hits, lane);
    if (lane == 0 && hits > 0u) atomicAdd(&w.acc[(blockIdx.x % (uint32_t)DQO_COUNT_LINES) * 64u + MR_HITS], (int32_t)hits);
    if (!dqo_last_block(w.head, &s_last)) return;
    dqo_line_totals(w.acc, MR_SUMMED, header);  // header[1..6]; the lines are zero again
    uint32_t used = 0u, all;
    for (uint32_t c = threadIdx.x; c < (n_views + (uint32_t)MR_CHUNK - 1u) / (uint32_t)MR_CHUNK; c += 256u) used += (uint32_t)__popc(w.viewbits[c]);
    dqo_block_exclusive<uint32_t>(used, all, s_wave);
    if (threadIdx.x == 0) header[0] = (int32_t)all, header[7] = 0;
}

// the ticket words | the count lines | the used views' bits | the keys
inline DqoLayout<MrWork> mr_ws(void* base, size_t pixels) {
    MrWork w;
    DqoCarver k(base);
    w.head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.acc = k.take<int32_t>(DQO_COUNT_LINES * 64 * 4);
    w.viewbits = k.take<uint32_t>(MR_BITS_BYTES);
    w.keys = k.take<u64>(pixels * sizeof(u64));
    return {w, k.total()};
}

inline bool mr_image_ok(int64_t n_views, int64_t W, int64_t H) {
    return n_views >= 1 && n_views <= MR_MAX_VIEWS && W >= 1 && H >= 1 && W <= MR_MAX_SIDE && H <= MR_MAX_SIDE &&
           (uint64_t)W * (uint64_t)H <= ((1ull << 40) - 1ull) / (uint64_t)n_views;
}

// what both entries check and size before their three launches
struct MrCall {
    MrWork w;
    MrCamera cam;
    uint32_t ucv, ucf, nv;
    size_t pixels, key_pairs;
    dim3 block, gc, gr, gs;
};

inline int mr_prepare(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces, int32_t n_views,
                      const float* w2c, int32_t W, int32_t H, float fx, float fy, float cx, float cy, float near, float depth_trunc,
                      const float* depth, const int32_t* header, void* workspace, size_t workspace_bytes, MrCall& c) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(n_views >= 1 && n_views <= MR_MAX_VIEWS, "bad n_views %d: 1 to 65535 views", n_views);
    DQO_CHECK_ARG(w2c, "null w2c");
    DQO_CHECK_ARG(mr_image_ok(n_views, W, H),
                  "bad image size %d x %d for %d views: both sides are at least 1 and at most 2^24, n_views * H * W is below 2^40", W, H, n_views);
    DQO_CHECK_ARG((int64_t)cap_faces * (int64_t)n_views < (1ll << 31),
                  "too many pairs: cap_faces %d * n_views %d is not below 2^31 (the pair counts are int32: render the views in chunks)", cap_faces,
                  n_views);
    DQO_CHECK_ARG(near - near == 0.0f && near >= 0.0f, "bad near: it is finite and at least 0");
    DQO_CHECK_ARG(depth_trunc > 0.0f, "bad depth_trunc: it is above 0 (it may be +inf)");
    DQO_CHECK_ARG(depth, "null depth");
    DQO_CHECK_ARG(header != counts, "header must not be the mesh's counts: the first launch clears it before the counts are read");
    c.pixels = (size_t)n_views * (size_t)W * (size_t)H;
    DQO_CHECK_WS("mesh render", workspace, workspace_bytes, mr_ws(nullptr, c.pixels).total);
    c.w = mr_ws(workspace, c.pixels).w;
    c.cam.W = W, c.cam.H = H, c.cam.fx = fx, c.cam.fy = fy, c.cam.cx = cx, c.cam.cy = cy, c.cam.near = near, c.cam.depth_trunc = depth_trunc;
    c.ucv = (uint32_t)cap_vertices, c.ucf = (uint32_t)cap_faces, c.nv = (uint32_t)n_views;
    const size_t chunks = ((size_t)n_views + MR_CHUNK - 1) / MR_CHUNK;
    c.key_pairs = (c.pixels + 1) / 2;
    const size_t clear_blocks = (c.key_pairs + 256 * MR_CLEAR_PAIRS - 1) / (256 * MR_CLEAR_PAIRS);
    c.block = dim3(256), c.gc = dim3((unsigned)(clear_blocks > mo_blocks(chunks) ? clear_blocks : mo_blocks(chunks)));
    c.gr = dim3((unsigned)mo_blocks((size_t)cap_faces), (unsigned)chunks);
    c.gs = dim3((unsigned)std::min<size_t>((c.pixels + 256 * MR_RES_PIX - 1) / (256 * MR_RES_PIX), MR_RES_BLOCKS));
    return DQO_OK;
}

}  // namespace

// ---- entry points (include/dqo_raster.h): size query, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_mesh_render_depth_workspace_bytes(int32_t n_views, int32_t W, int32_t H) {
    return mr_image_ok(n_views, W, H) ? mr_ws(nullptr, (size_t)n_views * (size_t)W * (size_t)H).total : 0;
}

DQO_API int dqo_mesh_render_depth(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                                  int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy, float cx,
                                  float cy, float near, float depth_trunc, float* depth, int32_t* face_index, int32_t* header, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    MrCall c;
    const int rc = mr_prepare(vertices, faces, counts, cap_vertices, cap_faces, n_views, w2c, W, H, fx, fy, cx, cy, near, depth_trunc, depth, header,
                              workspace, workspace_bytes, c);
    if (rc != DQO_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("mesh_render_clear_kernel", mesh_render_clear_kernel, c.gc, c.block, s, c.nv, view_keep, c.key_pairs, c.w, header);
    DQO_LAUNCH("mesh_render_raster_kernel", mesh_render_raster_kernel<false>, c.gr, c.block, s, vertices, faces, counts, c.ucv, c.ucf, w2c, c.cam, c.w);
    DQO_LAUNCH("mesh_render_resolve_kernel", mesh_render_resolve_kernel, c.gs, c.block, s, c.pixels, c.nv, c.w, depth, face_index, header);
    return DQO_OK;
}

// the same call with the rasterise launch's CLIP instantiation: a pair that crosses the near plane is rasterised, header[3] counts it
DQO_API int dqo_mesh_render_depth_clip(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                                       int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy,
                                       float cx, float cy, float near, float depth_trunc, float* depth, int32_t* face_index, int32_t* header,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    MrCall c;
    const int rc = mr_prepare(vertices, faces, counts, cap_vertices, cap_faces, n_views, w2c, W, H, fx, fy, cx, cy, near, depth_trunc, depth, header,
                              workspace, workspace_bytes, c);
    if (rc != DQO_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("mesh_render_clear_kernel", mesh_render_clear_kernel, c.gc, c.block, s, c.nv, view_keep, c.key_pairs, c.w, header);
    DQO_LAUNCH("mesh_render_raster_clip_kernel", mesh_render_raster_kernel<true>, c.gr, c.block, s, vertices, faces, counts, c.ucv, c.ucf, w2c, c.cam,
               c.w);
    DQO_LAUNCH("mesh_render_resolve_kernel", mesh_render_resolve_kernel, c.gs, c.block, s, c.pixels, c.nv, c.w, depth, face_index, header);
    return DQO_OK;
}

}  // extern "C"
