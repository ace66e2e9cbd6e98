// The map as a triangle mesh for gfx950: TSDF fusion of rendered RGB-D frames into a dense uniform volume, and marching tetrahedra on it.
// The reference names the pieces — make_mesh.py walks the dataset's cameras, eval_frame (SLAM/eval.py:299, 316-343) turns each render into
// an RGB-D image and calls volume.integrate(rgbd, intrinsics, w2c) on an open3d TSDF volume — but its make_mesh.py breaks off inside the
// loop, and open3d does not exist on this platform.  So the rule below is the definition (it follows open3d's UniformTSDFVolume integrate
// as published) and tests/tsdf_oracle.py restates it in numpy; nothing here is pinned against the library.
//
// The volume: a dense grid over the caller's box, x fastest, structure of arrays so that a wave's accesses coalesce — tsdf [nz,ny,nx],
// weight [nz,ny,nx], color [3,nz,ny,nx], all float32, and an int32 [8] header.  Cleared (tsdf = 1, weight = 0, color = 0, header = 0) by
// a launch (tsdf_clear_kernel), never by a memset.
//
// tsdf_integrate_kernel (dqo_tsdf_integrate) — one launch, one thread per voxel, float32, one rounding per operation, left to right, none
// contracted; `/` and sqrtf are the correctly rounded ones (hipcc's default for HIP):
//     pw_a = origin_a + ((float)i_a + 0.5f) * L                                  a = x, y, z
//     pc_r = ((m[r][0] * pw_x + m[r][1] * pw_y) + m[r][2] * pw_z) + m[r][3]      m = w2c, row major, read from device memory
//     skip unless pc_z > 0
//     u_f = ((pc_x * fx) / pc_z + cx) + 0.5f;  v_f likewise with fy, cy
//     skip unless u_f >= 0.0001f && u_f < (float)W - 0.0001f                     (the same for v_f and H)
//     u = (int)u_f;  v = (int)v_f;  d = depth[v][u]
//     skip unless d > 0 && d <= depth_trunc
//     mult = sqrtf((1.0f + ((u - cx) / fx) * ((u - cx) / fx)) + ((v - cy) / fy) * ((v - cy) / fy))
//     sdf = (d - pc_z) * mult;  skip unless sdf > -sdf_trunc
//     t = fminf(1.0f, sdf / sdf_trunc);  w = weight
//     tsdf = (tsdf * w + t) / (w + 1.0f);  color_c = (color_c * w + image[c][v][u]) / (w + 1.0f);  weight = w + 1.0f
// Every skip comes before the thread's first access to the volume: a voxel behind the camera, outside the image or without a depth costs
// arithmetic and at most one gathered pixel, and a wave whose 64 voxels are all skipped retires without a volume access.  A touched voxel
// reads 20 bytes and writes 20.  A render that outgrew its context (DqoRastHeader.overflow != 0, tested as dqo_eval_picture tests it)
// integrates nothing and counts in header[5]; every other frame counts in header[4].
//
// dqo_tsdf_extract — a welded, indexed, coloured mesh by marching tetrahedra on the Kuhn decomposition (six tetrahedra per cube around
// its body diagonal: no case table of marching cubes, and watertight by construction because neighbouring cubes cut their shared face
// along the same diagonal).
//   - a cube is the eight lattice points o + {0,1}^3, named by o; it is valid iff all eight weights are > 0;
//   - the corner o + (dx,dy,dz) has code dx + 2 dy + 4 dz.  Tetrahedron k belongs to the k-th permutation p of (0,1,2) in lexicographic
//     order; its path corners are c0 = o, c1 = c0 + e[p0], c2 = c1 + e[p1], c3 = o + (1,1,1);
//   - every tetrahedron edge is one of seven translation-invariant types — offsets (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1),
//     types 0..6 — so an edge is owned by its lower lattice point and its type;
//   - a corner is negative iff tsdf < 0 (0 is positive).  An edge carries a vertex iff its ends differ in sign and at least one valid cube
//     contains it (then both weights are > 0): no vertex is unreferenced;
//   - with a the negative end, s = f_a / (f_a - f_b); position and colour are p_a + s * (p_b - p_a) per component, p the voxel centre;
//   - vertices are numbered in ascending (lattice linear index, edge type);
//   - triangles per tetrahedron case (bit i: path corner i is negative): one negative corner a — the edges (a,b), b the positive corners
//     ascending; three — the edges (a,b), a the negative corners ascending; two, a0 < a1 and b0 < b1 — the quad (a0b0, a0b1, a1b1, a1b0)
//     cut into (q0,q1,q2), (q0,q2,q3).  The last two indices are swapped iff bit `case` of TS_FLIP differs from the parity of p, which
//     turns the right-hand normal to the positive side (free space) by a table, not by a float test;
//   - faces are numbered in ascending (cube linear index, tetrahedron, triangle).
// With cap_vertices below the count the vertex list is cut there, the faces that name a cut vertex are removed from the list, and what is
// left is cut at cap_faces.  header[0..3]: vertices written, faces written, vertices dropped, faces dropped.
// Four launches, no float atomics, the only integer atomics the tickets of dqo_reduce.h: the same bits on every run.  A block of the last
// three walks a SPAN of 2048 consecutive lattice points, 256 at a time: with one block per 256 points the two launches that end in
// dqo_last_block took 1.3 ms each at 256^3 (65536 blocks, each with its fence and ticket) against 0.07 ms for the flags launch.
//   flags    a byte per lattice point: bit 0 the cube it names is valid, bit 1 its tsdf is negative;
//   edges    the 7-bit mask of the point's edges that carry a vertex, their exclusive count within the span (uint16), the span's count;
//            the last block turns the spans' counts into offsets (dqo_scan_block_counts): an edge's vertex id is
//            span offset + in-span count + popcount(mask below its type) — four bytes of workspace per point instead of seven ids;
//   vertices emits the point's vertices and counts the cube's faces (a byte per cube; the ids are looked up only when the vertex list
//            was cut); the last block scans the spans' (kept, all) face counts and writes the header;
//   faces    block-wide scans of the cubes' counts, then every cube writes its triangles.
#include "dqo_common.h"
#include "dqo_reduce.h"

namespace {

typedef unsigned long long u64;

enum : uint32_t {
    TS_FLIP = 0x4D24u,           // cases 0010 0101 1000 1010 1011 1110 (bit 3 first) flip for an even permutation
    TS_PARITY = 0x26u,           // bit k: permutation k is odd
    TS_C1 = 0x442211u,           // nibble k: the code of path corner 1 of tetrahedron k
    TS_C2 = 0x656353u,           // nibble k: the code of path corner 2
    TS_EDGE_CODE = 0x7653421u,   // nibble t: the offset code of edge type t
    TS_TYPE_OF_CODE = 0x65423100u,  // nibble c: the edge type of offset code c
};
enum {
    TS_CHUNKS = 8,                   // runs of 256 lattice points that a block of the edges / vertices / faces launches walks
    TS_SPAN_SHIFT = 11,              // a block's span: 2048 consecutive lattice points
    TS_SPAN = 1 << TS_SPAN_SHIFT,
    TS_VTOTAL = 2,  // a free word of the ticket's line 0: the volume's vertex count, from the edges launch to the next two
};
static_assert(TS_VTOTAL < 16 && TS_SPAN == 256 * TS_CHUNKS && 7 * TS_SPAN < 65536, "workspace head layout; TsdfWs.base is a uint16");

struct TsdfGrid {
    int nx, ny, nz;
    uint32_t N;
    float ox, oy, oz, L;
};

struct TsdfWs {
    int32_t* head;
    uint32_t* vblock;  // [spans] vertices of the span, then of the spans before it
    u64* fpairs;       // [spans] kept faces | all faces << 32 of the span, then of the spans before it
    uint8_t* flags;    // [N]
    uint8_t* mask;     // [N]
    uint8_t* fcount;   // [N] kept faces of the cube
    uint16_t* base;    // [N] vertices of the span's points before this one
};

__host__ __device__ inline size_t ts_blocks(size_t N) { return (N + 255) / 256; }
__host__ __device__ inline size_t ts_spans(size_t N) { return (N + TS_SPAN - 1) / TS_SPAN; }

__device__ __forceinline__ uint32_t ts_offset(const TsdfGrid& g, uint32_t code) {
    return (code & 1u) + ((code >> 1) & 1u) * (uint32_t)g.nx + ((code >> 2) & 1u) * (uint32_t)g.nx * (uint32_t)g.ny;
}

__device__ __forceinline__ void ts_coords(const TsdfGrid& g, uint32_t i, int& x, int& y, int& z) {
    const uint32_t r = i / (uint32_t)g.nx;
    x = (int)(i - r * (uint32_t)g.nx), z = (int)(r / (uint32_t)g.ny), y = (int)(r - (uint32_t)z * (uint32_t)g.ny);
}

// ---- the volume -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_clear_kernel(uint32_t N, float* __restrict__ tsdf, float* __restrict__ weight,
                                                         float* __restrict__ color, int32_t* __restrict__ header) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 8u) header[i] = 0;
    if (i >= N) return;
    tsdf[i] = 1.0f, weight[i] = 0.0f;
    color[i] = 0.0f, color[(size_t)N + i] = 0.0f, color[2 * (size_t)N + i] = 0.0f;
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfGrid g, float sdf_trunc, float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ color, int32_t* __restrict__ header, int W, int H,
                                                             const float* __restrict__ depth, const float* __restrict__ image, float fx,
                                                             float fy, float cx, float cy, const float* __restrict__ w2c, float depth_trunc,
                                                             const DqoRastHeader* __restrict__ render_header) {
#pragma clang fp contract(off)
    // a block is a tile of 64 x 4 voxels of one z: a wave is 64 consecutive x, and the tile's place comes from divisions of the block
    // index — one per wave on the scalar unit, not two per voxel
    const uint32_t nxb = ((uint32_t)g.nx + 63u) / 64u, nyb = ((uint32_t)g.ny + 3u) / 4u;
    const uint32_t rest = blockIdx.x / nxb;
    const int x = (int)((blockIdx.x - rest * nxb) * 64u + (threadIdx.x & 63u));
    const int z = (int)(rest / nyb), y = (int)((rest - (uint32_t)z * nyb) * 4u + (threadIdx.x >> 6));
    const bool valid = render_header == nullptr || render_header->overflow == 0u;  // (an overflowed render: its images are invalid)
    if (blockIdx.x == 0u && threadIdx.x == 0u) header[valid ? 4 : 5] += 1;
    if (!valid || x >= g.nx || y >= g.ny) return;
    const uint32_t i = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx + (uint32_t)x;
    const float pwx = g.ox + ((float)x + 0.5f) * g.L, pwy = g.oy + ((float)y + 0.5f) * g.L, pwz = g.oz + ((float)z + 0.5f) * g.L;
    const float pcz = ((w2c[8] * pwx + w2c[9] * pwy) + w2c[10] * pwz) + w2c[11];
    if (!(pcz > 0.0f)) return;
    const float pcx = ((w2c[0] * pwx + w2c[1] * pwy) + w2c[2] * pwz) + w2c[3];
    const float pcy = ((w2c[4] * pwx + w2c[5] * pwy) + w2c[6] * pwz) + w2c[7];
    const float uf = ((pcx * fx) / pcz + cx) + 0.5f, vf = ((pcy * fy) / pcz + cy) + 0.5f;
    if (!(uf >= 0.0001f && uf < (float)W - 0.0001f && vf >= 0.0001f && vf < (float)H - 0.0001f)) return;
    const int u = (int)uf, v = (int)vf;  // (inside [0, W) x [0, H): the test above)
    const size_t pix = (size_t)v * (size_t)W + (size_t)u;
    const float d = depth[pix];
    if (!(d > 0.0f && d <= depth_trunc)) return;
    const float a = ((float)u - cx) / fx, b = ((float)v - cy) / fy;
    const float mult = sqrtf((1.0f + a * a) + b * b);
    const float sdf = (d - pcz) * mult;
    if (!(sdf > -sdf_trunc)) return;
    const float t = fminf(1.0f, sdf / sdf_trunc);
    const float w = weight[i], w1 = w + 1.0f;
    const size_t WH = (size_t)W * (size_t)H;
    tsdf[i] = (tsdf[i] * w + t) / w1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t k = (size_t)c * g.N + i;
        color[k] = (color[k] * w + image[(size_t)c * WH + pix]) / w1;
    }
    weight[i] = w1;
}

// ---- extract: flags ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_flags_kernel(TsdfGrid g, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= g.N) return;
    int x, y, z;
    ts_coords(g, i, x, y, z);
    bool valid = x + 1 < g.nx && y + 1 < g.ny && z + 1 < g.nz;  // (then every corner i + ts_offset(c) is a lattice point)
    if (valid) {
#pragma unroll
        for (uint32_t c = 0; c < 8u; c++) valid = valid && weight[i + ts_offset(g, c)] > 0.0f;
    }
    flags[i] = (uint8_t)((valid ? 1u : 0u) | (tsdf[i] < 0.0f ? 2u : 0u));
}

// ---- extract: edges ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_edges_kernel(TsdfGrid g, TsdfWs w) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_last;
    uint32_t run = 0u;  // vertices of the span so far
    for (uint32_t chunk = 0; chunk < (uint32_t)TS_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)TS_CHUNKS + chunk) * 256u + threadIdx.x;
        uint32_t mask = 0u;
        if (i < g.N) {
            int x, y, z;
            ts_coords(g, i, x, y, z);
            // bit s of `around`: the cube named by this point - (sx,sy,sz) exists and is valid — the eight cubes that hold this point
            uint32_t around = 0u;
#pragma unroll
            for (uint32_t s = 0; s < 8u; s++) {
                if (((s & 1u) && x == 0) || ((s & 2u) && y == 0) || ((s & 4u) && z == 0)) continue;
                around |= (uint32_t)(w.flags[i - ts_offset(g, s)] & 1u) << s;
            }
            if (around != 0u) {
                const uint32_t neg = (w.flags[i] >> 1) & 1u;
#pragma unroll
                for (uint32_t t = 0; t < 7u; t++) {
                    const uint32_t d = (TS_EDGE_CODE >> (4u * t)) & 7u;
                    // the cubes that hold the edge: those that hold this point and do not step back along an axis the edge runs along
                    uint32_t holds = 0u;
#pragma unroll
                    for (uint32_t s = 0; s < 8u; s++)
                        if ((s & d) == 0u) holds |= (around >> s) & 1u;
                    if (holds == 0u) continue;  // (a valid cube holds the edge: its upper end is a lattice point)
                    if ((((uint32_t)w.flags[i + ts_offset(g, d)] >> 1) & 1u) != neg) mask |= 1u << t;
                }
            }
            w.mask[i] = (uint8_t)mask;
        }
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>((uint32_t)__popc(mask), total, s_wave);
        if (i < g.N) w.base[i] = (uint16_t)(run + before);  // (< 7 * TS_SPAN)
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.vblock[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const uint32_t V = dqo_scan_block_counts<uint32_t, 4>(w.vblock, gridDim.x, 1, s_wave);  // (<= 7 N < 2^31)
    if (threadIdx.x == 0) w.head[TS_VTOTAL] = (int32_t)V;
}

// the vertex id of edge (lattice point, type)
__device__ __forceinline__ uint32_t ts_edge_id(const TsdfWs& w, uint32_t lin, uint32_t t) {
    return w.vblock[lin >> TS_SPAN_SHIFT] + (uint32_t)w.base[lin] + (uint32_t)__popc((uint32_t)w.mask[lin] & ((1u << t) - 1u));
}

// The faces of the valid cube named by lattice point `lin`; neg8: bit c = corner code c is negative.  Returns kept | all << 32.  ids:
// look the vertex ids up (always when EMIT) and keep a triangle only if all three lie below cap_v.  EMIT: kept triangle n goes to
// faces[first + n] if that lies below cap_f.
template <bool EMIT>
__device__ __forceinline__ u64 ts_cube_faces(const TsdfGrid& g, const TsdfWs& w, uint32_t lin, uint32_t neg8, bool ids, uint32_t cap_v,
                                             int32_t* __restrict__ faces, u64 first, u64 cap_f) {
    uint32_t kept = 0u, all = 0u;
    if (neg8 == 0u || neg8 == 255u) return 0ull;
    for (uint32_t k = 0; k < 6u; k++) {
        const uint32_t codes = (((TS_C1 >> (4u * k)) & 7u) << 3) | (((TS_C2 >> (4u * k)) & 7u) << 6) | (7u << 9);  // 3 bits per path corner
        uint32_t cs = 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++) cs |= ((neg8 >> ((codes >> (3u * c)) & 7u)) & 1u) << c;
        if (cs == 0u || cs == 15u) continue;
        const uint32_t inv = ~cs & 15u, n = (uint32_t)__popc(cs);
        // the polygon's corners, 4 bits each: path corner of the negative end | path corner of the positive end << 2
        uint32_t poly = 0u, m = 0u;
        if (n == 1u) {
            const uint32_t a = (uint32_t)__ffs(cs) - 1u;
            for (uint32_t b = 0; b < 4u; b++)
                if ((inv >> b) & 1u) poly |= (a | (b << 2)) << (4u * m++);
        } else if (n == 3u) {
            const uint32_t b = (uint32_t)__ffs(inv) - 1u;
            for (uint32_t a = 0; a < 4u; a++)
                if ((cs >> a) & 1u) poly |= (a | (b << 2)) << (4u * m++);
        } else {
            const uint32_t a0 = (uint32_t)__ffs(cs) - 1u, a1 = 31u - (uint32_t)__clz(cs);
            const uint32_t b0 = (uint32_t)__ffs(inv) - 1u, b1 = 31u - (uint32_t)__clz(inv);
            poly = (a0 | (b0 << 2)) | (a0 | (b1 << 2)) << 4 | (a1 | (b1 << 2)) << 8 | (a1 | (b0 << 2)) << 12;
            m = 4u;
        }
        uint32_t id0 = 0u, id1 = 0u, id2 = 0u, id3 = 0u;
        if (EMIT || ids) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                if (j >= m) break;
                const uint32_t e = (poly >> (4u * j)) & 15u, p = e & 3u, q = e >> 2;
                const uint32_t lo = (codes >> (3u * (p < q ? p : q))) & 7u, hi = (codes >> (3u * (p < q ? q : p))) & 7u;
                const uint32_t id = ts_edge_id(w, lin + ts_offset(g, lo), (TS_TYPE_OF_CODE >> (4u * (hi ^ lo))) & 7u);
                if (j == 0u) id0 = id;
                else if (j == 1u) id1 = id;
                else if (j == 2u) id2 = id;
                else id3 = id;
            }
        }
        const bool flip = (((TS_FLIP >> cs) ^ (TS_PARITY >> k)) & 1u) != 0u;
        for (uint32_t tri = 0; tri + 2u < m; tri++) {  // (q0,q1,q2) and, of a quad, (q0,q2,q3)
            const uint32_t b = tri == 0u ? id1 : id2, c = tri == 0u ? id2 : id3;
            all++;
            if (ids && !(id0 < cap_v && b < cap_v && c < cap_v)) continue;
            if (EMIT) {
                const u64 f = first + kept;
                if (f < cap_f) faces[3 * f] = (int32_t)id0, faces[3 * f + 1] = (int32_t)(flip ? c : b), faces[3 * f + 2] = (int32_t)(flip ? b : c);
            }
            kept++;
        }
    }
    return (u64)kept | ((u64)all << 32);
}

__device__ __forceinline__ uint32_t ts_corner_signs(const TsdfGrid& g, const TsdfWs& w, uint32_t i) {
    uint32_t neg8 = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) neg8 |= (((uint32_t)w.flags[i + ts_offset(g, c)] >> 1) & 1u) << c;
    return neg8;
}

// ---- extract: vertices, and the cubes' face counts ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_vertices_kernel(TsdfGrid g, TsdfWs w, const float* __restrict__ tsdf, const float* __restrict__ color,
                                                            float* __restrict__ vertices, float* __restrict__ vertex_color, uint32_t cap_v,
                                                            uint32_t cap_f, int32_t* __restrict__ header) {
#pragma clang fp contract(off)
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = (uint32_t)w.head[TS_VTOTAL];  // (the edges launch wrote it)
    u64 pair = 0ull;  // this thread's cubes
    for (uint32_t chunk = 0; chunk < (uint32_t)TS_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)TS_CHUNKS + chunk) * 256u + threadIdx.x;
        if (i >= g.N) break;
        const uint32_t mask = w.mask[i];
        if (mask != 0u) {
            int x, y, z;
            ts_coords(g, i, x, y, z);
            uint32_t id = w.vblock[blockIdx.x] + (uint32_t)w.base[i];
            const float fi = tsdf[i];
            for (uint32_t t = 0; t < 7u; t++) {
                if (!((mask >> t) & 1u)) continue;
                if (id < cap_v) {
                    const uint32_t d = (TS_EDGE_CODE >> (4u * t)) & 7u, j = i + ts_offset(g, d);
                    const float fj = tsdf[j];
                    const bool lo_neg = fi < 0.0f;  // a, the negative end, is this point; otherwise the edge's upper end
                    const float fa = lo_neg ? fi : fj, fb = lo_neg ? fj : fi;
                    const float s = fa / (fa - fb);
                    const int xj = x + (int)(d & 1u), yj = y + (int)((d >> 1) & 1u), zj = z + (int)((d >> 2) & 1u);
                    const float pix = g.ox + ((float)x + 0.5f) * g.L, piy = g.oy + ((float)y + 0.5f) * g.L, piz = g.oz + ((float)z + 0.5f) * g.L;
                    const float pjx = g.ox + ((float)xj + 0.5f) * g.L, pjy = g.oy + ((float)yj + 0.5f) * g.L, pjz = g.oz + ((float)zj + 0.5f) * g.L;
                    const float pa[3] = {lo_neg ? pix : pjx, lo_neg ? piy : pjy, lo_neg ? piz : pjz};
                    const float pb[3] = {lo_neg ? pjx : pix, lo_neg ? pjy : piy, lo_neg ? pjz : piz};
                    const uint32_t ia = lo_neg ? i : j, ib = lo_neg ? j : i;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        vertices[3 * (size_t)id + c] = pa[c] + s * (pb[c] - pa[c]);
                        const float ca = color[(size_t)c * g.N + ia], cb = color[(size_t)c * g.N + ib];
                        vertex_color[3 * (size_t)id + c] = ca + s * (cb - ca);
                    }
                }
                id++;
            }
        }
        uint32_t kept = 0u;
        if (w.flags[i] & 1u) {
            const u64 mine = ts_cube_faces<false>(g, w, i, ts_corner_signs(g, w, i), V > cap_v, cap_v, nullptr, 0ull, 0ull);
            kept = (uint32_t)mine, pair += mine;
        }
        w.fcount[i] = (uint8_t)kept;  // (<= 12)
    }
    // the span's (kept, all) pair: both halves of every sum stay below 2^32 (12 N), so one 64-bit add adds the two without a carry
    u64 total;
    dqo_block_exclusive<u64>(pair, total, s_wave);
    if (threadIdx.x == 0) __hip_atomic_store(&w.fpairs[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.fpairs, gridDim.x, 1, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t kept = (uint32_t)sums, all = (uint32_t)(sums >> 32);
        const uint32_t nv = V < cap_v ? V : cap_v, nf = kept < cap_f ? kept : cap_f;
        const uint32_t lost = all - nf;
        header[0] = (int32_t)nv, header[1] = (int32_t)nf, header[2] = (int32_t)(V - nv);
        header[3] = (int32_t)(lost < 0x7fffffffu ? lost : 0x7fffffffu);
    }
}

// ---- extract: faces ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_faces_kernel(TsdfGrid g, TsdfWs w, int32_t* __restrict__ faces, uint32_t cap_v, uint32_t cap_f) {
    __shared__ uint32_t s_wave[4];
    const bool ids = (uint32_t)w.head[TS_VTOTAL] > cap_v;
    u64 run = (u64)(uint32_t)w.fpairs[blockIdx.x];  // kept faces of the spans before this one, then of the span so far
    for (uint32_t chunk = 0; chunk < (uint32_t)TS_CHUNKS; chunk++) {
        if (run >= (u64)cap_f) return;  // (the whole block)
        const uint32_t i = (blockIdx.x * (uint32_t)TS_CHUNKS + chunk) * 256u + threadIdx.x;
        const uint32_t mine = i < g.N ? (uint32_t)w.fcount[i] : 0u;
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>(mine, total, s_wave);
        if (mine != 0u && run + before < (u64)cap_f) ts_cube_faces<true>(g, w, i, ts_corner_signs(g, w, i), ids, cap_v, faces, run + before, (u64)cap_f);
        run += total;
    }
}

inline TsdfGrid ts_grid(int nx, int ny, int nz, float ox, float oy, float oz, float L) {
    TsdfGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.N = (uint32_t)((size_t)nx * ny * nz), g.ox = ox, g.oy = oy, g.oz = oz, g.L = L;
    return g;
}

// every dim >= 2 (a cube needs two points a side) and fewer than 2^28 voxels (7 edges a point: every vertex id stays below 2^31)
inline bool ts_dims_ok(int64_t nx, int64_t ny, int64_t nz) { return nx >= 2 && ny >= 2 && nz >= 2 && nx < (1 << 28) && ny < (1 << 28) && nz < (1 << 28); }
inline bool ts_count_ok(int64_t nx, int64_t ny, int64_t nz) { return nx * ny < (1ll << 28) && nx * ny * nz < (1ll << 28); }

// dqo_tsdf_extract's workspace: the ticket words | vblock | fpairs | flags | mask | fcount | base
inline DqoLayout<TsdfWs> ts_ws(void* base, size_t N) {
    TsdfWs w;
    DqoCarver k(base);
    w.head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.vblock = k.take<uint32_t>(ts_spans(N) * sizeof(uint32_t));
    w.fpairs = k.take<u64>(ts_spans(N) * sizeof(u64));
    w.flags = k.take<uint8_t>(N);
    w.mask = k.take<uint8_t>(N);
    w.fcount = k.take<uint8_t>(N);
    w.base = k.take<uint16_t>(N * sizeof(uint16_t));
    return {w, k.total()};
}

}  // namespace

#define DQO_TSDF_CHECK_DIMS(nx, ny, nz)                                                                                    \
    do {                                                                                                                   \
        DQO_CHECK_ARG(ts_dims_ok(nx, ny, nz), "bad dims %d x %d x %d: every side is at least 2", nx, ny, nz);              \
        DQO_CHECK_ARG(ts_count_ok(nx, ny, nz), "too many voxels: %d x %d x %d is not below 2^28", nx, ny, nz);             \
    } while (0)

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_tsdf_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return ts_dims_ok(nx, ny, nz) && ts_count_ok(nx, ny, nz) ? ts_ws(nullptr, (size_t)nx * ny * nz).total : 0;
}

DQO_API int dqo_tsdf_clear(int32_t nx, int32_t ny, int32_t nz, float* tsdf, float* weight, float* color, int32_t* header, void* stream) {
    DQO_TSDF_CHECK_DIMS(nx, ny, nz);
    DQO_CHECK_ARG(tsdf && weight && color && header, "null volume buffer / header");
    const TsdfGrid g = ts_grid(nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f);
    DQO_LAUNCH("tsdf_clear_kernel", tsdf_clear_kernel, dim3((unsigned)ts_blocks(g.N)), dim3(256), (hipStream_t)stream, g.N, tsdf, weight, color,
               header);
    return DQO_OK;
}

DQO_API int dqo_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_length,
                               float sdf_trunc, float* tsdf, float* weight, float* color, int32_t* header, int32_t W, int32_t H,
                               const float* depth, const float* image, float fx, float fy, float cx, float cy, const float* w2c,
                               float depth_trunc, const DqoRastHeader* render_header, void* stream) {
    DQO_TSDF_CHECK_DIMS(nx, ny, nz);
    DQO_CHECK_ARG(voxel_length > 0.0f && sdf_trunc > 0.0f, "bad voxel_length / sdf_trunc: both are above 0");
    DQO_CHECK_ARG(tsdf && weight && color && header, "null volume buffer / header");
    DQO_CHECK_ARG(W >= 1 && H >= 1 && (int64_t)W * H < (1ll << 31), "bad image size");
    DQO_CHECK_ARG(depth && image && w2c, "null depth / color / w2c");
    const TsdfGrid g = ts_grid(nx, ny, nz, origin_x, origin_y, origin_z, voxel_length);
    const size_t tiles = (size_t)((nx + 63) / 64) * (size_t)((ny + 3) / 4) * (size_t)nz;  // (<= nx ny nz < 2^28)
    DQO_LAUNCH("tsdf_integrate_kernel", tsdf_integrate_kernel, dim3((unsigned)tiles), dim3(256), (hipStream_t)stream, g, sdf_trunc, tsdf,
               weight, color, header, W, H, depth, image, fx, fy, cx, cy, w2c, depth_trunc, render_header);
    return DQO_OK;
}

DQO_API int dqo_tsdf_extract(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_length,
                             const float* tsdf, const float* weight, const float* color, float* vertices, float* vertex_color, int32_t* faces,
                             int32_t cap_vertices, int32_t cap_faces, int32_t* header, void* workspace, size_t workspace_bytes, void* stream) {
    DQO_TSDF_CHECK_DIMS(nx, ny, nz);
    DQO_CHECK_ARG(tsdf && weight && color && header, "null volume buffer / header");
    DQO_CHECK_ARG(cap_vertices >= 0 && cap_faces >= 0, "bad capacity: %d vertices, %d faces", cap_vertices, cap_faces);
    DQO_CHECK_ARG((cap_vertices == 0 || (vertices && vertex_color)) && (cap_faces == 0 || faces), "null mesh buffer");
    const TsdfGrid g = ts_grid(nx, ny, nz, origin_x, origin_y, origin_z, voxel_length);
    DQO_CHECK_WS("tsdf", workspace, workspace_bytes, ts_ws(nullptr, g.N).total);
    const TsdfWs w = ts_ws(workspace, g.N).w;
    const dim3 grid((unsigned)ts_spans(g.N)), block(256);
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("tsdf_flags_kernel", tsdf_flags_kernel, dim3((unsigned)ts_blocks(g.N)), block, s, g, tsdf, weight, w.flags);
    DQO_LAUNCH("tsdf_edges_kernel", tsdf_edges_kernel, grid, block, s, g, w);
    DQO_LAUNCH("tsdf_vertices_kernel", tsdf_vertices_kernel, grid, block, s, g, w, tsdf, color, vertices, vertex_color, (uint32_t)cap_vertices,
               (uint32_t)cap_faces, header);
    DQO_LAUNCH("tsdf_faces_kernel", tsdf_faces_kernel, grid, block, s, g, w, faces, (uint32_t)cap_vertices, (uint32_t)cap_faces);
    return DQO_OK;
}

}  // extern "C"
