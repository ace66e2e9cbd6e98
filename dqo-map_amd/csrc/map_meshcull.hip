// Mesh evaluation for gfx950, the cull: a mesh restricted to what K views see — the frustum test and the occlusion test against the
// frames' depth that every mesh-evaluation protocol of dense SLAM (the NICE-SLAM lineage) applies to BOTH meshes before it samples them.
// Neither a reference implementation nor open3d exists on this platform, so include/dqo_raster.h (dqo_mesh_cull) defines the rule and
// tests/mesh_cull_oracle.py restates it in numpy.  The operand, the counts and the compaction rules are dqo_mesh_components'
// (dqo_mesh_operand.h, shared with map_meshops.hip): rows behind the counts are never read and never written, grids are sized from the capacities.
//
// This file is compiled with -ffp-contract=off.  Per vertex v < V and used view k, float32, one rounding per operation, left to right,
// `/` the correctly rounded one — dqo_tsdf_integrate's own statements (map_tsdf.hip), so a mesh is culled by the pixels that made it:
//     pc_r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3]              m = w2c[k], row major
//     not seen unless pc_z > near
//     u_f = ((pc_x * fx) / pc_z + cx) + 0.5f;  v_f likewise with fy, cy
//     not seen unless u_f >= 0.0001f && u_f < (float)W - 0.0001f                (the same for v_f and H)
//     depth == NULL: seen
//     else u = (int)u_f;  v = (int)v_f;  d = depth[k][v][u];  seen iff d > 0 && d <= depth_trunc && pc_z <= d + eps
// views(v) = the used views that see v.  A face is kept iff it is valid and at least min_corners of its corners have views > 0.
//
// dqo_mesh_cull — six launches of 256-thread blocks, whatever the data:
//   init      views[v] = 0, mark[v] = 0, header = 0; the used views as one bit each, 32 to a word (view_keep's bytes are read here and
//             nowhere else);
//   views     the hot path, V x n_views.  A grid over (256 vertices, MC_CHUNK = 32 views): a block holds its vertex in three VGPRs and
//             walks the set bits of its chunk's word.  The word, the view's index and its twelve matrix words are wave-uniform — scalar
//             loads into SGPRs, no LDS — and the one per-pair memory access is the gathered depth pixel.  blockIdx.x runs over the
//             vertices, so the blocks in flight share a chunk: 32 depth maps of 1200 x 680 are 104 MB, inside the 256 MiB Infinity
//             Cache, where a thread that walked all views would drag every map through it once per vertex block.  A vertex's count is
//             merged by ONE integer atomic add per (vertex, chunk) that saw it.  Without vertex_views only views > 0 matters: a wave
//             leaves its chunk once all its lanes are seen, and stores 1;
//   fcount    a face's seen corners (a repeated index counts once per corner), keep[f], the kept faces' vertices marked (plain stores
//             of 1); a span's (kept, bad) counts, scanned by the last block (dqo_reduce.h) -> header[1], [4], [5];
//   vcount    a span's (marked, seen) vertex counts, scanned -> header[0], [6], [2]; the used views' bits counted -> header[3];
//   vscatter  marked vertices, in order, to their dense new ids (positions and colours bit for bit); mark[v] becomes the new id;
//   fscatter  kept faces, in order, renumbered.
// Integer atomics only (the adds of `views`, whose sum does not depend on their order, and the tickets, which come back at zero);
// nothing is allocated, set by a memset, read back or synchronised: the entry can be captured in a hipGraph.
//
// dqo_mesh_cull_faces — visibility per FACE, by the pixels a face wins in a render of the mesh (face_index, rdepth: map_meshrender.hip's
// outputs); six launches too, in the same workspace (the per-face counts are the caller's face_pixels):
//   finit     mark[v] = 0, face_pixels[f] = 0, header = 0, the used views' bits;
//   pixels    the hot path, n_views x H x W: a pixel counts for f = face_index iff 0 <= f < F and, with the frames' depth,
//             s > 0 && s <= depth_trunc && rdepth <= s + eps — the occlusion statement above.  One integer add per RUN of one id;
//   fpix      fcount with the rule pixels(f) >= min_pixels; the faces with a pixel and the pixels -> header[2], [7];
//   vcount (without the seen vertices), vscatter, fscatter: the launches above.
#include "dqo_common.h"
#include "dqo_mesh_operand.h"
#include "dqo_reduce.h"

namespace {

typedef unsigned long long u64;

enum {
    MC_CHUNK = 32,       // views per block of the views launch: one word of used-view bits
    MC_MAX_VIEWS = 65535,
    MC_BITS_BYTES = (MC_MAX_VIEWS / MC_CHUNK + 1) * 4,  // 2048 words: a multiple of 256 bytes
};
static_assert(MC_BITS_BYTES % 256 == 0, "the workspace's parts are multiples of 256 bytes");

struct McWork {
    int32_t* head;
    int32_t* views;      // [cap_v] the caller's vertex_views, or the workspace's
    int32_t* mark;       // [cap_v] 1: a kept face names the vertex; after vscatter: its new id
    uint8_t* keep;       // [cap_f]
    u64* vpair;          // [spans of cap_v] marked vertices | seen vertices << 32
    u64* fpair;          // [spans of cap_f] kept faces | bad faces << 32
    uint32_t* viewbits;  // [chunks of n_views] bit j of word c: view 32 c + j is used
};

// The spans that have items (one at least, whose last block writes the header): a block of a span launch behind them leaves at once
// and takes no ticket — the grids are sized from the capacities, and a mesh of half a million faces in buffers of twelve million would
// otherwise pay for 5 600 empty blocks' barriers, fences and tickets (fcount 0.137 ms, vcount 0.057 ms: profiles/mesh_eval.txt).
__device__ __forceinline__ uint32_t mc_active_spans(uint32_t n) {
    const uint32_t s = (n + (uint32_t)MO_SPAN - 1u) >> MO_SPAN_SHIFT;
    return s > 0u ? s : 1u;
}

struct McCamera {
    int W, H;
    float fx, fy, cx, cy, near, eps, depth_trunc;
};

__global__ __launch_bounds__(256) void mesh_cull_init_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t n_views,
                                                             const uint8_t* __restrict__ view_keep, McWork w, int32_t* __restrict__ header) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 8u) header[i] = 0;
    if (i < (n_views + (uint32_t)MC_CHUNK - 1u) / (uint32_t)MC_CHUNK) {
        uint32_t bits = 0u;
        for (uint32_t j = 0; j < (uint32_t)MC_CHUNK; j++) {
            const uint32_t k = i * (uint32_t)MC_CHUNK + j;
            if (k < n_views && (view_keep == nullptr || view_keep[k] != 0)) bits |= 1u << j;
        }
        w.viewbits[i] = bits;
    }
    if (i >= mo_count(counts, 0, cap_v)) return;
    w.views[i] = 0, w.mark[i] = 0;
}

// DEPTH: the occlusion test against depth[k]; COUNT: views[v] is the exact count (vertex_views was asked for)
template <bool DEPTH, bool COUNT>
__global__ __launch_bounds__(256) void mesh_cull_views_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ counts,
                                                              uint32_t cap_v, const float* __restrict__ w2c,
                                                              const uint32_t* __restrict__ viewbits, const float* __restrict__ depth,
                                                              McCamera cam, int32_t* __restrict__ views) {
#pragma clang fp contract(off)
    const uint32_t V = mo_count(counts, 0, cap_v);
    if (blockIdx.x * 256u >= V) return;  // (block-uniform)
    uint32_t bits = viewbits[blockIdx.y];  // (wave-uniform: a scalar load)
    if (bits == 0u) return;
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < V;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    const float wmax = (float)cam.W - 0.0001f, hmax = (float)cam.H - 0.0001f;
    const size_t plane = (size_t)cam.W * (size_t)cam.H;
    int32_t n = 0;
    while (bits != 0u) {  // (wave-uniform)
        const uint32_t k = blockIdx.y * (uint32_t)MC_CHUNK + (uint32_t)(__ffs((int)bits) - 1);
        bits &= bits - 1u;
        const float* __restrict__ m = w2c + 16 * (size_t)k;  // (a wave-uniform address: twelve words by scalar loads)
        const float pcz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        bool seen = live && pcz > cam.near;
        if (seen) {
            const float pcx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            const float pcy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            const float uf = ((pcx * cam.fx) / pcz + cam.cx) + 0.5f, vf = ((pcy * cam.fy) / pcz + cam.cy) + 0.5f;
            seen = uf >= 0.0001f && uf < wmax && vf >= 0.0001f && vf < hmax;
            if (DEPTH && seen) {
                const int u = (int)uf, vv = (int)vf;  // (inside [0, W) x [0, H): the test above)
                const float d = depth[(size_t)k * plane + (size_t)vv * (size_t)cam.W + (size_t)u];
                seen = d > 0.0f && d <= cam.depth_trunc && pcz <= d + cam.eps;
            }
        }
        n += seen ? 1 : 0;
        if (!COUNT && __ballot(live && n == 0) == 0ull) break;  // (every lane of the wave is seen: the outputs cannot tell)
    }
    if (n == 0) return;
    if (COUNT) atomicAdd(&views[v], n);
    else views[v] = 1;  // (the same word from every chunk that saw it)
}

__global__ __launch_bounds__(256) void mesh_cull_fcount_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                               uint32_t cap_v, uint32_t cap_f, McWork w, int32_t min_corners,
                                                               int32_t* __restrict__ header) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    const uint32_t nact = mc_active_spans(F);
    if (blockIdx.x >= nact) return;
    u64 run = 0ull;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        u64 pair = 0ull;
        if (f < F) {
            int32_t a, b, c;
            if (mo_face(faces, f, V, a, b, c)) {
                const int32_t corners = (w.views[a] > 0 ? 1 : 0) + (w.views[b] > 0 ? 1 : 0) + (w.views[c] > 0 ? 1 : 0);
                if (corners >= min_corners) {
                    pair = 1ull;
                    w.mark[a] = 1, w.mark[b] = 1, w.mark[c] = 1;
                }
            } else pair = 1ull << 32;
            w.keep[f] = (uint8_t)(pair & 1ull);
        }
        u64 total;
        dqo_block_exclusive<u64>(pair, total, s_wave);
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.fpair[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last, (int)nact)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.fpair, nact, 1, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t kept = (uint32_t)sums, bad = (uint32_t)(sums >> 32);
        header[1] = (int32_t)kept, header[4] = (int32_t)bad, header[5] = (int32_t)(F - bad - kept);
    }
}

// SEEN: header[2] = the vertices with views > 0 (dqo_mesh_cull); dqo_mesh_cull_faces, which has no views, leaves the word to its fpix launch
template <bool SEEN>
__global__ __launch_bounds__(256) void mesh_cull_vcount_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t n_views, McWork w,
                                                               int32_t* __restrict__ header) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v);
    const uint32_t nact = mc_active_spans(V);
    if (blockIdx.x >= nact) return;
    u64 pair = 0ull;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        if (i >= V) break;
        pair += (u64)(uint32_t)w.mark[i];
        if (SEEN && w.views[i] > 0) pair += 1ull << 32;
    }
    u64 total;
    dqo_block_exclusive<u64>(pair, total, s_wave);
    if (threadIdx.x == 0) __hip_atomic_store(&w.vpair[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last, (int)nact)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.vpair, nact, 1, s_wave);
    u64 used = 0ull, all;
    for (uint32_t c = threadIdx.x; c < (n_views + (uint32_t)MC_CHUNK - 1u) / (uint32_t)MC_CHUNK; c += 256u) used += (u64)__popc(w.viewbits[c]);
    dqo_block_exclusive<u64>(used, all, s_wave);
    if (threadIdx.x == 0) {
        header[0] = (int32_t)(uint32_t)sums, header[6] = (int32_t)(V - (uint32_t)sums);
        if (SEEN) header[2] = (int32_t)(sums >> 32);
        header[3] = (int32_t)all;
    }
}

__global__ __launch_bounds__(256) void mesh_cull_vscatter_kernel(const float* __restrict__ vertices, const float* __restrict__ colors,
                                                                 const int32_t* __restrict__ counts, uint32_t cap_v, McWork w,
                                                                 float* __restrict__ out_vertices, float* __restrict__ out_colors) {
    const uint32_t V = mo_count(counts, 0, cap_v);
    if (blockIdx.x >= mc_active_spans(V)) return;  // (no vertex, and its pair was never written)
    // (the pairs' low words: the marked vertices / kept faces of the spans before this one)
    mo_scatter_vertices(vertices, colors, V, w.mark, (uint32_t)w.vpair[blockIdx.x], out_vertices, out_colors);
}

__global__ __launch_bounds__(256) void mesh_cull_fscatter_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                                 uint32_t cap_f, McWork w, int32_t* __restrict__ out_faces) {
    const uint32_t F = mo_count(counts, 1, cap_f);
    if (blockIdx.x >= mc_active_spans(F)) return;
    mo_scatter_faces(faces, F, w.keep, w.mark, (uint32_t)w.fpair[blockIdx.x], out_faces);
}

// ---- dqo_mesh_cull_faces: a face is kept by the pixels it wins in a render of the mesh ----
enum {
    MC_PIX_BATCH = 16,                  // rounds of 64 consecutive pixels whose loads a wave of the pixels launch issues together
    MC_PIX_ROUNDS = 4 * MC_PIX_BATCH,   // rounds that a wave walks
    MC_PIX_WAVE = 64 * MC_PIX_ROUNDS,   // a wave's pixels: consecutive, so a run of one face id goes on from round to round
    MC_PIX_BLOCK = 4 * MC_PIX_WAVE,
};

__global__ __launch_bounds__(256) void mesh_cull_finit_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t cap_f, uint32_t n_views,
                                                              const uint8_t* __restrict__ view_keep, McWork w, int32_t* __restrict__ face_pixels,
                                                              int32_t* __restrict__ header) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 8u) header[i] = 0;
    if (i < (n_views + (uint32_t)MC_CHUNK - 1u) / (uint32_t)MC_CHUNK) {
        uint32_t bits = 0u;
        for (uint32_t j = 0; j < (uint32_t)MC_CHUNK; j++) {
            const uint32_t k = i * (uint32_t)MC_CHUNK + j;
            if (k < n_views && (view_keep == nullptr || view_keep[k] != 0)) bits |= 1u << j;
        }
        w.viewbits[i] = bits;
    }
    if (i < mo_count(counts, 0, cap_v)) w.mark[i] = 0;
    if (i < mo_count(counts, 1, cap_f)) face_pixels[i] = 0;
}

// The hot path, n_views x H x W pixels: blockIdx.y is the view (its used bit a scalar load), a wave walks MC_PIX_WAVE consecutive
// pixels.  A wall wins most of a view, so an add per pixel would queue on one address: a lane shift and a ballot find the heads of
// the runs of one face id across the wave, and a run is ONE integer add; a round whose 64 pixels all continue the run of the round
// before adds nothing — the run's length rides in a scalar until the run ends.  A pixel that does not count has id -1, which ends a
// run and starts none.  DEPTH: the occlusion statement against the frames' depth.
template <bool DEPTH>
__global__ __launch_bounds__(256) void mesh_cull_pixels_kernel(const int32_t* __restrict__ counts, uint32_t cap_f,
                                                               const uint32_t* __restrict__ viewbits, size_t plane,
                                                               const int32_t* __restrict__ face_index, const float* __restrict__ rdepth,
                                                               const float* __restrict__ depth, float eps, float depth_trunc,
                                                               int32_t* __restrict__ face_pixels) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.y;
    if ((viewbits[k >> 5] >> (k & 31u) & 1u) == 0u) return;  // (block-uniform: a scalar load)
    const uint32_t F = mo_count(counts, 1, cap_f);
    const int lane = threadIdx.x & 63;
    const size_t view = (size_t)k * plane;
    const size_t first = (size_t)blockIdx.x * MC_PIX_BLOCK + (size_t)(threadIdx.x >> 6) * MC_PIX_WAVE;
    int32_t run_id = -1, run_len = 0;  // (wave-uniform) the run that the rounds so far left open
    for (int batch = 0; batch < MC_PIX_ROUNDS / MC_PIX_BATCH; batch++) {
        const size_t start = first + (size_t)batch * (64 * MC_PIX_BATCH);
        if (start >= plane) break;  // (wave-uniform)
        // the batch's loads first, none waiting for another: a round's ballot and adds would otherwise stand between two loads
        int32_t ids[MC_PIX_BATCH];
#pragma unroll
        for (int r = 0; r < MC_PIX_BATCH; r++) {
            const size_t i = start + (size_t)r * 64 + (size_t)lane;
            int32_t id = -1;
            if (i < plane) {
                const int32_t f = face_index[view + i];
                bool on = (uint32_t)f < F;  // (anything else, -1 included, is never an index)
                if (DEPTH && on) {
                    const float s = depth[view + i];
                    on = s > 0.0f && s <= depth_trunc && rdepth[view + i] <= s + eps;
                }
                if (on) id = f;
            }
            ids[r] = id;
        }
#pragma unroll
        for (int r = 0; r < MC_PIX_BATCH; r++) {
            if (start + (size_t)r * 64 >= plane) break;  // (wave-uniform)
            const int32_t id = ids[r];
            const int32_t prev = __shfl_up(id, 1);
            const bool head = lane == 0 || prev != id;
            const u64 heads = __ballot(head);
            if (heads == 1ull) {  // (wave-uniform) one id in all 64 lanes
                const int32_t id0 = __builtin_amdgcn_readfirstlane(id);
                if (id0 != run_id) {
                    if (run_id >= 0 && lane == 0) atomicAdd(&face_pixels[run_id], run_len);
                    run_id = id0, run_len = 0;
                }
                run_len += 64;
                continue;
            }
            if (run_id >= 0 && lane == 0) atomicAdd(&face_pixels[run_id], run_len);
            run_id = -1, run_len = 0;
            if (head && id >= 0) {
                const u64 above = lane < 63 ? heads >> (lane + 1) : 0ull;  // the next head ends the run
                atomicAdd(&face_pixels[id], above != 0ull ? (int32_t)__ffsll((long long)above) : 64 - lane);
            }
        }
    }
    if (run_id >= 0 && lane == 0) atomicAdd(&face_pixels[run_id], run_len);
}

// dqo_mesh_cull's fcount with the pixel rule: keep[f], the kept faces' vertices marked, a span's (kept, bad) counts scanned by the last
// block -> header[1], [4], [5]; the faces with a pixel and the pixels -> header[2], [7], one integer add per wave and word (the finit
// launch cleared them).  A bad face's count is put back to 0: a pixel counts for a valid face only.
__global__ __launch_bounds__(256) void mesh_cull_fpix_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts, uint32_t cap_v,
                                                             uint32_t cap_f, McWork w, int32_t min_pixels, int32_t* __restrict__ face_pixels,
                                                             int32_t* __restrict__ header) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    const uint32_t nact = mc_active_spans(F);
    if (blockIdx.x >= nact) return;
    const int lane = threadIdx.x & 63;
    u64 run = 0ull;
    uint32_t n_with = 0u, n_pixels = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        u64 pair = 0ull;
        if (f < F) {
            const int32_t px = face_pixels[f];
            int32_t a, b, c;
            if (mo_face(faces, f, V, a, b, c)) {
                n_with += px != 0 ? 1u : 0u, n_pixels += (uint32_t)px;
                if (px >= min_pixels) {
                    pair = 1ull;
                    w.mark[a] = 1, w.mark[b] = 1, w.mark[c] = 1;
                }
            } else {
                pair = 1ull << 32;
                if (px != 0) face_pixels[f] = 0;
            }
            w.keep[f] = (uint8_t)(pair & 1ull);
        }
        u64 total;
        dqo_block_exclusive<u64>(pair, total, s_wave);
        run += total;
    }
    n_with = dqo_wave_sum_u32(n_with, lane), n_pixels = dqo_wave_sum_u32(n_pixels, lane);
    if (lane == 0) {
        if (n_with > 0u) atomicAdd(&header[2], (int32_t)n_with);
        if (n_pixels > 0u) atomicAdd(&header[7], (int32_t)n_pixels);
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.fpair[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last, (int)nact)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.fpair, nact, 1, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t kept = (uint32_t)sums, bad = (uint32_t)(sums >> 32);
        header[1] = (int32_t)kept, header[4] = (int32_t)bad, header[5] = (int32_t)(F - bad - kept);
    }
}

// the ticket words | views | mark | keep | vpair | fpair | the used views' bits
inline DqoLayout<McWork> mc_ws(void* base, size_t cv, size_t cf) {
    McWork w;
    DqoCarver k(base);
    w.head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.views = k.take<int32_t>(cv * 4);
    w.mark = k.take<int32_t>(cv * 4);
    w.keep = k.take<uint8_t>(cf);
    w.vpair = k.take<u64>(mo_spans(cv) * sizeof(u64));
    w.fpair = k.take<u64>(mo_spans(cf) * sizeof(u64));
    w.viewbits = k.take<uint32_t>(MC_BITS_BYTES);
    return {w, k.total()};
}

}  // namespace

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_mesh_cull_workspace_bytes(int32_t cap_vertices, int32_t cap_faces) {
    return mo_caps_ok(cap_vertices, cap_faces) ? mc_ws(nullptr, (size_t)cap_vertices, (size_t)cap_faces).total : 0;
}

DQO_API int dqo_mesh_cull(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                          int32_t cap_faces, int32_t n_views, const float* w2c, const uint8_t* view_keep, int32_t W, int32_t H, float fx, float fy,
                          float cx, float cy, const float* depth, float near, float eps, float depth_trunc, int32_t min_corners,
                          float* out_vertices, float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces,
                          int32_t* vertex_views, int32_t* header, void* workspace, size_t workspace_bytes, void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(n_views >= 1 && n_views <= MC_MAX_VIEWS, "bad n_views %d: 1 to 65535 views", n_views);
    DQO_CHECK_ARG(w2c, "null w2c");
    DQO_CHECK_ARG(W >= 1 && H >= 1 && (uint64_t)W * (uint64_t)H <= ((1ull << 40) - 1ull) / (uint64_t)n_views,
                  "bad image size %d x %d for %d views: both sides are at least 1, n_views * H * W is below 2^40", W, H, n_views);
    DQO_CHECK_ARG(near - near == 0.0f && near >= 0.0f, "bad near: it is finite and at least 0");
    DQO_CHECK_ARG(eps - eps == 0.0f && eps >= 0.0f, "bad eps: it is finite and at least 0");
    DQO_CHECK_ARG(depth_trunc > 0.0f, "bad depth_trunc: it is above 0 (it may be +inf)");
    DQO_CHECK_ARG(min_corners >= 1 && min_corners <= 3, "bad min_corners %d: 1, 2 or 3", min_corners);
    DQO_MESH_CHECK_OUT();
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh cull", workspace, workspace_bytes, mc_ws(nullptr, cv, cf).total);
    McWork w = mc_ws(workspace, cv, cf).w;
    if (vertex_views != nullptr) w.views = vertex_views;  // (the part is taken all the same: the size does not depend on the option)
    McCamera cam;
    cam.W = W, cam.H = H, cam.fx = fx, cam.fy = fy, cam.cx = cx, cam.cy = cy, cam.near = near, cam.eps = eps, cam.depth_trunc = depth_trunc;
    const uint32_t ucv = (uint32_t)cap_vertices, ucf = (uint32_t)cap_faces, nv = (uint32_t)n_views;
    const size_t chunks = ((size_t)n_views + MC_CHUNK - 1) / MC_CHUNK;
    const dim3 block(256), gi((unsigned)mo_blocks(cv > chunks ? cv : chunks)), gvk((unsigned)mo_blocks(cv), (unsigned)chunks);
    const dim3 sv((unsigned)mo_spans(cv)), sf((unsigned)mo_spans(cf));
    const bool count = vertex_views != nullptr;
    auto views_kernel = depth != nullptr ? (count ? mesh_cull_views_kernel<true, true> : mesh_cull_views_kernel<true, false>)
                                         : (count ? mesh_cull_views_kernel<false, true> : mesh_cull_views_kernel<false, false>);
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("mesh_cull_init_kernel", mesh_cull_init_kernel, gi, block, s, counts, ucv, nv, view_keep, w, header);
    DQO_LAUNCH("mesh_cull_views_kernel", views_kernel, gvk, block, s, vertices, counts, ucv, w2c, (const uint32_t*)w.viewbits, depth, cam,
               w.views);
    DQO_LAUNCH("mesh_cull_fcount_kernel", mesh_cull_fcount_kernel, sf, block, s, faces, counts, ucv, ucf, w, min_corners, header);
    DQO_LAUNCH("mesh_cull_vcount_kernel", mesh_cull_vcount_kernel<true>, sv, block, s, counts, ucv, nv, w, header);
    DQO_LAUNCH("mesh_cull_vscatter_kernel", mesh_cull_vscatter_kernel, sv, block, s, vertices, colors, counts, ucv, w, out_vertices, out_colors);
    DQO_LAUNCH("mesh_cull_fscatter_kernel", mesh_cull_fscatter_kernel, sf, block, s, faces, counts, ucf, w, out_faces);
    return DQO_OK;
}

DQO_API int dqo_mesh_cull_faces(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                                int32_t cap_faces, int32_t n_views, const uint8_t* view_keep, int32_t W, int32_t H, const int32_t* face_index,
                                const float* rdepth, const float* depth, float eps, float depth_trunc, int32_t min_pixels, float* out_vertices,
                                float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* face_pixels,
                                int32_t* header, void* workspace, size_t workspace_bytes, void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(n_views >= 1 && n_views <= MC_MAX_VIEWS, "bad n_views %d: 1 to 65535 views", n_views);
    DQO_CHECK_ARG(W >= 1 && H >= 1 && (uint64_t)W * (uint64_t)H <= ((1ull << 40) - 1ull) / (uint64_t)n_views,
                  "bad image size %d x %d for %d views: both sides are at least 1, n_views * H * W is below 2^40", W, H, n_views);
    DQO_CHECK_ARG(face_index && rdepth, "null face_index / rdepth: the entry culls by a render of this mesh");
    DQO_CHECK_ARG(face_pixels, "null face_pixels");
    DQO_CHECK_ARG(eps - eps == 0.0f && eps >= 0.0f, "bad eps: it is finite and at least 0");
    DQO_CHECK_ARG(depth_trunc > 0.0f, "bad depth_trunc: it is above 0 (it may be +inf)");
    DQO_CHECK_ARG(min_pixels >= 1, "bad min_pixels %d: at least 1", min_pixels);
    DQO_MESH_CHECK_OUT();
    DQO_CHECK_ARG(face_pixels != faces && face_pixels != out_faces && face_pixels != header && face_pixels != counts,
                  "face_pixels must be a buffer of its own");
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh cull", workspace, workspace_bytes, mc_ws(nullptr, cv, cf).total);
    const McWork w = mc_ws(workspace, cv, cf).w;
    const uint32_t ucv = (uint32_t)cap_vertices, ucf = (uint32_t)cap_faces, nv = (uint32_t)n_views;
    const size_t chunks = ((size_t)n_views + MC_CHUNK - 1) / MC_CHUNK, plane = (size_t)W * (size_t)H;
    const size_t most = cv > cf ? (cv > chunks ? cv : chunks) : (cf > chunks ? cf : chunks);
    const dim3 block(256), gi((unsigned)mo_blocks(most)), gp((unsigned)((plane + MC_PIX_BLOCK - 1) / MC_PIX_BLOCK), (unsigned)n_views);
    const dim3 sv((unsigned)mo_spans(cv)), sf((unsigned)mo_spans(cf));
    auto pixels_kernel = depth != nullptr ? mesh_cull_pixels_kernel<true> : mesh_cull_pixels_kernel<false>;
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("mesh_cull_finit_kernel", mesh_cull_finit_kernel, gi, block, s, counts, ucv, ucf, nv, view_keep, w, face_pixels, header);
    DQO_LAUNCH("mesh_cull_pixels_kernel", pixels_kernel, gp, block, s, counts, ucf, (const uint32_t*)w.viewbits, plane, face_index, rdepth, depth,
               eps, depth_trunc, face_pixels);
    DQO_LAUNCH("mesh_cull_fpix_kernel", mesh_cull_fpix_kernel, sf, block, s, faces, counts, ucv, ucf, w, min_pixels, face_pixels, header);
    DQO_LAUNCH("mesh_cull_vcount_kernel", mesh_cull_vcount_kernel<false>, sv, block, s, counts, ucv, nv, w, header);
    DQO_LAUNCH("mesh_cull_vscatter_kernel", mesh_cull_vscatter_kernel, sv, block, s, vertices, colors, counts, ucv, w, out_vertices, out_colors);
    DQO_LAUNCH("mesh_cull_fscatter_kernel", mesh_cull_fscatter_kernel, sf, block, s, faces, counts, ucf, w, out_faces);
    return DQO_OK;
}

}  // extern "C"
