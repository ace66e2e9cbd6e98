// The mesh operand of the operators that work on dqo_tsdf_extract's mesh in place of its counts (map_meshops.hip: components, smooth,
// normals, simplify; map_meshcull.hip: cull): vertices float32 [cap_v,3], colors float32 [cap_v,3] (may be NULL), faces int32 [cap_f,3]
// and counts, a device pointer to two int32 (vertices, faces; NULL: the capacities are the counts; a count is clamped to
// [0, capacity]).  Rows behind the counts are never read and never written; grids are sized from the capacities.  Here: the sizes, a
// count's and a face's read, and the ordered compaction that dqo_mesh_components and dqo_mesh_cull end with — kept faces and the
// vertices they name keep their order, are renumbered densely and are copied bit for bit.  Blocks are 256 threads.
#pragma once
#include "dqo_common.h"
#include "dqo_reduce.h"

enum {
    MO_CHUNKS = 8,        // runs of 256 items that a block of a span launch walks
    MO_SPAN_SHIFT = 11,   // a span: 2048 consecutive vertices / faces
    MO_SPAN = 1 << MO_SPAN_SHIFT,
    MO_MAX = 1 << 28,     // capacities lie below it: 6 cap_f adjacency entries stay below 2^32
};
static_assert(MO_SPAN == 256 * MO_CHUNKS, "a span is MO_CHUNKS runs of a block");

__host__ __device__ inline size_t mo_blocks(size_t n) { return (n + 255) / 256; }
__host__ __device__ inline size_t mo_spans(size_t n) { return (n + MO_SPAN - 1) / MO_SPAN; }
inline bool mo_caps_ok(int64_t cap_v, int64_t cap_f) { return cap_v >= 1 && cap_f >= 1 && cap_v < MO_MAX && cap_f < MO_MAX; }

#define DQO_MESH_CHECK_CAPS(cv, cf) \
    DQO_CHECK_ARG(mo_caps_ok(cv, cf), "bad capacity: %d vertices, %d faces: both are at least 1 and below 2^28", cv, cf)

// the out mesh and the header of dqo_mesh_components, dqo_mesh_simplify and dqo_mesh_cull, under the entries' own argument names
#define DQO_MESH_CHECK_OUT()                                                                                                                  \
    DQO_CHECK_ARG(out_cap_vertices >= cap_vertices && out_cap_faces >= cap_faces,                                                             \
                  "out capacity (%d vertices, %d faces) below the input's (%d, %d)", out_cap_vertices, out_cap_faces, cap_vertices, cap_faces); \
    DQO_CHECK_ARG(out_vertices && out_faces && (colors == nullptr || out_colors), "null out mesh buffer");                                    \
    DQO_CHECK_ARG(out_vertices != vertices && out_faces != faces && (colors == nullptr || out_colors != colors),                              \
                  "the out mesh must not be the input mesh");                                                                                 \
    DQO_CHECK_ARG(header != counts, "header must not be the input's counts: the first launch clears it before the counts are read")

__device__ __forceinline__ uint32_t mo_count(const int32_t* counts, int k, uint32_t cap) {
    if (counts == nullptr) return cap;
    const int32_t n = counts[k];
    return n <= 0 ? 0u : ((uint32_t)n < cap ? (uint32_t)n : cap);
}

__device__ __forceinline__ bool mo_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t V, int32_t& a, int32_t& b, int32_t& c) {
    a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
}

// By every thread of a block that owns span blockIdx.x of the vertices: the vertices with mark != 0 go, in order, to their dense new ids
// (positions and colours bit for bit) and mark[v] becomes the new id.  run: the marked vertices of the spans before this one.
__device__ __forceinline__ void mo_scatter_vertices(const float* __restrict__ vertices, const float* __restrict__ colors, uint32_t V,
                                                    int32_t* __restrict__ mark, uint32_t run, float* __restrict__ out_vertices,
                                                    float* __restrict__ out_colors) {
    __shared__ uint32_t s_wave[4];
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        const uint32_t m = i < V ? (uint32_t)mark[i] : 0u;
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>(m, total, s_wave);
        if (m != 0u) {
            const size_t id = (size_t)run + before;  // (<= i: inside the out buffers, whose capacities are not below the input's)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                out_vertices[3 * id + c] = vertices[3 * (size_t)i + c];
                if (colors != nullptr) out_colors[3 * id + c] = colors[3 * (size_t)i + c];
            }
            mark[i] = (int32_t)id;
        }
        run += total;
    }
}

// By every thread of a block that owns span blockIdx.x of the faces: the faces with keep != 0 go, in order, to the out list, their
// indices renumbered through mark (mo_scatter_vertices' new ids).  run: the kept faces of the spans before this one.
__device__ __forceinline__ void mo_scatter_faces(const int32_t* __restrict__ faces, uint32_t F, const uint8_t* __restrict__ keep,
                                                 const int32_t* __restrict__ mark, uint32_t run, int32_t* __restrict__ out_faces) {
    __shared__ uint32_t s_wave[4];
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        const uint32_t k = f < F ? (uint32_t)keep[f] : 0u;
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>(k, total, s_wave);
        if (k != 0u) {
            const size_t o = (size_t)run + before;  // (<= f)
#pragma unroll
            for (int c = 0; c < 3; c++) out_faces[3 * o + c] = mark[faces[3 * (size_t)f + c]];
        }
        run += total;
    }
}
