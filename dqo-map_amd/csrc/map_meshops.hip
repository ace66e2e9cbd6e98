// Mesh clean-up for gfx950 on the indexed mesh dqo_tsdf_extract leaves (map_tsdf.hip): connected components and the filtered mesh,
// simplification by vertex clustering, Laplacian / Taubin smoothing, area-weighted vertex normals — what a SLAM mesh pipeline does with open3d's cluster_connected_triangles +
// remove_triangles_by_mask + remove_unreferenced_vertices, simplify_vertex_clustering, filter_smooth_laplacian / filter_smooth_taubin (the reference's
// configs/Cube_Diorama_base.yaml:45-46 names mesh_smooth_iter: 10, mesh_smooth_lambda: 0.5) and compute_vertex_normals.  open3d does not
// exist on this platform, so the rules of include/dqo_raster.h are the definition (they follow open3d's published algorithms; the
// departures are listed there) and tests/mesh_ops_oracle.py and tests/mesh_simplify_oracle.py restate them in numpy; nothing is pinned against the library.
//
// The operand: vertices float32 [cap_v,3], colors float32 [cap_v,3] (may be NULL), faces int32 [cap_f,3], counts = a device pointer to
// two int32 (vertices, faces; NULL: the capacities are the counts; a count is clamped to [0, capacity]).  Rows behind the counts are never
// read and never written; grids are sized from the capacities, so the launch count is a fixed function of the arguments: no host read, no
// synchronise, no memset (what must be zero is cleared by a launch), no float atomics.  Blocks are 256 threads.  A face is VALID iff its
// three indices lie in [0, V).
//
// dqo_mesh_components — eleven launches:
//   init      parent[v] = v, size[v] = 0, mark[v] = 0, header = 0;
//   prelink   parent[x] = min(parent[x], the smallest index of a valid face that names x) by atomicMin, nothing returned, then a first
//   flatten   — a forest of the right sets already, whose trees end in local minima.  Without the two the hook took 1.14 ms on the mesh
//             of a 256^3 room scan (514 k faces in lattice order: long chains of dependent reads), with them 0.29 ms (profiles/mesh_ops.txt);
//   hook      a lock-free union-find over `parent`: a valid face unites (a, b) and (a, c); a union finds both roots with path halving and
//             links the LARGER root under the smaller by a returning CAS that expects the root to still be one.  parent[x] <= x always, so
//             the final root of a set is its smallest vertex id whatever order the hardware ran in.  Bad faces are counted, one integer
//             atomic per wave that has any;
//   flatten   parent[v] = root(v), by a walk that stores nothing: v's own thread is the only writer of parent[v], so it is final;
//   label     label[f] = parent[a] (-1: a bad face), size[root] += 1 — aggregated first: a lane carries (root, count) over the eight
//             faces it visits and hands it on only when the root changes, and a wave issues ONE atomic per distinct root among its lanes
//             (a mesh that is one big component costs one same-address atomic per 512 faces, not one per face);
//   stats     components (roots with size > 0) and the largest size: block partials, folded by the launch's last block (dqo_reduce.h);
//   fcount    threshold = max(min_faces, largest_only ? largest : 0); keep[f] = label >= 0 && size[label] >= threshold; the vertices of a
//             kept face are marked; the spans' kept counts, scanned by the last block (dqo_scan_block_counts) -> header[1], [7];
//   vcount    the spans' marked-vertex counts and kept-component counts, scanned -> header[0], [6], [3];
//   vscatter  marked vertices, in order, to their dense new ids (positions and colours copied bit for bit); mark[v] becomes the new id;
//   fscatter  kept faces, in order, renumbered.
// dqo_mesh_smooth / dqo_mesh_normals share one CSR build (five launches), templated on what a corner contributes: its two other
// vertices (neighbours) or its face:
//   zero      deg[v] = 0;
//   count     deg[vertex of a corner of a valid face] += entries (integer atomics on scattered addresses);
//   scan      a vertex's exclusive count within its span of 2048 and the spans' totals, scanned by the last block;
//   fill      every corner takes its slots through the vertex's own count as a cursor (atomicSub; the order inside a segment is racy here);
//   tidy      every segment is sorted ascending; neighbours also lose their duplicates and the vertex itself.  After it nothing depends on
//             the race.  Up to 32 raw entries (a marching-tetrahedra vertex has at most 20): an insertion sort by the vertex's thread.
//             More: the vertex's block sorts it with a bitonic network (the same-direction form, which takes any length) — in LDS up to
//             2048 entries, in place in global memory beyond — and compacts it with block scans.
// dqo_mesh_simplify — open3d's simplify_vertex_clustering with the Average contraction — twelve launches, no device-wide sort:
//   clear     the two tables to -1 (their slots: the power of two that is at least twice the COUNT, so a small mesh in large buffers
//             clears and probes a small table), the member counts, the marks and the header to 0, by a bounded grid that strides;
//   cells     a vertex's cell from its position in double; an open-addressed table of vertex ids with linear probing:
//             atomicCAS(slot, -1, v) claims an empty slot; an occupant of the same cell — recomputed from the immutable positions —
//             makes it atomicMin(slot, v); another cell's sends it on.  A slot's cell never changes, so the slot ends at the cluster's
//             smallest vertex id whatever order the hardware ran in.  The vertex keeps its slot.  Vertices outside the grid are counted;
//   faces     a face is bad, outside, collapsed (counted, one integer atomic per span of 2048 faces that has any) or live; a live
//             face's representatives, rotated so that the smallest comes first, go to the workspace and are marked (plain stores of 1);
//   ftable    the same table over the live faces, keyed by the rotated triple; an occupant's triple is read from what `faces` wrote,
//             which is why the two are two launches;
//   number    a marked representative's rank within its span; the spans' totals scanned by the last block -> header[0], [2];
//   members   every in-grid vertex of a written cluster takes the cluster's id and adds one to its member count;
//   scan      mesh_csr_scan_kernel with the written clusters as the segment owners (its counts: the header);
//   fill      members into their cluster's segment through the count as a cursor;
//   order     every member list ascending: up to 2048 members, each member counts the ids below its own and takes that place (one
//             thread per member: a clustering at a few voxels has thousands of lists of a hundred, which the CSR's tidy would sort
//             one after the other on a few blocks — it took 1.31 ms of a 1.95 ms call at four voxels, profiles/mesh_ops.txt); longer
//             lists by their cluster's block with the tidy's bitonic network in global memory;
//   average   one thread per written cluster: the sum in double over the ascending members, divided, rounded once;
//   keep      a live face is kept iff its slot holds its own index; the spans' kept counts scanned -> header[1], [7];
//   scatter   kept faces, in order, renumbered.
//   Every probe loop ends after as many steps as the table has slots; a table of twice the entries always has an empty one.
// Then smoothing runs one thread per vertex per step (a gather over the segment, double arithmetic, ping-pong between the mesh and the
// workspace, a copy back after an odd number of steps), normals one thread per vertex.  Every double statement is the one written,
// rounded once, none contracted (the Makefile states -ffp-contract=off); sqrt and `/` on doubles are the correctly rounded ones.
#include "dqo_common.h"
#include "dqo_mesh_operand.h"
#include "dqo_reduce.h"

namespace {

typedef unsigned long long u64;

enum {
    MO_THREAD_MAX = 32,   // tidy: raw entries a single thread sorts
    MO_LDS_MAX = 2048,    // tidy: raw entries a block sorts in LDS
    MO_CLEAR_BLOCKS = 2048,  // simplify: the most blocks of its clearing launch
};

__device__ __forceinline__ int32_t mo_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mo_st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- components -------------------------------------------------------------------------------------------------------------------------
struct MoComp {
    int32_t* head;
    int32_t* parent;   // [cap_v]
    int32_t* size;     // [cap_v] faces of the component whose root this vertex is
    int32_t* mark;     // [cap_v] 1: a kept face names the vertex; after vscatter: its new id
    int32_t* label;    // [cap_f] (the caller's, or the workspace's)
    uint8_t* keep;     // [cap_f]
    u64* spair;        // [spans of cap_v] stats: components | largest << 32 of the span
    u64* vpair;        // [spans of cap_v] marked vertices | kept components << 32
    uint32_t* fblock;  // [spans of cap_f] kept faces
};

// the root of x, with path halving.  parent[y] <= y, and a vertex that is no root never becomes one again: the store below only ever
// replaces an ancestor of a non-root by another ancestor, and no CAS of mo_unite succeeds on a non-root.  That keeps the SETS right under
// any interleaving; it does not keep parent[x] moving towards the root — a store formed from older loads can land behind a newer one
// and put a farther ancestor back.  So whoever needs THE root walks for it (mo_unite, the final flatten's mo_root)
__device__ __forceinline__ int32_t mo_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = mo_ld(parent + x);
        if (p == x) return x;
        const int32_t gp = mo_ld(parent + p);
        if (gp != p) mo_st(parent + x, gp);
        x = gp;
    }
}

__device__ __forceinline__ void mo_unite(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = mo_find(parent, a), rb = mo_find(parent, b);
    while (ra != rb) {
        if (ra < rb) {
            const int32_t t = ra;
            ra = rb, rb = t;
        }
        const int32_t old = atomicCAS(parent + ra, ra, rb);  // the larger root under the smaller, if it still is a root
        if (old == ra) return;
        ra = mo_find(parent, old), rb = mo_find(parent, rb);
    }
}

__global__ __launch_bounds__(256) void mesh_comp_init_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoComp w,
                                                             int32_t* __restrict__ header) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 8u) header[i] = 0;
    if (i >= mo_count(counts, 0, cap_v)) return;
    w.parent[i] = (int32_t)i, w.size[i] = 0, w.mark[i] = 0;
}

// before the hook: every vertex of a valid face is linked to the face's smallest index if that is below its parent (atomicMin on
// scattered addresses, nothing returned).  parent[x] <= x still holds and a parent lies in its child's component, so this is a forest of
// the right sets already; flattened once, it leaves the hook little more than the unions between the local minima's trees.
__global__ __launch_bounds__(256) void mesh_comp_prelink_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                                uint32_t cap_v, uint32_t cap_f, MoComp w) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    if (f >= F) return;
    int32_t a, b, c;
    if (!mo_face(faces, f, V, a, b, c)) return;
    const int32_t m = min(a, min(b, c));
    if (a != m) atomicMin(w.parent + a, m);
    if (b != m) atomicMin(w.parent + b, m);
    if (c != m) atomicMin(w.parent + c, m);
}

__global__ __launch_bounds__(256) void mesh_comp_hook_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                             uint32_t cap_v, uint32_t cap_f, MoComp w, int32_t* __restrict__ header) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    bool bad = false;
    if (f < F) {
        int32_t a, b, c;
        if (mo_face(faces, f, V, a, b, c)) {
            if (a != b) mo_unite(w.parent, a, b);
            if (a != c) mo_unite(w.parent, a, c);
        } else bad = true;
    }
    const int n = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&header[4], n);
}

// the root of x by a walk that stores nothing
__device__ __forceinline__ int32_t mo_root(const int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = mo_ld(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// parent[i] = root(i).  FINAL (behind the hook; the label launch takes parent[a] as the root without a find): the walk stores nothing, so
// parent[i] has ONE writer in the launch, thread i, and what it writes is the root — no union runs beside it, a root stays one, and
// whatever a walk reads on its way (an older ancestor, or a root another thread has just written) lies on the path to the same root.
// A halving walk here could leave parent[i] short of the root: thread j, passing through i, reads parent[i] and parent[parent[i]],
// thread i writes the root in between, and j's late store puts the nearer ancestor back.  The first flatten (behind prelink) only
// shortens paths for the hook, which finds for itself, and keeps the halving.
template <bool FINAL>
__global__ __launch_bounds__(256) void mesh_comp_flatten_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoComp w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= mo_count(counts, 0, cap_v)) return;
    mo_st(w.parent + i, FINAL ? mo_root(w.parent, (int32_t)i) : mo_find(w.parent, (int32_t)i));
}

// size[root] += cnt for the lanes with `active`, one atomic per distinct root of the wave.  Called by every lane of the wave.
__device__ __forceinline__ void mo_wave_add(int32_t* size, int32_t root, uint32_t cnt, bool active, int lane) {
    u64 todo = __ballot(active);
    while (todo != 0ull) {  // (wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t r = __shfl(root, leader);
        const bool same = active && root == r;
        const uint32_t total = dqo_wave_sum_u32(same ? cnt : 0u, lane);
        if (lane == leader) atomicAdd(&size[r], (int32_t)total);
        todo &= ~__ballot(same);
    }
}

__global__ __launch_bounds__(256) void mesh_comp_label_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                              uint32_t cap_v, uint32_t cap_f, MoComp w) {
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    const int lane = threadIdx.x & 63;
    int32_t held = -1;  // the root this lane is counting for, and how many faces so far
    uint32_t held_n = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        int32_t r = -1;
        if (f < F) {
            int32_t a, b, c;
            if (mo_face(faces, f, V, a, b, c)) r = w.parent[a];
            w.label[f] = r;
        }
        const bool flush = held_n != 0u && r >= 0 && r != held;
        mo_wave_add(w.size, held, held_n, flush, lane);
        if (flush) held_n = 0u;
        if (r >= 0) held = r, held_n++;
    }
    mo_wave_add(w.size, held, held_n, held_n != 0u, lane);
}

// the block's sum of n and maximum of mx, for every thread.  s8: 8 words of LDS.
__device__ __forceinline__ void mo_block_sum_max(uint32_t& n, uint32_t& mx, uint32_t* s8) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    n = dqo_wave_sum_u32(n, lane), mx = dqo_wave_max_u32(mx, lane);
    __syncthreads();  // (s8 may still be read by the previous call)
    if (lane == 0) s8[wave] = n, s8[4 + wave] = mx;
    __syncthreads();
    n = (s8[0] + s8[1]) + (s8[2] + s8[3]);
    mx = max(max(s8[4], s8[5]), max(s8[6], s8[7]));
}

__global__ __launch_bounds__(256) void mesh_comp_stats_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoComp w,
                                                              int32_t* __restrict__ header) {
    __shared__ uint32_t s8[8];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v);
    uint32_t n = 0u, mx = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        if (i < V && w.parent[i] == (int32_t)i) {
            const uint32_t s = (uint32_t)w.size[i];
            if (s != 0u) n++, mx = max(mx, s);
        }
    }
    mo_block_sum_max(n, mx, s8);
    if (threadIdx.x == 0) __hip_atomic_store(&w.spair[blockIdx.x], (u64)n | ((u64)mx << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    n = 0u, mx = 0u;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += 256u) {
        const u64 p = __hip_atomic_load(&w.spair[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n += (uint32_t)p, mx = max(mx, (uint32_t)(p >> 32));
    }
    mo_block_sum_max(n, mx, s8);
    if (threadIdx.x == 0) header[2] = (int32_t)n, header[5] = (int32_t)mx;
}

__device__ __forceinline__ int32_t mo_threshold(const int32_t* header, int32_t min_faces, int32_t largest_only) {
    const int32_t largest = largest_only ? header[5] : 0;
    return min_faces > largest ? min_faces : largest;
}

__global__ __launch_bounds__(256) void mesh_comp_fcount_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                               uint32_t cap_f, MoComp w, int32_t min_faces, int32_t largest_only,
                                                               int32_t* __restrict__ header) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_last;
    const uint32_t F = mo_count(counts, 1, cap_f);
    const int32_t thr = mo_threshold(header, min_faces, largest_only);
    uint32_t run = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        uint32_t keep = 0u;
        if (f < F) {
            const int32_t l = w.label[f];
            keep = (l >= 0 && w.size[l] >= thr) ? 1u : 0u;
            w.keep[f] = (uint8_t)keep;
            if (keep) {  // (a labelled face: its indices are in range)
                w.mark[faces[3 * (size_t)f]] = 1, w.mark[faces[3 * (size_t)f + 1]] = 1, w.mark[faces[3 * (size_t)f + 2]] = 1;
            }
        }
        uint32_t total;
        dqo_block_exclusive<uint32_t>(keep, total, s_wave);
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.fblock[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const uint32_t kept = dqo_scan_block_counts<uint32_t, 4>(w.fblock, gridDim.x, 1, s_wave);
    if (threadIdx.x == 0) header[1] = (int32_t)kept, header[7] = (int32_t)(F - (uint32_t)header[4] - kept);
}

__global__ __launch_bounds__(256) void mesh_comp_vcount_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoComp w, int32_t min_faces,
                                                               int32_t largest_only, int32_t* __restrict__ header) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v);
    const int32_t thr = mo_threshold(header, min_faces, largest_only);
    u64 pair = 0ull;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        if (i >= V) break;
        pair += (u64)(uint32_t)w.mark[i];
        if (w.parent[i] == (int32_t)i) {
            const int32_t s = w.size[i];
            if (s > 0 && s >= thr) pair += 1ull << 32;
        }
    }
    u64 total;
    dqo_block_exclusive<u64>(pair, total, s_wave);
    if (threadIdx.x == 0) __hip_atomic_store(&w.vpair[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.vpair, gridDim.x, 1, s_wave);
    if (threadIdx.x == 0) header[0] = (int32_t)(uint32_t)sums, header[6] = (int32_t)(V - (uint32_t)sums), header[3] = (int32_t)(sums >> 32);
}

__global__ __launch_bounds__(256) void mesh_comp_vscatter_kernel(const float* __restrict__ vertices, const float* __restrict__ colors,
                                                                 const int32_t* __restrict__ counts, uint32_t cap_v, MoComp w,
                                                                 float* __restrict__ out_vertices, float* __restrict__ out_colors) {
    // (vpair's low word: the marked vertices of the spans before this one)
    mo_scatter_vertices(vertices, colors, mo_count(counts, 0, cap_v), w.mark, (uint32_t)w.vpair[blockIdx.x], out_vertices, out_colors);
}

__global__ __launch_bounds__(256) void mesh_comp_fscatter_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                                 uint32_t cap_f, MoComp w, int32_t* __restrict__ out_faces) {
    mo_scatter_faces(faces, mo_count(counts, 1, cap_f), w.keep, w.mark, w.fblock[blockIdx.x], out_faces);
}

// ---- the CSR of a vertex's neighbours (NBR) or of its corners' faces ----------------------------------------------------------------------
struct MoCsr {
    int32_t* head;
    uint32_t* deg;   // [cap_v + 1] raw entries (count), the fill's cursor (fill), the tidied entries (tidy)
    uint32_t* off;   // [cap_v + 1] raw entries of the span's vertices before this one
    uint32_t* span;  // [spans of cap_v + 1] raw entries of the span, then of the spans before it
    int32_t* adj;    // [6 cap_f] (NBR) or [3 cap_f]
};

__device__ __forceinline__ size_t mo_start(const MoCsr& c, uint32_t v) { return (size_t)c.span[v >> MO_SPAN_SHIFT] + (size_t)c.off[v]; }

__global__ __launch_bounds__(256) void mesh_csr_zero_kernel(uint32_t cap_v, MoCsr c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= cap_v) c.deg[i] = 0u;
}

template <bool NBR>
__global__ __launch_bounds__(256) void mesh_csr_count_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                             uint32_t cap_v, uint32_t cap_f, MoCsr c) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    if (f >= F) return;
    int32_t a, b, d;
    if (!mo_face(faces, f, V, a, b, d)) return;
    const uint32_t e = NBR ? 2u : 1u;
    atomicAdd(&c.deg[a], e), atomicAdd(&c.deg[b], e), atomicAdd(&c.deg[d], e);
}

__global__ __launch_bounds__(256) void mesh_csr_scan_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoCsr c) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v);
    uint32_t run = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        const uint32_t n = i < V ? c.deg[i] : 0u;
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>(n, total, s_wave);
        if (i <= V) c.off[i] = run + before;  // (V itself: the end of the last segment)
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&c.span[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(c.head, &s_last)) return;
    dqo_scan_block_counts<uint32_t, 4>(c.span, gridDim.x, 1, s_wave);  // (<= 6 cap_f < 2^32)
}

template <bool NBR>
__global__ __launch_bounds__(256) void mesh_csr_fill_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                            uint32_t cap_v, uint32_t cap_f, MoCsr c) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    if (f >= F) return;
    int32_t idx[3];
    if (!mo_face(faces, f, V, idx[0], idx[1], idx[2])) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)idx[k], e = NBR ? 2u : 1u;
        const size_t at = mo_start(c, v) + (size_t)(atomicSub(&c.deg[v], e) - e);  // (the count launch added e for this corner)
        if (NBR) c.adj[at] = idx[(k + 1) % 3], c.adj[at + 1] = idx[(k + 2) % 3];
        else c.adj[at] = (int32_t)f;
    }
}

// a[0 .. n) ascending, by the block: the bitonic network whose merges compare i with its mirror image first, so that every comparator
// puts the smaller value at the lower index — entries behind n then act as +infinity without being there, and any n sorts
__device__ __forceinline__ void mo_block_sort(int32_t* a, uint32_t n) {
    u64 npow = 1ull;
    while (npow < (u64)n) npow <<= 1;
    for (u64 k = 2ull; k <= npow; k <<= 1) {
        const u64 half = k >> 1;
        for (u64 t = threadIdx.x; t < (npow >> 1); t += 256ull) {
            const u64 lo = ((t & ~(half - 1ull)) << 1) + (t & (half - 1ull)), hi = ((t & ~(half - 1ull)) << 1) + (k - 1ull) - (t & (half - 1ull));
            if (hi < (u64)n) {
                const int32_t x = a[lo], y = a[hi];
                if (x > y) a[lo] = y, a[hi] = x;
            }
        }
        __syncthreads();
        for (u64 s = k >> 2; s >= 1ull; s >>= 1) {
            for (u64 t = threadIdx.x; t < (npow >> 1); t += 256ull) {
                const u64 lo = ((t & ~(s - 1ull)) << 1) + (t & (s - 1ull)), hi = lo + s;
                if (hi < (u64)n) {
                    const int32_t x = a[lo], y = a[hi];
                    if (x > y) a[lo] = y, a[hi] = x;
                }
            }
            __syncthreads();
        }
    }
}

template <bool NBR>
__global__ __launch_bounds__(256) void mesh_csr_tidy_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoCsr c) {
    __shared__ int32_t s_sort[MO_LDS_MAX];
    __shared__ uint32_t s_queue[256];
    __shared__ uint32_t s_nq;
    __shared__ uint32_t s_wave[4];
    const uint32_t V = mo_count(counts, 0, cap_v);
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x == 0) s_nq = 0u;
    __syncthreads();
    if (v < V) {
        const size_t start = mo_start(c, v);
        const uint32_t n = (uint32_t)(mo_start(c, v + 1u) - start);
        if (n <= (uint32_t)MO_THREAD_MAX) {
            int32_t* a = c.adj + start;
            for (uint32_t i = 1; i < n; i++) {
                const int32_t x = a[i];
                uint32_t j = i;
                for (; j > 0u && a[j - 1u] > x; j--) a[j] = a[j - 1u];
                a[j] = x;
            }
            uint32_t m = n;
            if (NBR) {
                m = 0u;
                for (uint32_t i = 0; i < n; i++) {
                    const int32_t x = a[i];
                    if (x != (int32_t)v && (m == 0u || a[m - 1u] != x)) a[m++] = x;
                }
            }
            c.deg[v] = m;
        } else s_queue[atomicAdd(&s_nq, 1u)] = v;
    }
    __syncthreads();
    const uint32_t nq = s_nq;
    for (uint32_t q = 0; q < nq; q++) {  // the block's long segments, one after the other, by the whole block
        const uint32_t u = s_queue[q];
        const size_t start = mo_start(c, u);
        const uint32_t n = (uint32_t)(mo_start(c, u + 1u) - start);
        int32_t* a = c.adj + start;
        if (n <= (uint32_t)MO_LDS_MAX) {
            for (uint32_t j = threadIdx.x; j < n; j += 256u) s_sort[j] = a[j];
            __syncthreads();
            mo_block_sort(s_sort, n);
            for (uint32_t j = threadIdx.x; j < n; j += 256u) a[j] = s_sort[j];
        } else mo_block_sort(a, n);
        __syncthreads();
        uint32_t m = n;
        if (NBR) {
            // in place: an entry moves to an index that is not above its own, a run of 256 is read before it is written, and the one entry
            // a run reads from the run before it (its last) can only have been overwritten by itself
            m = 0u;
            for (uint32_t base = 0; base < n; base += 256u) {
                const uint32_t j = base + threadIdx.x;
                int32_t x = 0;
                uint32_t keep = 0u;
                if (j < n) {
                    x = a[j];
                    keep = (x != (int32_t)u && (j == 0u || a[j - 1u] != x)) ? 1u : 0u;
                }
                uint32_t total;
                const uint32_t before = dqo_block_exclusive<uint32_t>(keep, total, s_wave);  // (its barriers: the reads are done)
                if (keep) a[m + before] = x;
                m += total;
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) c.deg[u] = m;
        __syncthreads();  // (s_sort is free again)
    }
}

// ---- smoothing --------------------------------------------------------------------------------------------------------------------------
// One step with factor lam for every vertex (include/dqo_raster.h states the rule): in double from the float32 values of `src`, sums
// left to right over the ascending neighbours.  POS / COL: which of the two arrays the step moves; the weights always come from p_src.
template <bool POS, bool COL>
__global__ __launch_bounds__(256) void mesh_smooth_step_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoCsr c,
                                                               const float* __restrict__ p_src, float* __restrict__ p_dst,
                                                               const float* __restrict__ c_src, float* __restrict__ c_dst, double lam) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= mo_count(counts, 0, cap_v)) return;
    const uint32_t n = c.deg[i];
    const float pf[3] = {p_src[3 * (size_t)i], p_src[3 * (size_t)i + 1], p_src[3 * (size_t)i + 2]};
    float cf[3] = {0.f, 0.f, 0.f};
    if (COL) cf[0] = c_src[3 * (size_t)i], cf[1] = c_src[3 * (size_t)i + 1], cf[2] = c_src[3 * (size_t)i + 2];
    if (n == 0u) {  // no neighbours: copied unchanged
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (POS) p_dst[3 * (size_t)i + k] = pf[k];
            if (COL) c_dst[3 * (size_t)i + k] = cf[k];
        }
        return;
    }
    const double px = (double)pf[0], py = (double)pf[1], pz = (double)pf[2];
    const int32_t* a = c.adj + mo_start(c, i);
    double Sx = 0.0, Sy = 0.0, Sz = 0.0, Cx = 0.0, Cy = 0.0, Cz = 0.0, T = 0.0;
    for (uint32_t k = 0; k < n; k++) {
        const size_t nb = (size_t)a[k];
        const double qx = (double)p_src[3 * nb], qy = (double)p_src[3 * nb + 1], qz = (double)p_src[3 * nb + 2];
        const double dx = px - qx, dy = py - qy, dz = pz - qz;
        const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
        const double w = 1.0 / (dist + 1e-12);
        if (POS) Sx = Sx + w * qx, Sy = Sy + w * qy, Sz = Sz + w * qz;
        if (COL) Cx = Cx + w * (double)c_src[3 * nb], Cy = Cy + w * (double)c_src[3 * nb + 1], Cz = Cz + w * (double)c_src[3 * nb + 2];
        T = T + w;
    }
    if (POS) {
        p_dst[3 * (size_t)i] = (float)(px + lam * (Sx / T - px));
        p_dst[3 * (size_t)i + 1] = (float)(py + lam * (Sy / T - py));
        p_dst[3 * (size_t)i + 2] = (float)(pz + lam * (Sz / T - pz));
    }
    if (COL) {
        const double cx = (double)cf[0], cy = (double)cf[1], cz = (double)cf[2];
        c_dst[3 * (size_t)i] = (float)(cx + lam * (Cx / T - cx));
        c_dst[3 * (size_t)i + 1] = (float)(cy + lam * (Cy / T - cy));
        c_dst[3 * (size_t)i + 2] = (float)(cz + lam * (Cz / T - cz));
    }
}

// after an odd number of steps: the workspace's half back into the mesh (a or b may be NULL)
__global__ __launch_bounds__(256) void mesh_smooth_copy_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, const float* __restrict__ a_src,
                                                               float* __restrict__ a_dst, const float* __restrict__ b_src,
                                                               float* __restrict__ b_dst) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= mo_count(counts, 0, cap_v)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (a_src != nullptr) a_dst[3 * (size_t)i + k] = a_src[3 * (size_t)i + k];
        if (b_src != nullptr) b_dst[3 * (size_t)i + k] = b_src[3 * (size_t)i + k];
    }
}

// ---- normals ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ counts, uint32_t cap_v, MoCsr c,
                                                           float* __restrict__ normals) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= mo_count(counts, 0, cap_v)) return;
    const uint32_t n = c.deg[i];
    const int32_t* a = c.adj + mo_start(c, i);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t k = 0; k < n; k++) {  // ascending face index; a face that names the vertex twice is there twice
        const size_t f = (size_t)a[k];
        const size_t i0 = (size_t)faces[3 * f], i1 = (size_t)faces[3 * f + 1], i2 = (size_t)faces[3 * f + 2];
        const double p0x = (double)vertices[3 * i0], p0y = (double)vertices[3 * i0 + 1], p0z = (double)vertices[3 * i0 + 2];
        const double ux = (double)vertices[3 * i1] - p0x, uy = (double)vertices[3 * i1 + 1] - p0y, uz = (double)vertices[3 * i1 + 2] - p0z;
        const double vx = (double)vertices[3 * i2] - p0x, vy = (double)vertices[3 * i2 + 1] - p0y, vz = (double)vertices[3 * i2 + 2] - p0z;
        sx = sx + (uy * vz - uz * vy), sy = sy + (uz * vx - ux * vz), sz = sz + (ux * vy - uy * vx);
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    float nx = 0.f, ny = 0.f, nz = 1.f;
    if (len > 0.0 && len <= 1.7976931348623157e308) nx = (float)(sx / len), ny = (float)(sy / len), nz = (float)(sz / len);
    normals[3 * (size_t)i] = nx, normals[3 * (size_t)i + 1] = ny, normals[3 * (size_t)i + 2] = nz;
}

// ---- simplification by vertex clustering ------------------------------------------------------------------------------------------------
struct MoSimp {
    int32_t* head;
    int32_t* vtab;     // [slots of cap_v] the vertex table: -1, or the smallest vertex id so far of the slot's cell
    int32_t* vslot;    // [cap_v] a vertex's slot of vtab (-1: outside the grid)
    int32_t* mark;     // [cap_v] 1: a live face names the cluster whose representative this vertex is
    int32_t* cnum;     // [cap_v] a written representative's rank among those of its span (-1: none)
    int32_t* vcid;     // [cap_v] the written cluster a vertex is a member of (-1: none)
    int32_t* sorted;   // [cap_v] the member lists of up to MO_LDS_MAX entries, ascending (the longer ones: sorted in the CSR's adj)
    int32_t* ftab;     // [slots of cap_f] the face table: -1, or the lowest face index so far of the slot's rotated triple
    int32_t* fslot;    // [cap_f] a live face's slot of ftab (-1: not live)
    int32_t* ftri;     // [cap_f,3] a live face's representatives, the smallest first
    u64* vspan;        // [spans of cap_v] written clusters | clusters formed << 32 of the span, then of the spans before it
    uint32_t* fspan;   // [spans of cap_f] kept faces, likewise
    double voxel, org[3];
};

// the slots of a table for n entries: the power of two that is at least 2 n (n < 2^28), so an empty slot always ends a probe
__host__ __device__ inline uint32_t mo_slots(uint32_t n) {
    uint32_t s = 2u;
    while (s < 2u * n) s <<= 1;
    return s;
}

__device__ __forceinline__ u64 mo_mix(u64 x) {  // (splitmix64's finaliser)
    x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27, x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the cell of vertex v as 21 bits an axis; false: outside the grid
__device__ __forceinline__ bool mo_cell(const float* __restrict__ vertices, uint32_t v, const MoSimp& w, u64& key) {
#pragma clang fp contract(off)
    key = 0ull;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double t = ((double)vertices[3 * (size_t)v + a] - w.org[a]) / w.voxel;
        const double i = floor(t);  // (NaN fails both comparisons; an infinite t is its own floor and fails one)
        in = in && i >= 0.0 && i < 2097152.0;
        key = (key << 21) | (u64)(in ? (uint32_t)i : 0u);
    }
    return in;
}

// (a grid of at most MO_CLEAR_BLOCKS blocks strides over what the COUNTS need: the capacities' tables may be a hundred times that)
__global__ __launch_bounds__(256) void mesh_simp_clear_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, uint32_t cap_f, MoSimp w,
                                                              uint32_t* __restrict__ deg, int32_t* __restrict__ header) {
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    const uint32_t sv = mo_slots(V), sf = mo_slots(F), n = max(max(sv, sf), 8u);  // (above V, and the header's eight words even when V = F = 0)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        if (i < sv) w.vtab[i] = -1;
        if (i < sf) w.ftab[i] = -1;
        if (i < V) w.mark[i] = 0;
        if (i <= V) deg[i] = 0u;
        if (i < 8u) header[i] = 0;
    }
}

// A vertex enters the table at the first slot of its cell's probe sequence that is empty or holds a vertex of its cell.  A slot's cell
// never changes (a replacement has the same cell) and a slot never empties, so every vertex of a cell ends in the same slot, and the
// slot's final value is the cell's smallest vertex id whatever order the hardware ran in.  Relaxed agent-scope atomics: the argument
// needs the order of the accesses to ONE word only; the positions an occupant's cell is recomputed from are never written.
__global__ __launch_bounds__(256) void mesh_simp_cells_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ counts,
                                                              uint32_t cap_v, MoSimp w, int32_t* __restrict__ header) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const uint32_t V = mo_count(counts, 0, cap_v);
    bool outside = false;
    if (v < V) {
        int32_t slot = -1;
        u64 key;
        if (mo_cell(vertices, v, w, key)) {
            const uint32_t mask = mo_slots(V) - 1u;
            uint32_t s = (uint32_t)mo_mix(key) & mask;
            for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {  // (bounded: a bug cannot spin)
                const int32_t occ = atomicCAS(w.vtab + s, -1, (int32_t)v);
                if (occ == -1) {
                    slot = (int32_t)s;
                    break;
                }
                u64 other;
                if ((uint32_t)occ < V && mo_cell(vertices, (uint32_t)occ, w, other) && other == key) {
                    if (occ > (int32_t)v) atomicMin(w.vtab + s, (int32_t)v);
                    slot = (int32_t)s;
                    break;
                }
            }
        }
        w.vslot[v] = slot;
        outside = slot < 0;
    }
    const int n = __popcll(__ballot(outside));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&header[3], n);
}

__device__ __forceinline__ void mo_wave_count(int32_t* word, bool pred) {  // (every lane of the wave calls it)
    const int n = __popcll(__ballot(pred));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(word, n);
}

// the representative of the cluster of v (-1: v is outside the grid)
__device__ __forceinline__ int32_t mo_rep(const MoSimp& w, int32_t v) {
    const int32_t s = w.vslot[v];
    return s < 0 ? -1 : w.vtab[s];
}

__global__ __launch_bounds__(256) void mesh_simp_faces_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ counts,
                                                              uint32_t cap_v, uint32_t cap_f, MoSimp w, int32_t* __restrict__ header) {
    __shared__ uint32_t s_n[3];
    const uint32_t V = mo_count(counts, 0, cap_v), F = mo_count(counts, 1, cap_f);
    if (threadIdx.x < 3u) s_n[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t n[3] = {0u, 0u, 0u};  // bad, outside, collapsed
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        if (f >= F) break;
        int32_t a, b, c;
        bool live = false;
        if (!mo_face(faces, f, V, a, b, c)) n[0]++;
        else {
            const int32_t ra = mo_rep(w, a), rb = mo_rep(w, b), rc = mo_rep(w, c);
            if (ra < 0 || rb < 0 || rc < 0) n[1]++;
            else if (ra == rb || rb == rc || ra == rc) n[2]++;
            else {
                live = true;
                int32_t t0 = ra, t1 = rb, t2 = rc;  // rotated, the smallest first: the orientation stays
                if (rb < ra && rb < rc) t0 = rb, t1 = rc, t2 = ra;
                else if (rc < ra && rc < rb) t0 = rc, t1 = ra, t2 = rb;
                w.ftri[3 * (size_t)f] = t0, w.ftri[3 * (size_t)f + 1] = t1, w.ftri[3 * (size_t)f + 2] = t2;
                w.mark[t0] = 1, w.mark[t1] = 1, w.mark[t2] = 1;
            }
        }
        w.fslot[f] = live ? 0 : -1;  // (a live face's slot: by the next launch)
    }
    // a span's counts: the waves' sums into LDS, then one integer atomic per word that is not zero — a mesh whose faces nearly all
    // collapse would otherwise send one same-address atomic per wave
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t t = dqo_wave_sum_u32(n[k], lane);
        if (lane == 0 && t != 0u) atomicAdd(&s_n[k], t);
    }
    __syncthreads();
    if (threadIdx.x < 3u && s_n[threadIdx.x] != 0u) atomicAdd(&header[4 + threadIdx.x], (int32_t)s_n[threadIdx.x]);
}

// The vertex table's protocol over the live faces, keyed by the rotated triple.  An occupant's triple is read from ftri, which the
// launch before this one wrote: nothing is ordered inside this launch but the accesses to one slot.
__global__ __launch_bounds__(256) void mesh_simp_ftable_kernel(const int32_t* __restrict__ counts, uint32_t cap_f, MoSimp w,
                                                               int32_t* __restrict__ header) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const uint32_t F = mo_count(counts, 1, cap_f);
    bool lost = false;
    if (f < F && w.fslot[f] >= 0) {  // live: mesh_simp_faces_kernel wrote its triple
        const int32_t t0 = w.ftri[3 * (size_t)f], t1 = w.ftri[3 * (size_t)f + 1], t2 = w.ftri[3 * (size_t)f + 2];
        const uint32_t mask = mo_slots(F) - 1u;
        uint32_t s = (uint32_t)mo_mix(mo_mix(((u64)(uint32_t)t0 << 32) | (u64)(uint32_t)t1) ^ (u64)(uint32_t)t2) & mask;
        int32_t slot = -1;
        for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
            const int32_t occ = atomicCAS(w.ftab + s, -1, (int32_t)f);
            if (occ == -1) {
                slot = (int32_t)s;
                break;
            }
            if ((uint32_t)occ < F && w.ftri[3 * (size_t)occ] == t0 && w.ftri[3 * (size_t)occ + 1] == t1 && w.ftri[3 * (size_t)occ + 2] == t2) {
                if (occ > (int32_t)f) atomicMin(w.ftab + s, (int32_t)f);
                slot = (int32_t)s;
                break;
            }
        }
        w.fslot[f] = slot;
        lost = slot < 0;  // (a full table: never, with twice the slots; the face then counts as bad)
    }
    mo_wave_count(&header[4], lost);
}

// cnum[v] = the rank of v among its span's written representatives; the spans' totals, scanned by the last block -> header[0], [2]
__global__ __launch_bounds__(256) void mesh_simp_number_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoSimp w,
                                                               int32_t* __restrict__ header) {
    __shared__ u64 s_wave[4];
    __shared__ int s_last;
    const uint32_t V = mo_count(counts, 0, cap_v);
    u64 run = 0ull;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t i = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        u64 pair = 0ull;
        if (i < V && mo_rep(w, (int32_t)i) == (int32_t)i) pair = (1ull << 32) | (u64)(uint32_t)w.mark[i];
        u64 total;
        const u64 before = dqo_block_exclusive<u64>(pair, total, s_wave);
        if (i < V) w.cnum[i] = (uint32_t)pair != 0u ? (int32_t)(uint32_t)(run + before) : -1;
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.vspan[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const u64 sums = dqo_scan_block_counts<u64, 2>(w.vspan, gridDim.x, 1, s_wave);
    if (threadIdx.x == 0) header[0] = (int32_t)(uint32_t)sums, header[2] = (int32_t)(sums >> 32);
}

// vcid[v] = the written cluster v is a member of, whose member count goes up by one
__global__ __launch_bounds__(256) void mesh_simp_members_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoSimp w,
                                                                uint32_t* __restrict__ deg) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= mo_count(counts, 0, cap_v)) return;
    const int32_t r = mo_rep(w, (int32_t)v);
    int32_t cid = -1;
    if (r >= 0 && w.cnum[r] >= 0) {
        cid = (int32_t)((uint32_t)w.vspan[(uint32_t)r >> MO_SPAN_SHIFT] + (uint32_t)w.cnum[r]);  // (<= r < cap_v)
        atomicAdd(&deg[cid], 1u);
    }
    w.vcid[v] = cid;
}

// the CSR's fill with the cluster as the segment's owner (the order inside a segment is racy here; mesh_simp_order_kernel ends that)
__global__ __launch_bounds__(256) void mesh_simp_fill_kernel(const int32_t* __restrict__ counts, uint32_t cap_v, MoSimp w, MoCsr c) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= mo_count(counts, 0, cap_v)) return;
    const int32_t cid = w.vcid[v];
    if (cid < 0) return;
    c.adj[mo_start(c, (uint32_t)cid) + (size_t)(atomicSub(&c.deg[cid], 1u) - 1u)] = (int32_t)v;
}

// The member lists in ascending order.  Clustering at a few voxels leaves thousands of lists of tens to hundreds of members: the CSR's
// tidy, which hands every list above 32 entries to its vertex's whole block, one after the other, would run them on a handful of
// blocks.  Here thread i is first VERTEX i: the member of a list of up to MO_LDS_MAX entries counts the entries below its own id —
// its place — and writes itself there in `sorted` (ids are distinct; one thread per member, the reads of a list shared by its
// members).  Then it is CLUSTER i: a longer list is queued, and the block sorts its queue in place in the raw list with the bitonic
// network of the CSR's tidy.  The two touch different lists.  mo_members() below picks the array by the length.
__global__ __launch_bounds__(256) void mesh_simp_order_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ header,
                                                              uint32_t cap_v, MoSimp w, MoCsr c) {
    __shared__ uint32_t s_queue[256];
    __shared__ uint32_t s_nq;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x == 0) s_nq = 0u;
    __syncthreads();
    if (i < mo_count(counts, 0, cap_v)) {
        const int32_t cid = w.vcid[i];
        if (cid >= 0) {
            const size_t start = mo_start(c, (uint32_t)cid);
            const uint32_t n = (uint32_t)(mo_start(c, (uint32_t)cid + 1u) - start);
            if (n <= (uint32_t)MO_LDS_MAX) {
                const int32_t* a = c.adj + start;
                uint32_t below = 0u;
                for (uint32_t j = 0; j < n; j++) below += a[j] < (int32_t)i ? 1u : 0u;
                w.sorted[start + below] = (int32_t)i;
            }
        }
    }
    if (i < mo_count(header, 0, cap_v) && (uint32_t)(mo_start(c, i + 1u) - mo_start(c, i)) > (uint32_t)MO_LDS_MAX) s_queue[atomicAdd(&s_nq, 1u)] = i;
    __syncthreads();
    const uint32_t nq = s_nq;
    for (uint32_t q = 0; q < nq; q++) {
        const size_t start = mo_start(c, s_queue[q]);
        mo_block_sort(c.adj + start, (uint32_t)(mo_start(c, s_queue[q] + 1u) - start));  // (every stage ends in a barrier)
    }
}

// cluster k's members, ascending, and their number
__device__ __forceinline__ const int32_t* mo_members(const MoSimp& w, const MoCsr& c, uint32_t k, uint32_t& n) {
    const size_t start = mo_start(c, k);
    n = (uint32_t)(mo_start(c, k + 1u) - start);
    return (n <= (uint32_t)MO_LDS_MAX ? w.sorted : c.adj) + start;
}

// one thread per written cluster: S = 0, S = S + (double)x over the members in ascending id, (float)(S / n); one member: copied
__global__ __launch_bounds__(256) void mesh_simp_average_kernel(const float* __restrict__ vertices, const float* __restrict__ colors,
                                                                const int32_t* __restrict__ header, uint32_t cap_v, MoSimp w, MoCsr c,
                                                                float* __restrict__ out_vertices, float* __restrict__ out_colors) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= mo_count(header, 0, cap_v)) return;
    uint32_t n;
    const int32_t* a = mo_members(w, c, k, n);
    if (n == 1u) {
        const size_t m = (size_t)a[0];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            out_vertices[3 * (size_t)k + j] = vertices[3 * m + j];
            if (colors != nullptr) out_colors[3 * (size_t)k + j] = colors[3 * m + j];
        }
        return;
    }
    double S[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < n; i++) {
        const size_t m = (size_t)a[i];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S[j] = S[j] + (double)vertices[3 * m + j];
            if (colors != nullptr) C[j] = C[j] + (double)colors[3 * m + j];
        }
    }
    const double dn = (double)n;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        out_vertices[3 * (size_t)k + j] = (float)(S[j] / dn);
        if (colors != nullptr) out_colors[3 * (size_t)k + j] = (float)(C[j] / dn);
    }
}

// a live face is kept iff its slot holds its own index; the spans' kept counts, scanned by the last block -> header[1], [7]
__global__ __launch_bounds__(256) void mesh_simp_keep_kernel(const int32_t* __restrict__ counts, uint32_t cap_f, MoSimp w,
                                                             int32_t* __restrict__ header) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_last;
    const uint32_t F = mo_count(counts, 1, cap_f);
    uint32_t run = 0u;
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        uint32_t keep = 0u;
        if (f < F) {
            const int32_t s = w.fslot[f];
            keep = (s >= 0 && w.ftab[s] == (int32_t)f) ? 1u : 0u;
        }
        uint32_t total;
        dqo_block_exclusive<uint32_t>(keep, total, s_wave);
        run += total;
    }
    if (threadIdx.x == 0) __hip_atomic_store(&w.fspan[blockIdx.x], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dqo_last_block(w.head, &s_last)) return;
    const uint32_t kept = dqo_scan_block_counts<uint32_t, 4>(w.fspan, gridDim.x, 1, s_wave);
    if (threadIdx.x == 0) {
        header[1] = (int32_t)kept;
        header[7] = (int32_t)(F - (uint32_t)header[4] - (uint32_t)header[5] - (uint32_t)header[6] - kept);  // live faces that are not kept
    }
}

__global__ __launch_bounds__(256) void mesh_simp_scatter_kernel(const int32_t* __restrict__ counts, uint32_t cap_f, MoSimp w,
                                                                int32_t* __restrict__ out_faces) {
    __shared__ uint32_t s_wave[4];
    const uint32_t F = mo_count(counts, 1, cap_f);
    uint32_t run = w.fspan[blockIdx.x];
    for (uint32_t chunk = 0; chunk < (uint32_t)MO_CHUNKS; chunk++) {
        const uint32_t f = (blockIdx.x * (uint32_t)MO_CHUNKS + chunk) * 256u + threadIdx.x;
        uint32_t keep = 0u;
        if (f < F) {
            const int32_t s = w.fslot[f];
            keep = (s >= 0 && w.ftab[s] == (int32_t)f) ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t before = dqo_block_exclusive<uint32_t>(keep, total, s_wave);
        if (keep != 0u) {
            const size_t o = (size_t)run + before;  // (<= f)
#pragma unroll
            for (int j = 0; j < 3; j++) out_faces[3 * o + j] = w.vcid[w.ftri[3 * (size_t)f + j]];  // (a representative is a member of its cluster)
        }
        run += total;
    }
}

// the ticket words | parent | size | mark | label | keep | spair | vpair | fblock
inline DqoLayout<MoComp> mo_comp_ws(void* base, size_t cv, size_t cf) {
    MoComp w;
    DqoCarver k(base);
    w.head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.parent = k.take<int32_t>(cv * 4);
    w.size = k.take<int32_t>(cv * 4);
    w.mark = k.take<int32_t>(cv * 4);
    w.label = k.take<int32_t>(cf * 4);
    w.keep = k.take<uint8_t>(cf);
    w.spair = k.take<u64>(mo_spans(cv) * sizeof(u64));
    w.vpair = k.take<u64>(mo_spans(cv) * sizeof(u64));
    w.fblock = k.take<uint32_t>(mo_spans(cf) * 4);
    return {w, k.total()};
}

// deg | off | span | adj (`entries` of it), from wherever the carver stands; the ticket words are the caller's
inline MoCsr mo_csr_take(DqoCarver& k, int32_t* head, size_t cv, size_t entries) {
    MoCsr c;
    c.head = head;
    c.deg = k.take<uint32_t>((cv + 1) * 4);
    c.off = k.take<uint32_t>((cv + 1) * 4);
    c.span = k.take<uint32_t>(mo_spans(cv + 1) * 4);
    c.adj = k.take<int32_t>(entries * 4);
    return c;
}

// smoothing (6 entries a face) and normals (3): the ticket words | the CSR | with `pingpong`, the positions' and the colours' other half
struct MoCsrWs {
    MoCsr c;
    float *other_p, *other_c;
    size_t total;
};
inline MoCsrWs mo_csr_ws(void* base, size_t cv, size_t cf, size_t per_face, bool pingpong) {
    DqoCarver k(base);
    int32_t* const head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    const MoCsr c = mo_csr_take(k, head, cv, per_face * cf);
    float* const other_p = pingpong ? k.take<float>(cv * 12) : nullptr;
    float* const other_c = pingpong ? k.take<float>(cv * 12) : nullptr;
    return {c, other_p, other_c, k.total()};
}

// the ticket words | MoSimp's arrays in the order of the struct | the members' CSR, which shares the ticket words (adj: one entry a vertex)
struct MoSimpWs {
    MoSimp w;
    MoCsr c;
    size_t total;
};
inline MoSimpWs mo_simp_ws(void* base, size_t cv, size_t cf) {
    MoSimp w = {};
    DqoCarver k(base);
    w.head = k.take_raw<int32_t>(DQO_REDUCE_HEAD_WORDS * 4);
    w.vtab = k.take<int32_t>((size_t)mo_slots((uint32_t)cv) * 4);
    w.vslot = k.take<int32_t>(cv * 4);
    w.mark = k.take<int32_t>(cv * 4);
    w.cnum = k.take<int32_t>(cv * 4);
    w.vcid = k.take<int32_t>(cv * 4);
    w.sorted = k.take<int32_t>(cv * 4);
    w.ftab = k.take<int32_t>((size_t)mo_slots((uint32_t)cf) * 4);
    w.fslot = k.take<int32_t>(cf * 4);
    w.ftri = k.take<int32_t>(cf * 12);
    w.vspan = k.take<u64>(mo_spans(cv) * sizeof(u64));
    w.fspan = k.take<uint32_t>(mo_spans(cf) * 4);
    return {w, mo_csr_take(k, w.head, cv, cv), k.total()};
}

// the five launches of the CSR build
template <bool NBR>
int mo_build_csr(const int32_t* faces, const int32_t* counts, uint32_t cv, uint32_t cf, const MoCsr& c, hipStream_t s) {
    const dim3 block(256), gv((unsigned)mo_blocks((size_t)cv + 1)), gf((unsigned)mo_blocks(cf));
    DQO_LAUNCH("mesh_csr_zero_kernel", mesh_csr_zero_kernel, gv, block, s, cv, c);
    DQO_LAUNCH("mesh_csr_count_kernel", mesh_csr_count_kernel<NBR>, gf, block, s, faces, counts, cv, cf, c);
    DQO_LAUNCH("mesh_csr_scan_kernel", mesh_csr_scan_kernel, dim3((unsigned)mo_spans((size_t)cv + 1)), block, s, counts, cv, c);
    DQO_LAUNCH("mesh_csr_fill_kernel", mesh_csr_fill_kernel<NBR>, gf, block, s, faces, counts, cv, cf, c);
    DQO_LAUNCH("mesh_csr_tidy_kernel", mesh_csr_tidy_kernel<NBR>, dim3((unsigned)mo_blocks(cv)), block, s, counts, cv, c);
    return DQO_OK;
}

}  // namespace

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

DQO_API size_t dqo_mesh_components_workspace_bytes(int32_t cap_vertices, int32_t cap_faces) {
    return mo_caps_ok(cap_vertices, cap_faces) ? mo_comp_ws(nullptr, (size_t)cap_vertices, (size_t)cap_faces).total : 0;
}

DQO_API size_t dqo_mesh_smooth_workspace_bytes(int32_t cap_vertices, int32_t cap_faces) {
    return mo_caps_ok(cap_vertices, cap_faces) ? mo_csr_ws(nullptr, (size_t)cap_vertices, (size_t)cap_faces, 6, true).total : 0;
}

DQO_API size_t dqo_mesh_normals_workspace_bytes(int32_t cap_vertices, int32_t cap_faces) {
    return mo_caps_ok(cap_vertices, cap_faces) ? mo_csr_ws(nullptr, (size_t)cap_vertices, (size_t)cap_faces, 3, false).total : 0;
}

DQO_API size_t dqo_mesh_simplify_workspace_bytes(int32_t cap_vertices, int32_t cap_faces) {
    return mo_caps_ok(cap_vertices, cap_faces) ? mo_simp_ws(nullptr, (size_t)cap_vertices, (size_t)cap_faces).total : 0;
}

DQO_API int dqo_mesh_simplify(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                              int32_t cap_faces, double voxel_size, double origin_x, double origin_y, double origin_z, float* out_vertices,
                              float* out_colors, int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* header,
                              void* workspace, size_t workspace_bytes, void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(voxel_size - voxel_size == 0.0 && voxel_size > 0.0, "bad voxel_size: it is finite and above 0");
    DQO_CHECK_ARG(origin_x - origin_x == 0.0 && origin_y - origin_y == 0.0 && origin_z - origin_z == 0.0, "bad origin: it is finite");
    DQO_MESH_CHECK_OUT();
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh simplify", workspace, workspace_bytes, mo_simp_ws(nullptr, cv, cf).total);
    const uint32_t ucv = (uint32_t)cap_vertices, ucf = (uint32_t)cap_faces;
    const MoSimpWs l = mo_simp_ws(workspace, cv, cf);
    MoSimp w = l.w;
    const MoCsr& c = l.c;
    w.voxel = voxel_size, w.org[0] = origin_x, w.org[1] = origin_y, w.org[2] = origin_z;
    const size_t slots = mo_slots(ucv) > mo_slots(ucf) ? mo_slots(ucv) : mo_slots(ucf);
    const size_t clear_blocks = mo_blocks(slots) < (size_t)MO_CLEAR_BLOCKS ? mo_blocks(slots) : (size_t)MO_CLEAR_BLOCKS;
    const dim3 block(256), gv((unsigned)mo_blocks(cv)), gf((unsigned)mo_blocks(cf)), sv((unsigned)mo_spans(cv)), sf((unsigned)mo_spans(cf));
    hipStream_t s = (hipStream_t)stream;
    // the segment owners of the CSR are the written clusters: the header's word 0 is its launches' vertex count
    DQO_LAUNCH("mesh_simp_clear_kernel", mesh_simp_clear_kernel, dim3((unsigned)clear_blocks), block, s, counts, ucv, ucf, w, c.deg, header);
    DQO_LAUNCH("mesh_simp_cells_kernel", mesh_simp_cells_kernel, gv, block, s, vertices, counts, ucv, w, header);
    DQO_LAUNCH("mesh_simp_faces_kernel", mesh_simp_faces_kernel, sf, block, s, faces, counts, ucv, ucf, w, header);
    DQO_LAUNCH("mesh_simp_ftable_kernel", mesh_simp_ftable_kernel, gf, block, s, counts, ucf, w, header);
    DQO_LAUNCH("mesh_simp_number_kernel", mesh_simp_number_kernel, sv, block, s, counts, ucv, w, header);
    DQO_LAUNCH("mesh_simp_members_kernel", mesh_simp_members_kernel, gv, block, s, counts, ucv, w, c.deg);
    DQO_LAUNCH("mesh_csr_scan_kernel", mesh_csr_scan_kernel, dim3((unsigned)mo_spans(cv + 1)), block, s, (const int32_t*)header, ucv, c);
    DQO_LAUNCH("mesh_simp_fill_kernel", mesh_simp_fill_kernel, gv, block, s, counts, ucv, w, c);
    DQO_LAUNCH("mesh_simp_order_kernel", mesh_simp_order_kernel, gv, block, s, counts, (const int32_t*)header, ucv, w, c);
    DQO_LAUNCH("mesh_simp_average_kernel", mesh_simp_average_kernel, gv, block, s, vertices, colors, (const int32_t*)header, ucv, w, c,
               out_vertices, out_colors);
    DQO_LAUNCH("mesh_simp_keep_kernel", mesh_simp_keep_kernel, sf, block, s, counts, ucf, w, header);
    DQO_LAUNCH("mesh_simp_scatter_kernel", mesh_simp_scatter_kernel, sf, block, s, counts, ucf, w, out_faces);
    return DQO_OK;
}

DQO_API int dqo_mesh_components(const float* vertices, const float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices,
                                int32_t cap_faces, int32_t min_faces, int32_t largest_only, float* out_vertices, float* out_colors,
                                int32_t* out_faces, int32_t out_cap_vertices, int32_t out_cap_faces, int32_t* labels, int32_t* header,
                                void* workspace, size_t workspace_bytes, void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && header, "null mesh buffer / header");
    DQO_CHECK_ARG(min_faces >= 0, "bad min_faces %d: it is at least 0", min_faces);
    DQO_MESH_CHECK_OUT();
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh components", workspace, workspace_bytes, mo_comp_ws(nullptr, cv, cf).total);
    MoComp w = mo_comp_ws(workspace, cv, cf).w;
    if (labels != nullptr) w.label = labels;  // (the part is taken all the same: the size does not depend on the option)
    const uint32_t ucv = (uint32_t)cap_vertices, ucf = (uint32_t)cap_faces;
    const dim3 block(256), gv((unsigned)mo_blocks(cv)), gf((unsigned)mo_blocks(cf)), sv((unsigned)mo_spans(cv)), sf((unsigned)mo_spans(cf));
    hipStream_t s = (hipStream_t)stream;
    DQO_LAUNCH("mesh_comp_init_kernel", mesh_comp_init_kernel, gv, block, s, counts, ucv, w, header);
    DQO_LAUNCH("mesh_comp_prelink_kernel", mesh_comp_prelink_kernel, gf, block, s, faces, counts, ucv, ucf, w);
    DQO_LAUNCH("mesh_comp_flatten_kernel", mesh_comp_flatten_kernel<false>, gv, block, s, counts, ucv, w);
    DQO_LAUNCH("mesh_comp_hook_kernel", mesh_comp_hook_kernel, gf, block, s, faces, counts, ucv, ucf, w, header);
    DQO_LAUNCH("mesh_comp_flatten_kernel", mesh_comp_flatten_kernel<true>, gv, block, s, counts, ucv, w);
    DQO_LAUNCH("mesh_comp_label_kernel", mesh_comp_label_kernel, sf, block, s, faces, counts, ucv, ucf, w);
    DQO_LAUNCH("mesh_comp_stats_kernel", mesh_comp_stats_kernel, sv, block, s, counts, ucv, w, header);
    DQO_LAUNCH("mesh_comp_fcount_kernel", mesh_comp_fcount_kernel, sf, block, s, faces, counts, ucf, w, min_faces, largest_only, header);
    DQO_LAUNCH("mesh_comp_vcount_kernel", mesh_comp_vcount_kernel, sv, block, s, counts, ucv, w, min_faces, largest_only, header);
    DQO_LAUNCH("mesh_comp_vscatter_kernel", mesh_comp_vscatter_kernel, sv, block, s, vertices, colors, counts, ucv, w, out_vertices, out_colors);
    DQO_LAUNCH("mesh_comp_fscatter_kernel", mesh_comp_fscatter_kernel, sf, block, s, faces, counts, ucf, w, out_faces);
    return DQO_OK;
}

DQO_API int dqo_mesh_smooth(float* vertices, float* colors, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                            int32_t iterations, double lambda, double mu, int32_t scope, void* workspace, size_t workspace_bytes,
                            void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces, "null mesh buffer");
    DQO_CHECK_ARG(iterations >= 0, "bad iterations %d: at least 0", iterations);
    DQO_CHECK_ARG(lambda == lambda && mu == mu && lambda - lambda == 0.0 && mu - mu == 0.0, "bad lambda / mu: both are finite");
    DQO_CHECK_ARG(scope >= DQO_MESH_SMOOTH_POSITIONS && scope <= DQO_MESH_SMOOTH_BOTH, "bad scope %d: 0 positions, 1 colours, 2 both", scope);
    DQO_CHECK_ARG(scope == DQO_MESH_SMOOTH_POSITIONS || colors, "null colors with a scope that smooths them");
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh smooth", workspace, workspace_bytes, mo_csr_ws(nullptr, cv, cf, 6, true).total);
    if (iterations == 0) return DQO_OK;
    const MoCsrWs l = mo_csr_ws(workspace, cv, cf, 6, true);
    const MoCsr& c = l.c;
    float *const other_p = l.other_p, *const other_c = l.other_c;
    const uint32_t ucv = (uint32_t)cap_vertices, ucf = (uint32_t)cap_faces;
    hipStream_t s = (hipStream_t)stream;
    const int rc = mo_build_csr<true>(faces, counts, ucv, ucf, c, s);
    if (rc != DQO_OK) return rc;
    const bool pos = scope != DQO_MESH_SMOOTH_COLOURS, col = scope != DQO_MESH_SMOOTH_POSITIONS;
    const dim3 block(256), gv((unsigned)mo_blocks(cv));
    const int steps = mu != 0.0 ? 2 * iterations : iterations;
    float *p_cur = vertices, *p_nxt = other_p, *c_cur = colors, *c_nxt = other_c;
    const auto step = pos && col ? mesh_smooth_step_kernel<true, true> : pos ? mesh_smooth_step_kernel<true, false> : mesh_smooth_step_kernel<false, true>;
    for (int k = 0; k < steps; k++) {
        const double lam = (mu != 0.0 && (k & 1)) ? mu : lambda;
        // (a scope's other array is read at most: positions give the weights of a colour step)
        DQO_LAUNCH("mesh_smooth_step_kernel", step, gv, block, s, counts, ucv, c, (const float*)p_cur, p_nxt, (const float*)c_cur, c_nxt, lam);
        if (pos) {
            float* t = p_cur;
            p_cur = p_nxt, p_nxt = t;
        }
        if (col) {
            float* t = c_cur;
            c_cur = c_nxt, c_nxt = t;
        }
    }
    if (steps & 1) {
        DQO_LAUNCH("mesh_smooth_copy_kernel", mesh_smooth_copy_kernel, gv, block, s, counts, ucv, pos ? other_p : nullptr, vertices,
                   col ? other_c : nullptr, colors);
    }
    return DQO_OK;
}

DQO_API int dqo_mesh_normals(const float* vertices, const int32_t* faces, const int32_t* counts, int32_t cap_vertices, int32_t cap_faces,
                             float* normals, void* workspace, size_t workspace_bytes, void* stream) {
    DQO_MESH_CHECK_CAPS(cap_vertices, cap_faces);
    DQO_CHECK_ARG(vertices && faces && normals, "null mesh buffer / normals");
    const size_t cv = (size_t)cap_vertices, cf = (size_t)cap_faces;
    DQO_CHECK_WS("mesh normals", workspace, workspace_bytes, mo_csr_ws(nullptr, cv, cf, 3, false).total);
    const MoCsr c = mo_csr_ws(workspace, cv, cf, 3, false).c;
    hipStream_t s = (hipStream_t)stream;
    const int rc = mo_build_csr<false>(faces, counts, (uint32_t)cap_vertices, (uint32_t)cap_faces, c, s);
    if (rc != DQO_OK) return rc;
    DQO_LAUNCH("mesh_normals_kernel", mesh_normals_kernel, dim3((unsigned)mo_blocks(cv)), dim3(256), s, vertices, faces, counts,
               (uint32_t)cap_vertices, c, normals);
    return DQO_OK;
}

}  // extern "C"
