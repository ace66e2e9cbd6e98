// The body of bin_count_kernel<K1> and bin_count_pf_kernel (K1 = true), included by both kernels.  As an inlined function it moved the
// register allocation of the existing kernel, whose gfx950 code must not change.  In scope: the kernel's parameters and the
// compile-time PF (the parameter form: raw opacities / scales / rotations, features_dc + rest).
    __shared__ uint32_t s_off[BIN_CHUNK + 1];  // exclusive prefix of the rect areas
    __shared__ uint2 s_rect[BIN_CHUNK];        // packed tile rects
    __shared__ float4 s_con[BIN_CHUNK];        // conic + opacity
    __shared__ float4 s_xyq[BIN_CHUNK];        // (pix.x, pix.y, q threshold, depth bits)
    __shared__ uint32_t s_cnt[BIN_CHUNK];      // live candidates of each Gaussian
    __shared__ uint32_t s_prev[BIN_CHUNK];     // ... of them in earlier windows (placement sweep)
    __shared__ uint32_t s_gb[BIN_CHUNK];       // exclusive prefix of s_cnt
    __shared__ uint32_t s_bits[BIN_WINDOW / 32];
    __shared__ uint32_t s_wave[BIN_THREADS / 64];
    __shared__ uint32_t s_base;
    __shared__ int s_gobj[BIN_CHUNK];          // object id (object gate only)
    const int tid = threadIdx.x;
    const uint32_t lane = lane_id(), wave = tid >> 6;
    const int chunk0 = blockIdx.x * BIN_CHUNK;
    const int my_idx = dqo_spread_index(chunk0 + tid, P);  // which Gaussian this thread owns (dqo_common.h)

    // ---- this thread's Gaussian: rect area (0 = culled by K1) and the inputs of the footprint test, parked in LDS ----
    uint32_t area = 0;
    {
        uint2 rc = make_uint2(0u, 0u);
        float4 co = make_float4(0.f, 0.f, 0.f, 0.f), xy = co;
        if constexpr (K1) {
            float view[16], proj[16];
#pragma unroll
            for (int i = 0; i < 16; i++) view[i] = k1.v.view[i], proj[i] = k1.v.proj[i];
            if (blockIdx.x == 0 && tid == 0) {
                g.header->stage = 1u;  // (the header still holds the previous frame: "stage 1" until the sort kernels rewrite it)
                // the frame_prezeroed promise: the previous frame's tail leaves a stamp behind its clearing; a frame that finds none — a
                // forward-only render, dqo_rast_backward, an error return in between — is flagged (folded into header.overflow)
                if (g.counters[9] != DQO_CLEARED_STAMP) atomicOr(&g.counters[8], 1u);
                g.counters[9] = 0u;
            }
            bool vis = false;
            uint32_t ncand = 0;
            if (my_idx < P) {
                const K1Early e = k1_early<false, PF>(k1.v, view, proj, 0.f, 0.f, 0.f, my_idx, k1.means3D, k1.scales, k1.rotations, k1.opacities,
                                                  nullptr, nullptr, k1.gobj, g, k1.radii_out, k1.n_touched_out);
                rc = make_uint2((uint32_t)e.rminx | ((uint32_t)e.rmaxx << 16), (uint32_t)e.rminy | ((uint32_t)e.rmaxy << 16));
                co = e.co, xy = e.xy;
                ncand = (uint32_t)((e.rmaxx - e.rminx) * (e.rmaxy - e.rminy));
                area = ncand;
                vis = e.radius > 0;
            }
            // visible count and (Gaussian, tile) pairs in the tile rects (the header's statistics): one pair of atomics per wave
            const uint32_t nv = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(vis));
            const uint32_t nc = dqo_wave_sum_u32(ncand, (int)lane);
            if (lane == 0 && (nv | nc) != 0u) {
                uint32_t* const my_line = g.spread + (size_t)((blockIdx.x * (BIN_THREADS / 64) + wave) % DQO_SPREAD) * 64;
                if (nv) atomicAdd(&my_line[0], nv);
                if (nc) atomicAdd(&my_line[1], nc);
            }
        } else if (my_idx < P) {
            // all three loads together (the tables of a culled Gaussian hold stale values that are never looked at): loading the
            // conic only after the rect says "visible" would put two memory latencies in series at the head of every block
            rc = g.rect16[my_idx];
            co = g.conic_opacity[my_idx];
            xy = g.xy_depth[my_idx];
            area = ((rc.x >> 16) - (rc.x & 0xffffu)) * ((rc.y >> 16) - (rc.y & 0xffffu));
        }
        s_rect[tid] = rc;
        if (area) {
            s_con[tid] = co;
            s_xyq[tid] = make_float4(xy.x, xy.y, dqo_q_threshold(co.w), xy.z);
            s_gobj[tid] = __float_as_int(xy.w);
        }
        s_cnt[tid] = 0;
        s_prev[tid] = 0;
    }
    uint32_t total;
    const uint32_t my_off = block_exclusive_scan(area, s_wave, lane, wave, &total);
    s_off[tid] = my_off;
    if (tid == BIN_THREADS - 1) s_off[BIN_CHUNK] = total;
    __syncthreads();
    if (total == 0) {  // nothing visible in this chunk
        if (my_idx < P) g.tiles_touched[my_idx] = 0, g.slot_base[my_idx] = 0;
        return;
    }

    // candidate w of the block -> (Gaussian, tile)
    auto decode = [&](uint32_t w) {
        int lo = 0, hi = BIN_CHUNK;  // largest gi with s_off[gi] <= w
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= w) lo = mid;
            else hi = mid;
        }
        const uint32_t r = w - s_off[lo];
        const uint2 rc = s_rect[lo];
        const uint32_t minx = rc.x & 0xffffu, rw = (rc.x >> 16) - minx, miny = rc.y & 0xffffu;
        const uint32_t ry = r / rw, rx = r - ry * rw;
        Cand c;
        c.gi = lo;
        c.tile = (int)((miny + ry) * (uint32_t)gx + minx + rx);
        return c;
    };
    // footprint test of every candidate of the window [win, wend) -> s_bits (and tile_flag for the dead ones)
    auto cull_window = [&](uint32_t win, uint32_t wend, bool flag_dead) {
        for (int i = tid; i < BIN_WINDOW / 32; i += BIN_THREADS) s_bits[i] = 0;
        __syncthreads();
        for (uint32_t w = win + tid; w < wend; w += BIN_THREADS) {
            const Cand c = decode(w);
            if (tile_mask != nullptr && !tile_mask[c.tile]) continue;
            const float4 co = s_con[c.gi], xyq = s_xyq[c.gi];
            const int x = c.tile % gx, y = c.tile / gx;
            bool live = dqo_splat_hits_rect(xyq.x, xyq.y, co.x, co.y, co.z, xyq.z, (float)(x * DQO_TILE), (float)(y * DQO_TILE),
                                            (float)(x * DQO_TILE + DQO_TILE - 1), (float)(y * DQO_TILE + DQO_TILE - 1));
            if (tile_objects != nullptr) live = live && ((tile_objects[c.tile] >> (s_gobj[c.gi] & 63)) & 1ull) != 0ull;
            if (live) {
                atomicOr(&s_bits[(w - win) >> 5], 1u << ((w - win) & 31));
            } else if (flag_dead && tile_flag[c.tile] == 0u) {
                // active in the reference (its list holds this dead entry): render the tile, do not leave the initial fills
                tile_flag[c.tile] = 1u;
            }
        }
        __syncthreads();
    };
    // per-Gaussian live count of the window, added to acc[]
    auto carry_window = [&](uint32_t win, uint32_t wend, uint32_t* acc) {
        const uint32_t a = max(my_off, win), b = min(my_off + area, wend);
        if (a < b) acc[tid] += popcount_range(s_bits, a - win, b - win);
    };

    // ---- sweep 1: live candidates per Gaussian ----
    const bool one_window = total <= (uint32_t)BIN_WINDOW;
    for (uint32_t win = 0; win < total; win += BIN_WINDOW) {
        const uint32_t wend = min(total, win + (uint32_t)BIN_WINDOW);
        cull_window(win, wend, true);
        carry_window(win, wend, s_cnt);
        if (!one_window) __syncthreads();  // s_bits is rebuilt by the next window
    }
    // ---- tiles_touched + gaussian-major slot allocation: block scan of the live counts, one atomic per block ----
    // A FROZEN row (DqoRastInputs.row_flags, bucket mode = the captured mapping iteration) is rendered — its list entries are written
    // below like any other's — but it is no parameter of the mapping call: its instances get NO gradient slots (slot = 0xffffffff in the
    // list record: every slot-indexed write of the backward is skipped, as it is for a slot beyond the capacity), so the backward's
    // blend kernel stores no partial gradient record for it and the per-Gaussian tail has nothing to read.
    const bool no_slots = bin.bucket > 0 && row_flags != nullptr && my_idx < P && (row_flags[my_idx] & DQO_ROW_FROZEN) != 0u;
    const uint32_t my_cnt = no_slots ? 0u : s_cnt[tid];
    __shared__ uint8_t s_noslot[BIN_CHUNK];
    s_noslot[tid] = no_slots ? (uint8_t)1 : (uint8_t)0;
    if (row_flags != nullptr && bin.bucket > 0) {  // (kernel-uniform) the header's num_rendered stays the sum of the LIST lengths
        const uint32_t nf = dqo_wave_sum_u32(no_slots ? s_cnt[tid] : 0u, (int)lane);
        if (lane == 0 && nf != 0u) atomicAdd(&g.spread[(size_t)((blockIdx.x * (BIN_THREADS / 64) + wave) % DQO_SPREAD) * 64 + 5], nf);
    }
    uint32_t block_live;
    const uint32_t my_gb = block_exclusive_scan(my_cnt, s_wave, lane, wave, &block_live);
    s_gb[tid] = my_gb;
    if (tid == 0) {
        if (block_live == 0u) {
            s_base = 0u;
        } else if (bin.bucket <= 0) {
            s_base = atomicAdd(&g.counters[0], block_live);
        } else {
            // Bucket mode (a caller that can re-run a frame): the slot space is cut into DQO_SPREAD regions with an allocator each — the
            // ONE same-address returning atomic of this kernel is otherwise taken by all ~2 000 blocks at about the same time and served
            // one per ~11 ns (same-address atomics serialise memory-side): up to 64 counters on 64 lines, 30 blocks each on cfg 3.  A region that
            // runs out of its share invalidates the frame like running out of the capacity does (counters[7]; nothing is written out of
            // bounds: the block's slots are placed past the capacity, where every slot-indexed write is skipped).
            // (at least 16 blocks per region, so that a region's load stays near the mean — the capacity is ~3x the instances kept:
            // a small map uses fewer regions, down to one)
            const uint32_t regions = min((uint32_t)DQO_SPREAD, max(1u, gridDim.x / 16u));
            const uint32_t r = blockIdx.x % regions, share = (uint32_t)(capacity / regions);
            const uint32_t off = atomicAdd(&g.spread[(size_t)r * 64 + 4], block_live);
            if (off + block_live > share) {
                g.counters[7] = 1u;
                s_base = (uint32_t)capacity;
            } else {
                s_base = r * share + off;
            }
        }
    }
    __syncthreads();
    const uint32_t base = s_base;
    if (my_idx < P) {
        g.tiles_touched[my_idx] = my_cnt;
        g.slot_base[my_idx] = base + my_gb;
    }
    if (block_live == 0) return;
    if (bin.bucket > 0) {
        // bucket mode has no placement pass to clear the validity words of the backward's partial gradient records: the block
        // clears its own contiguous slot range here, coalesced
        for (uint32_t i = tid; i < block_live; i += BIN_THREADS)
            if ((int64_t)(base + i) < capacity) bin.rec_valid[base + i] = 0u;
    }

    // ---- sweep 2: every live candidate takes its rank in its tile and records (tile, rank, Gaussian) at its slot ----
    for (uint32_t win = 0; win < total; win += BIN_WINDOW) {
        const uint32_t wend = min(total, win + (uint32_t)BIN_WINDOW);
        if (!one_window) cull_window(win, wend, false);  // (a single window's bits are still in LDS)
        for (uint32_t w0 = win + tid; w0 < wend; w0 += BIN_THREADS * BIN_FLIGHT) {
            uint32_t slot[BIN_FLIGHT], rank[BIN_FLIGHT];
            int tile[BIN_FLIGHT], gid[BIN_FLIGHT];
            float depth[BIN_FLIGHT];
            bool ok[BIN_FLIGHT];
#pragma unroll
            for (int u = 0; u < BIN_FLIGHT; u++) {
                const uint32_t w = w0 + u * BIN_THREADS;
                ok[u] = w < wend && ((s_bits[(w - win) >> 5] >> ((w - win) & 31)) & 1u);
                if (ok[u]) {
                    const Cand c = decode(w);
                    const uint32_t first = max(s_off[c.gi], win);
                    slot[u] = s_noslot[c.gi] ? 0xffffffffu : base + s_gb[c.gi] + s_prev[c.gi] + popcount_range(s_bits, first - win, w - win);
                    tile[u] = c.tile;
                    gid[u] = dqo_spread_index(chunk0 + c.gi, P);
                    depth[u] = s_xyq[c.gi].w;
                    rank[u] = atomicAdd(&tile_count[(size_t)c.tile * DQO_TSTRIDE], 1u);
                }
            }
#pragma unroll
            for (int u = 0; u < BIN_FLIGHT; u++) {
                if (ok[u] && ((int64_t)slot[u] < capacity || slot[u] == 0xffffffffu)) {
                    if (bin.bucket > 0) {
                        // fixed per-tile buckets: the rank IS the list position (what bin_place_kernel derives from the scanned
                        // ranges in the packed mode); an instance beyond the bucket is dropped — tile_scan_kernel flags the frame
                        if (rank[u] < (uint32_t)bin.bucket) {
                            const size_t pos = (size_t)tile[u] * (size_t)bin.bucket + rank[u];
                            bin.recs[pos] = make_uint4((uint32_t)gid[u], __float_as_uint(depth[u]), slot[u], 0u);
                        }
                    } else {
                        bin.slot_info[slot[u]] = make_uint2((uint32_t)tile[u], rank[u]);
                        bin.slot_gid[slot[u]] = (uint32_t)gid[u];
                    }
                }
            }
        }
        if (!one_window) {
            __syncthreads();  // the loop above still reads s_prev and s_bits
            carry_window(win, wend, s_prev);
            __syncthreads();
        }
    }
