// The body of tile_sort_wave_kernel<LATE> and tile_sort_wave_pf_kernel (LATE = true), included by both kernels.  As an inlined function it moved the
// register allocation of the existing kernel, whose gfx950 code must not change.  In scope: the kernel's parameters and the
// compile-time PF (the parameter form: raw opacities / scales / rotations, features_dc + rest).
    if constexpr (LATE) {
        if ((int)blockIdx.x >= late.first_block) {  // (block-uniform; the sort blocks come first: the longest lists start at once)
            k1_late_block<SORTW_THREADS, PF>(late, g, (int)blockIdx.x - late.first_block, rest);
            return;
        }
    }
    __shared__ uint64_t s_key[2 * SORTP_RUN];
    __shared__ uint32_t s_val[2 * SORTP_RUN];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ti = blockIdx.x;
    // the threshold the queue is built with, for the backward: its split kernel leaves to the queue exactly the lists that are in it
    // (whatever the caller's backward context says)
    if (ti == 0 && threadIdx.x == 0) g.counters[6] = (uint32_t)list_split;
    const uint32_t tile = img.tile_order[ti];  // [8][T8] slots, unused ones hold ~0
    if (tile >= (uint32_t)T) {
        if (threadIdx.x == 0) img.slot_info[ti] = make_uint4(0xffffffffu, 0u, 0u, 0u);
        return;
    }
    uint2 rg;
    if (keep_order) {
        const uint32_t c = img.tile_count[(size_t)tile * DQO_TSTRIDE];
        // the slot tables are incomplete when the instance capacity ran out: every list is emptied, as tile_scan_kernel does; a
        // list that outgrew its bucket is cut at the bucket (bin_count_kernel dropped the rest); both invalidate the frame
        const bool lost = g.counters[7] != 0u;  // (bucket mode: a slot region ran out of its share, bin_count_kernel)
        const uint32_t n_keep = lost ? 0u : min(c, (uint32_t)bin.bucket);
        const uint32_t first = tile * (uint32_t)bin.bucket;
        rg = make_uint2(n_keep ? first : 0u, n_keep ? first + n_keep : 0u);
        if (threadIdx.x == 0) {
            img.ranges[tile] = rg;
            if (c) {
                uint32_t* const line = g.spread + (size_t)(ti % DQO_SPREAD) * 64;
                atomicMax(&line[2], c);
                atomicAdd(&line[3], 1u);
            }
        }
    } else {
        rg = img.ranges[tile];
    }
    if (threadIdx.x == 0) img.slot_info[ti] = make_uint4(tile, rg.x, rg.y, 0u);  // (DqoImageLayout.slot_info: the blend kernels' one-round head)
    const int n = (int)(rg.y - rg.x);
    if (n <= 0) return;
    // DqoRastCtx.list_split: the blend kernels' queue of lists shared between eight waves (longest first, like the one below)
    if (list_split > 0 && n > list_split && threadIdx.x == 0) img.split_tiles[atomicAdd(&g.counters[4], 1u)] = tile;
    if (n > SORTW_CAP) {  // tile_sort_kernel's: queued (the blocks run longest list first, so the queue is close to that order too)
        if (threadIdx.x == 0) img.long_tiles[atomicAdd(&g.counters[1], 1u)] = tile;
        return;
    }
    if (n > SORTP_RUN) {
        pair_sort_tile(bin, rg.x, n, lane, wave, s_key, s_val);
        return;
    }
    if (wave != 0) return;
    if (n <= 64) wave_sort_tile<1>(bin, rg.x, n, lane);
    else if (n <= 128) wave_sort_tile<2>(bin, rg.x, n, lane);
    else if (n <= 256) wave_sort_tile<4>(bin, rg.x, n, lane);
    else wave_sort_tile<8>(bin, rg.x, n, lane);
