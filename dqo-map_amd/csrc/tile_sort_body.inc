// The body of tile_sort_kernel<LATE> and tile_sort_pf_kernel (LATE = true), included by both kernels.  As an inlined function it moved the
// register allocation of the existing kernel, whose gfx950 code must not change.  In scope: the kernel's parameters and the
// compile-time PF (the parameter form: raw opacities / scales / rotations, features_dc + rest).
    if constexpr (LATE) {  // (the late part of the per-Gaussian forward behind the long-list sort blocks: dqo_k1_where == 2)
        if ((int)blockIdx.x >= late.first_block) {
            k1_late_block<SORT_THREADS, PF>(late, g, (int)blockIdx.x - late.first_block, rest);
            return;
        }
    }
    const uint32_t sort_blocks = LATE ? (uint32_t)late.first_block : gridDim.x;
    __shared__ uint64_t s_keys[SORTL_SEG];
    __shared__ uint32_t s_vals[SORTL_SEG];
    if (keep_order && blockIdx.x == 0 && threadIdx.x < 64) dqo_header_from_spread(g, capacity, bin.bucket, (int)threadIdx.x);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t n_long = min(g.counters[1], (uint32_t)T);  // tiles queued by tile_sort_wave_kernel
    for (uint32_t q = blockIdx.x; q < n_long; q += sort_blocks) {  // (block-uniform trip count; every helper ends with a barrier)
    const uint32_t tile = img.long_tiles[q];
    const uint2 rg = img.ranges[tile];
    const int n = (int)(rg.y - rg.x);
    uint4* gr = bin.recs + rg.x;
    int n2 = 2 * SORTL_RUN;
    while (n2 < n) n2 <<= 1;
    const int seg_len = min(n2, SORTL_SEG);

    // one ascending compare-exchange step of the network on the segment in LDS: `flip` pairs i with its mirror inside blocks of k
    // (first step of a merge of two ascending halves), otherwise i with i + j
    auto lds_step = [&](int k, int j, bool flip) {
        for (int t = tid; t < seg_len / 2; t += SORT_THREADS) {
            int i, p;
            if (flip) {
                const int h = k >> 1, blk = t / h, off = t - blk * h;
                i = blk * k + off, p = blk * k + k - 1 - off;
            } else {
                i = 2 * j * (t / j) + (t % j), p = i + j;
            }
            const uint64_t a = s_keys[i], b = s_keys[p];
            if (a > b) {
                s_keys[i] = b, s_keys[p] = a;
                const uint32_t va = s_vals[i];
                s_vals[i] = s_vals[p], s_vals[p] = va;
            }
        }
        __syncthreads();
    };
    // every run of the segment through the registers of one wave: full sort (first) or the last nine steps of a merge
    auto runs_in_registers = [&](bool full_sort) {
        for (int run = wave; run < seg_len / SORTL_RUN; run += SORT_THREADS / 64) {
            uint64_t key[SORTP_E];
            uint32_t val[SORTP_E];
            const int base = run * SORTL_RUN + lane * SORTP_E;
#pragma unroll
            for (int r = 0; r < SORTP_E; r++) key[r] = s_keys[base + r], val[r] = s_vals[base + r];
            if (full_sort) wave_bitonic<SORTP_E>(key, val, lane);
            else wave_bitonic_phase<SORTP_E>(key, val, lane, 2 * SORTL_RUN);
#pragma unroll
            for (int r = 0; r < SORTP_E; r++) s_keys[base + r] = key[r], s_vals[base + r] = val[r];
        }
        __syncthreads();
    };
    auto load_segment = [&](int s0) {
        for (int i = tid; i < seg_len; i += SORT_THREADS) {
            const bool in = s0 + i < n;
            const uint4 e = in ? gr[s0 + i] : make_uint4(~0u, ~0u, 0u, 0u);  // padding sorts behind every real key
            s_keys[i] = ((uint64_t)e.y << 32) | e.x;
            s_vals[i] = e.z;
        }
        __syncthreads();
    };
    auto store_segment = [&](int s0, bool final_lists) {
        for (int i = tid; i < seg_len; i += SORT_THREADS) {
            if (s0 + i >= n) continue;
            if (final_lists) {
                bin.point_list[rg.x + s0 + i] = (uint32_t)(s_keys[i] & 0xffffffffu);
                bin.slot_list[rg.x + s0 + i] = s_vals[i];
            } else {
                gr[s0 + i] = make_uint4((uint32_t)s_keys[i], (uint32_t)(s_keys[i] >> 32), s_vals[i], 0u);
            }
        }
        __syncthreads();
    };
    const int nseg = n2 / seg_len;
    // ---- every segment sorted on its own ----
    for (int sg = 0; sg < nseg; sg++) {
        load_segment(sg * seg_len);
        runs_in_registers(true);
        for (int k = 2 * SORTL_RUN; k <= seg_len; k <<= 1) {
            lds_step(k, 0, true);
            for (int j = k >> 2; j >= SORTL_RUN; j >>= 1) lds_step(k, j, false);
            runs_in_registers(false);
        }
        store_segment(sg * seg_len, nseg == 1);
    }
    // ---- merges across segments ----
    for (int k = 2 * seg_len; k <= n2 && nseg > 1; k <<= 1) {
        for (int j = k >> 1; j >= seg_len; j >>= 1) {  // global steps: the flip at distance k, then half cleaners down to one segment
            const bool flip = j == (k >> 1);
            for (int t = tid; t < n2 / 2; t += SORT_THREADS) {
                int i, p;
                if (flip) {
                    const int blk = t / j, off = t - blk * j;
                    i = blk * k + off, p = blk * k + k - 1 - off;
                } else {
                    i = 2 * j * (t / j) + (t % j), p = i + j;
                }
                if (p < n) {  // (a partner past the end is +infinity: nothing to exchange)
                    const uint4 a = gr[i], b = gr[p];
                    if ((((uint64_t)a.y << 32) | a.x) > (((uint64_t)b.y << 32) | b.x)) gr[i] = b, gr[p] = a;
                }
            }
            __syncthreads();
        }
        const bool last = (k << 1) > n2;
        for (int sg = 0; sg < nseg; sg++) {
            if (sg * seg_len >= n) break;  // a segment of padding only
            load_segment(sg * seg_len);
            for (int j = seg_len >> 1; j >= SORTL_RUN; j >>= 1) lds_step(2 * j, j, false);
            runs_in_registers(false);
            store_segment(sg * seg_len, last);
        }
    }
    }  // queue loop
