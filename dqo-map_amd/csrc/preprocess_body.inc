// The body of preprocess_kernel<LATE> and preprocess_pf_kernel<LATE>, included by both kernels.  As an inlined function it moved the
// register allocation of the existing kernel, whose gfx950 code must not change.  In scope: the kernel's parameters and the
// compile-time PF (the parameter form: raw opacities / scales / rotations, features_dc + rest).  Compiled with contraction off (the pragma opens both kernels).
    __shared__ uint32_t s_visible;
    const int tid = threadIdx.x;
    const int P = v.P;
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; i++) view[i] = v.view[i], proj[i] = v.proj[i];
    const float cam0 = v.campos[0], cam1 = v.campos[1], cam2 = v.campos[2];
    __shared__ uint32_t s_cand;
    if (tid == 0) s_visible = 0, s_cand = 0;
    // (a frame_prezeroed frame still holds the previous frame's header: mark it "stage 1" until the sort kernels rewrite it)
    if (blockIdx.x == 0 && tid == 0) g.header->stage = 1u;
    // DqoRastCtx.frame_prezeroed is a promise of the caller (the previous frame on this ctx ended in dqo_rast_backward_adam, whose tail
    // clears the per-frame scalars).  A broken promise — a forward-only render, dqo_rast_backward, an error return in between — would
    // give wrong slot bases and doubled statistics without a sign: the first block looks at the words no kernel of THIS frame has
    // touched yet (slot allocators, queue counters, loss-tap sums; not words 0, 1 of the lines, which this launch is adding to) and
    // raises counters[8], which both header writers fold into header.overflow.
    if (check_prezeroed && blockIdx.x == 0 && tid < DQO_SPREAD) {
        const uint32_t* line = g.spread + (size_t)tid * 64;
        uint32_t bad = line[2] | line[3] | line[4] | line[5];
#pragma unroll
        for (int i = 8; i < 16; i++) bad |= line[i];
        if (tid < 8) bad |= g.counters[tid];
        if (bad != 0u) atomicOr(&g.counters[8], 1u);
    }
    // this launch also zeroes the tile histogram + tile flags for bin_count_kernel (one contiguous range, a slice per block)
    {
        const size_t per = (zero_words + gridDim.x - 1) / gridDim.x;
        const size_t z0 = (size_t)blockIdx.x * per, z1 = min(zero_words, z0 + per);
        for (size_t i = z0 + tid; i < z1; i += K1_THREADS) zero_base[i] = 0u;
    }
    __syncthreads();

    uint32_t nvis = 0, ncand = 0;
#pragma unroll 1
    for (int it = 0; it < K1_ITEMS; it++) {
        const int idx = blockIdx.x * (K1_THREADS * K1_ITEMS) + it * K1_THREADS + tid;
        if (idx >= P) continue;
        const K1Early e = k1_early<LATE, PF>(v, view, proj, cam0, cam1, cam2, idx, means3D, scales, rotations, opacities, shs, colors_precomp, gobj,
                                             g, radii_out, n_touched_out, rest);
        const int radius = e.radius, rminx = e.rminx, rminy = e.rminy, rmaxx = e.rmaxx, rmaxy = e.rmaxy;
        nvis += radius > 0 ? 1u : 0u;
        ncand += (uint32_t)((rmaxx - rminx) * (rmaxy - rminy));
    }
    // visible count (statistics) and the number of (Gaussian, tile) pairs in the tile rects — the reference's num_rendered
    // (rasterizer_impl.cu:303-309) and an upper bound of the instances the binning keeps
    if (nvis) atomicAdd(&s_visible, nvis);
    if (ncand) atomicAdd(&s_cand, ncand);
    __syncthreads();
    uint32_t* const my_line = g.spread + (size_t)(blockIdx.x % DQO_SPREAD) * 64;
    if (tid == 0 && s_visible) atomicAdd(&my_line[0], s_visible);
    if (tid == 0 && s_cand) atomicAdd(&my_line[1], s_cand);
