// k_wideband_tx_rational_body.inc — the body of k_wbtxr_duc and k_wbtxr_duc_tuned (k_wideband_tx_rational.hip), which include it once each: the text of a kernel,
// not a function, so that `a` stays the kernel's own by-value argument (handed to a function, even one forced inline, its
// pointers are no longer known to be global where the span is filled, and the unscheduled kernel then costs 6 % more than it did:
// profiles/wideband_tune_cost.txt). The including kernel defines WB_LO_OF(k, first): the phase functor of channel k for a workgroup
// whose first wide sample of the push is `first` (k_wideband_common.h: WbLoFixed::channel or WbLoTuned::channel).
    __shared__ int tile[OPV_WBTXR_MAXJ / 2][OPV_WBTXR_THREADS];   // taps (2 j, 2 j + 1) of thread tid's row: lo | hi << 16
    __shared__ int xs[2][OPV_WBTXR_SPAN];                        // packed int16 I | Q << 16
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t M = a.M, U = a.U, H = a.H, J2 = a.J2;

    wbtx_write_next_carry<OPV_WBTXR_THREADS>(a.hist_out, a.hist_in, H, a.in, a.n_in, a.K, tid);
    const uint32_t out0 = blockIdx.x * OPV_WBTXR_THREADS;                 // first wide output of this workgroup, within the push
    if (out0 >= a.n_out) return;
    const uint32_t cnt = a.n_out - out0 < OPV_WBTXR_THREADS ? a.n_out - out0 : OPV_WBTXR_THREADS;

    // output out0 + l of the push: (p0 + (out0 + l) U) / M inputs behind the push's first, remainder = its phase. 64 bits once per
    // workgroup for out0; per lane pbase + l U < 2^13 + 2^8 2^13 stays in 32.
    const uint64_t t0 = (uint64_t)a.p0 + (uint64_t)out0 * U;
    const uint64_t q0 = t0 / M;
    const uint32_t pbase = (uint32_t)(t0 - q0 * M);
    const uint32_t tl = pbase + (tid < cnt ? tid : cnt - 1) * U;          // (threads past the end redo the last output and store nothing)
    const uint32_t dq = tl / M, p = tl - dq * M;
    // local sample i of the span is input q0 - front + i of this push: negative ones lie in the carry, or in front of it (zeros:
    // they meet the zero padding of a tap row). The newest input of the workgroup's last output, q0 + dq_last, is < n_in by W's rule.
    const uint32_t front = 2 * J2 - 1;
    const uint32_t span = front + (pbase + (cnt - 1) * U) / M + 1;        // <= 63 + 256
    const int64_t m0 = (int64_t)q0 - (int64_t)front;
    const uint32_t xq = front + dq;                                       // where x[q] stands; tap j reads xq - j >= 0

    auto fetch = [&](uint32_t k, uint32_t i) -> int {
        if (i >= span) return 0;
        const int64_t m = m0 + (int64_t)i;
        if (m < -(int64_t)H) return 0;
        if (m < 0) return a.hist_in[(size_t)k * H + (size_t)((int64_t)H + m)];
        const int* src = a.in[k];
        return src ? src[m] : 0;
    };

    wb_load_lo<OPV_WBTXR_THREADS>(lo, a.lo, tid);
    {
        const int2* row = (const int2*)(a.taps + (size_t)p * a.rowlen);   // rowlen is a multiple of 4: rows start on 8 bytes
        for (uint32_t i = 0; i < a.rowlen / 4; ++i) {
            const int2 h = row[i];
            tile[2 * i][tid] = h.x;
            tile[2 * i + 1][tid] = h.y;
        }
    }
    const uint32_t dn = tid < cnt ? tid : cnt - 1;                        // the LO of wide sample out0 + dn of the push (WbLoFixed: phi = (uint32)((first_sample + n) * inc))
    int64_t wr = 0, wi = 0;
    int v0 = fetch(0, tid), v1 = fetch(0, tid + OPV_WBTXR_THREADS);
    for (uint32_t k = 0; k < a.K; ++k) {
        int* x = xs[k & 1];
        x[tid] = v0;
        if (tid < OPV_WBTXR_SPAN - OPV_WBTXR_THREADS) x[tid + OPV_WBTXR_THREADS] = v1;
        __syncthreads();                                                  // (also: lo, before the first channel; tile is each thread's own)
        if (k + 1 < a.K) {
            v0 = fetch(k + 1, tid);
            v1 = fetch(k + 1, tid + OPV_WBTXR_THREADS);
        }
        int yr = 0, yi = 0;
        for (uint32_t j = 0; j < J2; ++j) {
            const int h2 = tile[j][tid];
            const int u0 = x[xq - 2 * j], u1 = x[xq - 2 * j - 1];
            const int h0 = (int16_t)(h2 & 0xFFFF), h1 = h2 >> 16;
            yr += h0 * (int)(int16_t)(u0 & 0xFFFF) + h1 * (int)(int16_t)(u1 & 0xFFFF);
            yi += h0 * (u0 >> 16) + h1 * (u1 >> 16);
        }
        int c, s;
        WB_LO_OF(k, out0)(lo, dn, c, s);
        wb_mix_up(wr, wi, yr, yi, c, s);
        // (no second barrier: the next channel fills the other span buffer, which was last read before the barrier above)
    }
    if (tid < cnt) a.out[out0 + tid] = wb_round_pack(wr, wi, a.S);
