// k_wideband_tx_body.inc — the body of k_wbtx_duc and k_wbtx_duc_tuned (k_wideband_tx.hip), which include it once each: the text of a kernel,
// not a function, so that `a` stays the kernel's own by-value argument (handed to a function, even one forced inline, its
// pointers are no longer known to be global where the span is filled, and the unscheduled kernel then costs 6 % more than it did:
// profiles/wideband_tune_cost.txt). The including kernel defines WB_LO_OF(k, first): the phase functor of channel k for a workgroup
// whose first wide sample of the push is `first` (k_wideband_common.h: WbLoFixed::channel or WbLoTuned::channel).
    __shared__ int xs[2][OPV_WBTX_SPAN];      // packed int16 I | Q << 16
    __shared__ int16_t tp[OPV_WBTX_TAPS];
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t U = a.U, H = a.H, J = a.J;

    wbtx_write_next_carry<OPV_WBTX_THREADS>(a.hist_out, a.hist_in, H, a.in, a.n_in, a.K, tid);
    const uint32_t n0 = blockIdx.x * OPV_WBTX_THREADS;                    // first wide output of this workgroup, within the push
    if (n0 >= a.n_out) return;

    wb_load_lo<OPV_WBTX_THREADS>(lo, a.lo, tid);
    for (uint32_t i = tid; i < J * U; i += OPV_WBTX_THREADS) tp[i] = i < a.L ? a.taps[i] : (int16_t)0;

    const uint32_t n_last = n0 + OPV_WBTX_THREADS - 1 < a.n_out ? n0 + OPV_WBTX_THREADS - 1 : a.n_out - 1;
    const uint32_t n = n0 + tid < a.n_out ? n0 + tid : n_last;           // (threads past the end redo the last output and store nothing)
    const uint32_t q_lo = n0 / U, q_last = n_last / U, q = n / U, p = n - q * U;
    // local sample i of the span is input sample q_lo - (J - 1) + i of this push: negative ones lie in the carry
    const uint32_t span = q_last - q_lo + J;
    const int64_t m0 = (int64_t)q_lo - (int64_t)(J - 1);
    const uint32_t xq = q - q_lo + J - 1;                                 // where x[q] stands; tap j reads xq - j >= 0
    const uint32_t dn = n - n0;                                           // the LO of wide sample n = n0 + dn of the push (WbLoFixed: phi = (uint32)((first_sample + n) * inc))
    int64_t wr = 0, wi = 0;
    for (uint32_t k = 0; k < a.K; ++k) {
        int* x = xs[k & 1];
        const int* src = a.in[k];
        const int* old = a.hist_in + (size_t)k * H;
        for (uint32_t i = tid; i < span; i += OPV_WBTX_THREADS) {
            const int64_t m = m0 + (int64_t)i;                            // -H <= -(J - 1) <= m <= q_last < n_in
            x[i] = m < 0 ? old[(int64_t)H + m] : src ? src[m] : 0;
        }
        __syncthreads();                                                  // (also: tp and lo, before the first channel)
        int yr = 0, yi = 0;
        for (uint32_t j = 0; j < J; ++j) {
            const int v = x[xq - j];
            const int h = tp[p + j * U];
            yr += h * (int)(int16_t)(v & 0xFFFF);
            yi += h * (v >> 16);
        }
        int c, s;
        WB_LO_OF(k, n0)(lo, dn, c, s);
        wb_mix_up(wr, wi, yr, yi, c, s);
        // (no second barrier: the next channel fills the other span buffer, which was last read before the barrier above)
    }
    if (n0 + tid < a.n_out) a.out[n0 + tid] = wb_round_pack(wr, wi, a.S);
