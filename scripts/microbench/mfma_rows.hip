// Can the fp64 matrix pipe sum the four DPP rows of a wave (lane bits 4-5) cheaper than the two permlane swaps? And is one
// 16-byte store cheaper for a lone wave than two 8-byte ones? (dev tool; mfma_reduce.hip asked the first question for a sum
// INSIDE a row, where the answer was no.)
//   part 1  lane maps of v_mfma_f64_4x4x4_4b_f64, all 64 lanes of A and of B, found with one-hot integer data
//   part 2  bits: the selector forms against the swap tree (r0 + r2) + (r1 + r3) on hostile row partials, every lane
//             A   s0 = mfma(selE, v, 0), s1 = mfma(selO, v, 0), s0 + s1      selE = 1.0 where lane bit 4 is clear, selO its complement
//             A2  mfma(selX, v, 0) -> [s0, s1, s0, s1] by rows, then the permlane16 swap and add
//   part 3  cycles: a dependent chain of (all-reduce, one multiply) per iteration, one wave alone on a CU, every sequence
//           written out in assembly with the wait states hipcc gives it
//   part 4  cycles: two global_store_dwordx2 against one global_store_dwordx4 per iteration behind the same filler
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__global__ void k_map(const double* a, const double* b, double* d) {
    const int l = threadIdx.x;
    d[l] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[l], b[l], 0.0, 0, 0, 0);
}

__device__ inline double sel_e(int l) { return ((l >> 4) & 1) ? 0.0 : 1.0; }
__device__ inline double sel_o(int l) { return ((l >> 4) & 1) ? 1.0 : 0.0; }
__device__ inline double sel_x(int l) { return (((l >> 4) ^ l) & 1) ? 0.0 : 1.0; }   // A: contraction index k on lane bits 4-5, output row i on lane bits 0-1 (part 1)

// 64-bit operands as two 32-bit registers: the swaps take one word each
struct W2 { unsigned lo, hi; };
__device__ inline W2 split(double d) { W2 w; w.lo = (unsigned)__double2loint(d); w.hi = (unsigned)__double2hiint(d); return w; }
__device__ inline double join(W2 w) { return __hiloint2double((int)w.hi, (int)w.lo); }

__device__ inline double tree_sum(double v) {            // what the kernel does today: (r0 + r2) + (r1 + r3) in every lane
    W2 a = split(v), b = a;
    auto lo = __builtin_amdgcn_permlane32_swap(a.lo, b.lo, false, false);
    auto hi = __builtin_amdgcn_permlane32_swap(a.hi, b.hi, false, false);
    double s = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
    a = split(s); b = a;
    lo = __builtin_amdgcn_permlane16_swap(a.lo, b.lo, false, false);
    hi = __builtin_amdgcn_permlane16_swap(a.hi, b.hi, false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ inline double pair_sum(double v, int l) {
    const double s0 = __builtin_amdgcn_mfma_f64_4x4x4f64(sel_e(l), v, 0.0, 0, 0, 0);
    const double s1 = __builtin_amdgcn_mfma_f64_4x4x4f64(sel_o(l), v, 0.0, 0, 0, 0);
    return s0 + s1;
}
__device__ inline double single_sum(double v, int l) {
    const double s = __builtin_amdgcn_mfma_f64_4x4x4f64(sel_x(l), v, 0.0, 0, 0, 0);
    W2 a = split(s), b = a;
    auto lo = __builtin_amdgcn_permlane16_swap(a.lo, b.lo, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(a.hi, b.hi, false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__global__ void k_bits(const double* in, double* tree, double* pair, double* single, int cases) {
    const int l = threadIdx.x;
    for (int c = 0; c < cases; ++c) {
        const double v = in[64 * c + l];
        tree[64 * c + l] = tree_sum(v);
        pair[64 * c + l] = pair_sum(v, l);
        single[64 * c + l] = single_sum(v, l);
    }
}

// MODE 0 swap tree with the two DPP moves in its wait states (the kernel today), 1 MFMA pair bare, 2 MFMA pair with the two
// DPP moves behind it, 3 with them in front, 4 one MFMA + swap16 (A2) with the moves in front, 5 swap tree bare
template <int MODE>
__global__ __launch_bounds__(64) void k_time(int n, double* out, long long* cyc) {
    const int l = threadIdx.x;
    double v = 1.0 + l * 1e-9, t = 0, s0 = 0, s1 = 0, m0 = 0.5 + l, m1 = 0.25 + l, o0 = 0, o1 = 0;
    double e = sel_e(l), o = sel_o(l), x = sel_x(l);
    const double q = 0.25;
    asm volatile("" : "+v"(e), "+v"(o), "+v"(x), "+v"(m0), "+v"(m1));
    const long long t0 = __builtin_amdgcn_s_memtime();
    // The sequences with permlane swaps: the whole loop in one block on fixed registers (a swap takes one 32-bit word per
    // operand, and inline assembly cannot name the halves of a 64-bit operand). v[20:21] the value, v[22:23] its copy.
#define OPV_DPP2 "v_mov_b64_dpp v[24:25], %[m0] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\tv_mov_b64_dpp v[26:27], %[m1] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
#define OPV_LOOP(BODY) \
    asm volatile("v_mov_b64 v[20:21], %[v]\n\ts_mov_b32 s20, %[n]\n\t1:\n\t" BODY \
                 "v_mul_f64 v[20:21], v[20:21], %[q]\n\ts_add_i32 s20, s20, -1\n\ts_cmp_eq_u32 s20, 0\n\ts_cbranch_scc0 1b\n\tv_mov_b64 %[v], v[20:21]" \
                 : [v] "+v"(v) : [n] "s"(n), [m0] "v"(m0), [m1] "v"(m1), [q] "v"(q), [x] "v"(x) \
                 : "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "s20", "scc")
#define OPV_SWAP16 "v_permlane16_swap_b32 v20, v22\n\tv_permlane16_swap_b32 v21, v23\n\tv_add_f64 v[20:21], v[20:21], v[22:23]\n\t"
#define OPV_SWAP32 "v_permlane32_swap_b32 v20, v22\n\tv_permlane32_swap_b32 v21, v23\n\tv_add_f64 v[20:21], v[20:21], v[22:23]\n\t"
    if constexpr (MODE == 0) OPV_LOOP("v_mov_b64 v[22:23], v[20:21]\n\t" OPV_DPP2 OPV_SWAP32 "v_mov_b64 v[22:23], v[20:21]\n\ts_nop 1\n\t" OPV_SWAP16);
    if constexpr (MODE == 5) OPV_LOOP("v_mov_b64 v[22:23], v[20:21]\n\ts_nop 1\n\t" OPV_SWAP32 "v_mov_b64 v[22:23], v[20:21]\n\ts_nop 1\n\t" OPV_SWAP16);
    if constexpr (MODE == 4) OPV_LOOP(OPV_DPP2 "v_mfma_f64_4x4x4_4b_f64 v[22:23], %[x], v[20:21], 0\n\ts_nop 5\n\tv_mov_b64 v[20:21], v[22:23]\n\ts_nop 1\n\t" OPV_SWAP16);
    for (int i = 0; i < n && MODE >= 1 && MODE <= 3; ++i) {
        if constexpr (MODE == 0) {}
        else if constexpr (MODE == 1)
            asm volatile("s_nop 1\n\t"
                         "v_mfma_f64_4x4x4_4b_f64 %[s0], %[e], %[v], 0\n\tv_mfma_f64_4x4x4_4b_f64 %[s1], %[o], %[v], 0\n\t"
                         "s_nop 5\n\t"
                         "v_add_f64 %[v], %[s0], %[s1]\n\tv_mul_f64 %[v], %[v], %[q]"
                         : [v] "+v"(v), [s0] "=&v"(s0), [s1] "=&v"(s1) : [e] "v"(e), [o] "v"(o), [q] "v"(q));
        else if constexpr (MODE == 2)
            asm volatile("s_nop 1\n\t"
                         "v_mfma_f64_4x4x4_4b_f64 %[s0], %[e], %[v], 0\n\tv_mfma_f64_4x4x4_4b_f64 %[s1], %[o], %[v], 0\n\t"
                         "v_mov_b64_dpp %[o0], %[m0] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                         "v_mov_b64_dpp %[o1], %[m1] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                         "s_nop 3\n\t"
                         "v_add_f64 %[v], %[s0], %[s1]\n\tv_mul_f64 %[v], %[v], %[q]"
                         : [v] "+v"(v), [s0] "=&v"(s0), [s1] "=&v"(s1), [o0] "=&v"(o0), [o1] "=&v"(o1)
                         : [e] "v"(e), [o] "v"(o), [m0] "v"(m0), [m1] "v"(m1), [q] "v"(q));
        else if constexpr (MODE == 3)
            asm volatile("v_mov_b64_dpp %[o0], %[m0] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                         "v_mov_b64_dpp %[o1], %[m1] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                         "v_mfma_f64_4x4x4_4b_f64 %[s0], %[e], %[v], 0\n\tv_mfma_f64_4x4x4_4b_f64 %[s1], %[o], %[v], 0\n\t"
                         "s_nop 5\n\t"
                         "v_add_f64 %[v], %[s0], %[s1]\n\tv_mul_f64 %[v], %[v], %[q]"
                         : [v] "+v"(v), [s0] "=&v"(s0), [s1] "=&v"(s1), [o0] "=&v"(o0), [o1] "=&v"(o1)
                         : [e] "v"(e), [o] "v"(o), [m0] "v"(m0), [m1] "v"(m1), [q] "v"(q));
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    out[l] = v + o0 + o1 + s1 + t;
    if (l == 0) cyc[MODE] = t1 - t0;
}

// PAIR 0: two 8-byte stores per iteration (16 bytes apart in time as in the loop: four filler instructions between them);
// PAIR 1: one 16-byte store. Every lane stores the same value to the same address as the kernel's soft log does. The address
// walks a 64 KiB ring from `base8` (0 or 8: the 16-byte store 16-byte aligned or not).
template <int PAIR>
__global__ __launch_bounds__(64) void k_store(int n, unsigned char* ring, unsigned base8, long long* cyc) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef d2 d2u __attribute__((aligned(8)));
    double a = 1.0 + threadIdx.x * 0.0, b = 2.0;
    asm volatile("" : "+v"(a), "+v"(b));
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < n; ++i) {
        unsigned off = (((unsigned)i * 16u) & 0xFFF0u) + base8;        // < 65536 + 8: the ring is 65536 + 64 bytes
        asm volatile("" : "+v"(off));
        asm volatile("v_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1" : "+v"(a) : "v"(b));
        if constexpr (PAIR == 0) *(double*)(ring + off) = a;
        asm volatile("v_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1\n\tv_fma_f64 %0, %0, 1.0, %1" : "+v"(b) : "v"(a));
        if constexpr (PAIR == 0) *(double*)(ring + off + 8u) = b;
        else *(d2u*)(ring + off) = d2{a, b};
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) cyc[PAIR] = t1 - t0;
}

static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

int main() {
    double *a, *b, *d;
    CK(hipMalloc(&a, 512)); CK(hipMalloc(&b, 512)); CK(hipMalloc(&d, 512));
    std::vector<double> ha(64), hb(64), hd(64);
    for (int which = 0; which < 2; ++which) {
        printf("%c lane -> D lanes that receive it (%c = ones):\n", which ? 'B' : 'A', which ? 'A' : 'B');
        for (int la = 0; la < 64; ++la) {
            for (int l = 0; l < 64; ++l) { (which ? hb : ha)[l] = (l == la) ? 1.0 : 0.0; (which ? ha : hb)[l] = 1.0; }
            CK(hipMemcpy(a, ha.data(), 512, hipMemcpyHostToDevice)); CK(hipMemcpy(b, hb.data(), 512, hipMemcpyHostToDevice));
            k_map<<<1, 64>>>(a, b, d);
            CK(hipMemcpy(hd.data(), d, 512, hipMemcpyDeviceToHost));
            printf("  %c lane %2d ->", which ? 'B' : 'A', la);
            for (int l = 0; l < 64; ++l) if (hd[l] != 0.0) printf(" %d", l);
            printf("\n");
        }
    }
    // part 2: row partials r0..r3 per output t (lane = 16 row + t): full-scale magnitudes, cancelling pairs, zero rows, tiny values
    const int cases = 64;
    std::vector<double> in(64 * cases), tr(64 * cases), pr(64 * cases), sg(64 * cases);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(long long)(s >> 11) / 9007199254740992.0 - 0.5; };
    for (int c = 0; c < cases; ++c)
        for (int l = 0; l < 64; ++l) {
            const int row = l >> 4, t = l & 15;
            double r = rnd() * ldexp(1.0, (c % 8) * 5 - 10);                     // 2^-10 .. 2^25
            if (c >= 8 && c < 24 && ((c >> row) & 1)) r = 0.0;                   // whole rows of exact zeros
            if (c >= 24 && c < 32 && row >= 2) r = -in[64 * c + l - 32];         // r2 = -r0, r3 = -r1: zero sums
            if (c >= 32 && c < 40 && (row & 1)) r = -in[64 * c + l - 16] * (1.0 + ldexp(1.0, -50));   // near-cancelling neighbours
            if (c >= 40 && c < 48) r = (t & 1) ? 1e-18 * rnd() : 32767.0 * 40.0 * 15.0 * (rnd() > 0 ? 1 : -1);
            if (c >= 48 && c < 56) r = (double)(long long)(rnd() * 1e9) + ldexp(rnd(), -30);   // long mantissas
            in[64 * c + l] = r;
        }
    double *din, *dtr, *dpr, *dsg;
    CK(hipMalloc(&din, in.size() * 8)); CK(hipMalloc(&dtr, in.size() * 8)); CK(hipMalloc(&dpr, in.size() * 8)); CK(hipMalloc(&dsg, in.size() * 8));
    CK(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    k_bits<<<1, 64>>>(din, dtr, dpr, dsg, cases);
    CK(hipMemcpy(tr.data(), dtr, in.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(pr.data(), dpr, in.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(sg.data(), dsg, in.size() * 8, hipMemcpyDeviceToHost));
    int bad_host = 0, bad_pair = 0, bad_single = 0;
    for (int c = 0; c < cases; ++c)
        for (int l = 0; l < 64; ++l) {
            const int t = l & 15;
            const double* r = &in[64 * c];
            volatile double s02 = r[t] + r[32 + t], s13 = r[16 + t] + r[48 + t];
            const double want = s02 + s13;
            bad_host += bits(tr[64 * c + l]) != bits(want);
            bad_pair += bits(pr[64 * c + l]) != bits(tr[64 * c + l]);
            bad_single += bits(sg[64 * c + l]) != bits(tr[64 * c + l]);
        }
    printf("bits over %d cases x 64 lanes: swap tree != host (r0+r2)+(r1+r3): %d; MFMA pair != swap tree: %d; one MFMA + swap16 != swap tree: %d\n",
           cases, bad_host, bad_pair, bad_single);
    // part 3
    double* out; long long* cyc;
    CK(hipMalloc(&out, 512)); CK(hipMalloc(&cyc, 64));
    const int n = 200000;
    long long hc[8];
    const char* names[6] = {"swap tree + 2 DPP moves in its wait states (today)", "MFMA pair, bare (s_nop 1 | s_nop 5)", "MFMA pair, 2 DPP moves behind (s_nop 1 | s_nop 3)",
                            "MFMA pair, 2 DPP moves in front (| s_nop 5)", "one MFMA + swap16, 2 DPP moves in front (A2)", "swap tree, bare"};
    for (int rep = 0; rep < 2; ++rep) {
        k_time<0><<<1, 64>>>(n, out, cyc); k_time<1><<<1, 64>>>(n, out, cyc); k_time<2><<<1, 64>>>(n, out, cyc);
        k_time<3><<<1, 64>>>(n, out, cyc); k_time<4><<<1, 64>>>(n, out, cyc); k_time<5><<<1, 64>>>(n, out, cyc);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(hc, cyc, 48, hipMemcpyDeviceToHost));
        for (int m = 0; m < 6; ++m) printf("pass %d: %-52s + 1 mul: %7.2f s_memtime ticks per iteration\n", rep, names[m], (double)hc[m] / n);
    }
    // part 4
    unsigned char* ring;
    CK(hipMalloc(&ring, 65536 + 64));
    for (unsigned base8 = 0; base8 <= 8; base8 += 8)
        for (int rep = 0; rep < 2; ++rep) {
            k_store<0><<<1, 64>>>(n, ring, base8, cyc); k_store<1><<<1, 64>>>(n, ring, base8, cyc);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(hc, cyc, 16, hipMemcpyDeviceToHost));
            printf("pass %d, address %u mod 16: 8 fma + two dwordx2 stores %7.2f, 8 fma + one dwordx4 store %7.2f s_memtime ticks per iteration\n",
                   rep, base8, (double)hc[0] / n, (double)hc[1] / n);
        }
    return 0;
}
