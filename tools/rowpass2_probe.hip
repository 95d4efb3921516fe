// Diagnostic: where do the waves of the second-generation row pass spend their cycles?  (not product code)
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/rowpass2_probe.hip -o tools/rowpass2_probe && tools/rowpass2_probe [T2] [wg per CU]
//   -DPROBE_NO_STAMPS: the kernel as it ships (launch times only); -DPROBE_KERNEL_SRC="\"file\"": another version of the source
//   -DPROBE_X16: the form on the methylated read counts (X16 + D16, V not read)
//   -DPROBE_PAIR (with -DPROBE_X16): the pair schedule, two blocks per phase B; cycles then also per pair of blocks
//   -DPROBE_DEFER_C (with -DPROBE_X16 -DPROBE_PAIR): phase C deferred into the other waves' phase-B window; the window is then
//     reported per role and the drain as a segment of its own (the x ring is written by the tile store: no copy to time);
//     -DDMF_V2_STAGGER_DEFER=n: its stagger, -DDMF_V2_DEFER_PRIO=n: the s_setprio of the deferred phase C
//   -DPROBE_BYTES (with -DPROBE_X16 -DPROBE_PAIR -DPROBE_DEFER_C): the byte form <.., BYTES> on the images X8 / D8 (built here by
//     k_build_rowpass_images, which is timed too) beside the u16 deferred-C form of the same source: the launches alternate,
//     and the stamps are reported for the u16 form first, then for the byte form
//   -DDMF_CHAIN_NO_UNROLL: the inner steps as a loop at every step count (T2 = 20 otherwise runs them written out)
//   -DDMF_CHAIN_NO_I32: the M combine with eight conversions per value instead of digit pairs joined in i32
//   both together: the kernel before either, from this source
#ifndef PROBE_NO_STAMPS
#define DMF_STAMPS 1
#endif
#ifdef PROBE_KERNEL_SRC
#include PROBE_KERNEL_SRC
#else
#include "../demethify_amd/csrc/dmf_kernels_rowpass2.hip"
#endif
#include <cstdio>
#include <random>
#include <vector>
using namespace dmf;
#ifdef PROBE_X16
constexpr bool kXS = true;
#else
constexpr bool kXS = false;
#endif
#ifdef PROBE_PAIR
constexpr bool kPair = true;
static_assert(kXS, "the pair schedule is an X16 form");
#else
constexpr bool kPair = false;
#endif
#ifdef PROBE_DEFER_C
constexpr bool kDefer = true;
static_assert(kPair, "the deferred-C schedule is a pair schedule");
#else
constexpr bool kDefer = false;
#endif
#ifdef PROBE_BYTES
constexpr bool kBytes = true;
static_assert(kDefer, "the byte form is a deferred-C form");
#else
constexpr bool kBytes = false;
#endif
#ifndef DMF2_NSTAMP
#define DMF2_NSTAMP 16
#endif
constexpr int kNS = DMF2_NSTAMP;
int main(int argc, char** argv) {
    const int64_t N = 1000000; const int S = 256, n_c = 12, n_u = 4, K = 16;
    const int T2 = argc > 1 ? atoi(argv[1]) : 20;
    const int per_cu = argc > 2 ? atoi(argv[2]) : 2;
    std::mt19937_64 rng(1); std::uniform_real_distribution<double> U(0, 1);
    std::vector<double> hV((size_t)N * S), hR((size_t)N * n_c), hu((size_t)N * n_u), ha((size_t)K * S);
    std::vector<unsigned short> hD((size_t)N * S), hX((size_t)N * S);
    for (auto& x : hV) x = U(rng); for (auto& x : hD) x = 1 + (int)(U(rng) * 80); for (auto& x : hR) x = U(rng);
    for (size_t i = 0; i < hX.size(); ++i) hX[i] = (unsigned short)(hV[i] * hD[i]);
    for (auto& x : hu) x = U(rng); for (auto& x : ha) x = U(rng) / K;
    double *V, *R, *u, *up, *a, *slab, *u2; unsigned short *D, *X; SolverState* st; unsigned long long* stamps;
    hipMalloc(&V, hV.size() * 8); hipMalloc(&D, hD.size() * 2); hipMalloc(&X, hX.size() * 2); hipMalloc(&R, hR.size() * 8); hipMalloc(&u, hu.size() * 8);
    hipMalloc(&up, hu.size() * 8); hipMalloc(&a, ha.size() * 8); hipMalloc(&u2, 8192 * 8); hipMalloc(&st, sizeof(SolverState));
    const int grid = 256 * per_cu;
    hipMalloc(&slab, (size_t)grid * n_u * S * 8); hipMalloc(&stamps, (size_t)grid * 4 * kNS * 8);
    hipMemcpy(V, hV.data(), hV.size() * 8, hipMemcpyHostToDevice); hipMemcpy(D, hD.data(), hD.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(X, hX.data(), hX.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(R, hR.data(), hR.size() * 8, hipMemcpyHostToDevice); hipMemcpy(u, hu.data(), hu.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(up, hu.data(), hu.size() * 8, hipMemcpyHostToDevice); hipMemcpy(a, ha.data(), ha.size() * 8, hipMemcpyHostToDevice);
    SolverState h{}; h.a1 = 1; h.a2 = 1; h.l_w = 1e4; h.l_w_prev = 1e4; h.l_h = 1e6; h.l_h_prev = 1e6; h.dsq = 6400;
    hipMemcpy(st, &h, sizeof(h), hipMemcpyHostToDevice); hipMemset(stamps, 0, (size_t)grid * 4 * kNS * 8);
    const size_t lds = rowpass_v2_lds_bytes(S, n_u, T2, kXS, kPair, kDefer);
    hipFuncSetAttribute((const void*)k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    // (PROBE_BYTES) the images of X / D (N is a multiple of 16 and S of 64 here: the arrays are their own padded copies), and
    // stamps of their own for the byte form
    unsigned char *X8 = nullptr, *D8 = nullptr; unsigned long long* stamps8 = nullptr;
    size_t lds8 = 0;
    if constexpr (kBytes) {
        static_assert(!kBytes || (N % 16 == 0 && S % 64 == 0), "X / D stand in for the padded copies");
        hipMalloc(&X8, (size_t)N * S); hipMalloc(&D8, (size_t)N * S); hipMalloc(&stamps8, (size_t)grid * 4 * kNS * 8);
        hipMemset(stamps8, 0, (size_t)grid * 4 * kNS * 8);
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0);
            const hipError_t e = launch_build_rowpass_images(X, D, N, S, X8, D8, 0);
            hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1); printf("k_build_rowpass_images %d: %.3f ms  (%s)\n", rep, ms, hipGetErrorString(e));
        }
        lds8 = rowpass_v2_lds_bytes(S, n_u, T2, kXS, kPair, kDefer, true);
        hipFuncSetAttribute((const void*)k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer, kBytes>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        printf("LDS per workgroup: u16 form %zu B, byte form %zu B\n", lds, lds8);
    }
    for (int rep = 0; rep < (argc > 3 ? atoi(argv[3]) : 3); ++rep) {
        hipEventRecord(e0);
#ifdef PROBE_NO_STAMPS
        hipLaunchKernelGGL((k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer>), dim3(grid), dim3(256), lds, 0, V, D, X, 256, R, a, u, up, st, N, S, n_c, T2, 0, 1, slab, u2);
#else
        hipLaunchKernelGGL((k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer>), dim3(grid), dim3(256), lds, 0, V, D, X, 256, R, a, u, up, st, N, S, n_c, T2, 0, 1, slab, u2, stamps);
#endif
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); printf("launch %d: %.3f ms  (%s)\n", rep, ms, hipGetErrorString(hipGetLastError()));
        if constexpr (kBytes) {
            hipEventRecord(e0);
#ifdef PROBE_NO_STAMPS
            hipLaunchKernelGGL((k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer, kBytes>), dim3(grid), dim3(256), lds8, 0, V, (const unsigned short*)D8, (const unsigned short*)X8, 256, R, a, u, up, st, N, S, n_c, T2, 0, 1, slab, u2);
#else
            hipLaunchKernelGGL((k_rowpass_v2<3, 4, 4, kXS, kPair, kDefer, kBytes>), dim3(grid), dim3(256), lds8, 0, V, (const unsigned short*)D8, (const unsigned short*)X8, 256, R, a, u, up, st, N, S, n_c, T2, 0, 1, slab, u2, stamps8);
#endif
            hipEventRecord(e1); hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1); printf("launch %d, byte form: %.3f ms  (%s)\n", rep, ms, hipGetErrorString(hipGetLastError()));
        }
    }
#ifdef PROBE_NO_STAMPS
    return 0;
#endif
    std::vector<unsigned long long> hs((size_t)grid * 4 * kNS);
  for (int form = 0; form < (kBytes ? 2 : 1); ++form) {
    if (kBytes) printf("---- %s\n", form == 0 ? "u16 deferred-C form" : "byte form");
    hipMemcpy(hs.data(), form == 0 ? stamps : stamps8, hs.size() * 8, hipMemcpyDeviceToHost);
    const char* an[16] = {"tile store (vmcnt wait)", "phase A (MFMA)", "partials", "wait X", "phase B / nothing", "wait Y", "phase C", "prefetch issue", "B: partial sums", "B: inner steps", "B: stores", "phase A, 2nd block", "partials, 2nd block", "phase C, 2nd block", "-", "-"};
    double sum[20] = {0}; int cnt = 0;
    for (int b = 0; b < grid; ++b) for (int w = 0; w < 4; ++w) { for (int i = 0; i < kNS; ++i) if (i != 15) sum[i] += (double)hs[((size_t)b * 4 + w) * kNS + i]; ++cnt; }
    double tot = 0; for (int i = 0; i < 8; ++i) tot += sum[i];  // (8..10: sub-segments of phase B, already inside segment 4)
    for (int i = 11; i < 15; ++i) tot += sum[i];
    for (int i = 16; i < 20; ++i) tot += sum[i];
    if (kDefer) {
        // a wave runs phase B's role in every second cycle and phase C's in the others: its sums hold both, one after the other
        an[4] = "window, B role: phase B"; an[7] = "window, B role: issue"; an[5] = "window, B role: wait Y";
        an[6] = "window, C role: phase C x 4"; an[13] = "drain (whole kernel)";  // (x goes into the ring at the tile store: no copy to time)
    }
    const double steps = (N / 16.0) / grid;
    printf("T2 = %d, %d workgroups per CU%s: mean cycles per wave %.0f over the kernel, %.0f per block, %.0f per pair of blocks\n", T2, per_cu,
           kPair ? ", pair schedule" : "", tot / cnt, tot / cnt / steps, 2 * tot / cnt / steps);
    for (int i = 0; i < 15; ++i) if (an[i][0] != '-' && (kPair || i < 11)) printf("   %-28s %6.1f %%  (%.0f cycles per block, %.0f per pair)\n", an[i], 100 * sum[i] / tot, sum[i] / cnt / steps, 2 * sum[i] / cnt / steps);
    if (kDefer) {
        // per cycle of that role (a wave has each role in half of its cycles: 4 x the per-block mean)
        printf("   window, C role: issue %.0f, wait Y %.0f cycles per pair\n", 2 * sum[16] / cnt / steps, 2 * sum[17] / cnt / steps);
        printf("   X -> Y window per cycle of the role: B role %.0f (issue %.0f + phase B %.0f + wait %.0f), C role %.0f (issue %.0f + phase C %.0f + wait %.0f)\n",
               4 * (sum[7] + sum[4] + sum[5]) / cnt / steps, 4 * sum[7] / cnt / steps, 4 * sum[4] / cnt / steps, 4 * sum[5] / cnt / steps,
               4 * (sum[16] + sum[6] + sum[17]) / cnt / steps, 4 * sum[16] / cnt / steps, 4 * sum[6] / cnt / steps, 4 * sum[17] / cnt / steps);
    }
    // where the waves sit: HW_ID bits 5:4 = SIMD.  Phase B of block s runs on wave s % 4: the pair schedule wants waves
    // w and w + 1 (mod 4) on different SIMDs
    int distinct = 0, adjacent_apart = 0;
    for (int b = 0; b < grid; ++b) {
        int simd[4], mask = 0;
        for (int w = 0; w < 4; ++w) { simd[w] = (int)((hs[((size_t)b * 4 + w) * kNS + 15] >> 4) & 3); mask |= 1 << simd[w]; }
        distinct += mask == 15;
        bool ok = true;
        for (int w = 0; w < 4; ++w) ok = ok && simd[w] != simd[(w + 1) % 4];
        adjacent_apart += ok;
    }
    printf("SIMD placement (HW_ID): %d of %d workgroups have their four waves on four SIMDs, %d have waves w, w + 1 apart\n", distinct, grid, adjacent_apart);
  }
    return 0;
}
