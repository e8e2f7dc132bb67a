// mgmc_fieldstats.hpp -- pointwise running mean and M2 (sum of squared deviations) of the level-0 state,
// accumulated on the device after every recorded cycle (the reference's posterior_statistics,
// driver_mgmc.cc:118-171, keeps the sums of x and x^2 on the host instead).
//
// One (mean, M2) pair per stored vertex of level 0, pooled over the handle's chains, as two arrays in
// level 0's padded layout (Layout, nstore doubles each; zeroed at enable).  k_fieldstats streams flat
// over [0, nstore): nstore and every chain's offset are multiples of 16 doubles (make_layout), so the
// kernel moves 16-byte pairs throughout; the halo and the padding of x are 0 and stay 0 in both fields.
// Per vertex the chains are folded in the order c = 0 .. K-1 with k_qoi_record's Welford update,
//     delta = x - mean;  mean' = mean + delta / cnt;  M2' = M2 + delta * (x - mean'),
// cnt = states recorded so far + 1, in plain IEEE double (the library is built with -ffp-contract=off).
//
// Counters (device memory: the graph is replayed): ctl[0] = cycles seen since enable / reset,
// ctl[1] = states recorded, ctl[2] = stride.  Cycle number ctl[0] + 1 is recorded when the stride divides
// it; on the other cycles every workgroup leaves on that uniform branch.  Every workgroup of k_fieldstats
// reads the counters, so the kernel never writes them: k_fieldstats_advance, one thread in a launch of
// its own right after it on the same stream, advances them.
//
// No LDS, no atomics.  The fields have no reuse before the next recorded cycle (512^3: 2 x 1.1 GB against
// a 256 MB last-level cache), so they are read and written with non-temporal accesses; x was written
// by the cycle's last sweep and is read with plain loads.  Traffic per recorded cycle and stored vertex:
// 8 K (x) + 16 (mean, M2 read) + 16 (written) bytes.  One pass per thread, FS_PAIRS pairs FS_NT * 16 bytes
// apart with their loads issued together, one workgroup per FS_NT * FS_PAIRS pairs at any size: the full
// grid streams faster than a capped one with a grid-stride loop (the same holds for the
// plain triad, profiles/r01_stream_ceiling.txt).
//
// Batch means (mgmc_field_stats_enable_batched; the instance k_fieldstats<NCH, true>): three more arrays in
// the same layout, zeroed at enable.  bsum is the sum of the current batch, bmean / bM2 the Welford mean
// and M2 of the completed batches' means.  With B = ctl[3] the batch length in recorded cycles and
// r = (ctl[0] + 1) / stride the number of this recorded cycle (= ctl[1] / K + 1: both counters are zeroed
// together), per vertex
//     for c = 0 .. K-1:  bsum = bsum + x_c
//     if r % B == 0:  bm = bsum / (double)(B K);  nb = r / B;  d = bm - bmean;  bmean' = bmean + d / nb;
//                     bM2' = bM2 + d * (bm - bmean');  bsum = +0.0
// A batch pools the K chains of its B cycles.  r % B is uniform over the launch: mid-batch the kernel
// moves 8 K + 48 bytes per stored vertex (bsum read and written besides mean and M2), at a batch end
// 8 K + 80 (bmean and bM2 read and written, bsum only written).  mean and M2 take the statements they
// take without batching, in their order; the batch statements stand under `if constexpr`, so the
// instances <1> and <0> are the kernels they were before the flag existed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgmc_tuning.hpp"

namespace mgmc {

typedef double fs_pair __attribute__((ext_vector_type(2)));

// launch shape: mgmc_tuning.hpp (threads per workgroup, pairs per thread)
constexpr int FS_NT = tune::FS_NT, FS_PAIRS = tune::FS_PAIRS;
constexpr int FS_CTL_WORDS = 4;  // ctl[0] cycles seen, ctl[1] states recorded, ctl[2] stride, ctl[3] batch length (0: no batching)

// x: level 0's state of chain 0, chain c's cs doubles on (cs even); npairs = nstore / 2;
// bsum, bmean, bm2: read by the BATCH instances only (nullptr otherwise)
template <int NCH, bool BATCH = false>
static __global__ void __launch_bounds__(FS_NT) k_fieldstats(const double* __restrict__ x, long long cs, int nchains,
                                                             double* __restrict__ mean, double* __restrict__ m2,
                                                             long long npairs, const uint64_t* __restrict__ ctl,
                                                             double* __restrict__ bsum, double* __restrict__ bmean,
                                                             double* __restrict__ bm2) {
    const uint64_t cycle = ctl[0] + 1, stride = ctl[2];
    if (cycle % stride != 0) return;  // thinning: not a recorded cycle (uniform over the launch)
    const uint64_t n0 = ctl[1];
    const int nch = NCH > 0 ? NCH : nchains;
    // batch means: this is recorded cycle r; the batch ends with it when B divides r (uniform over the launch).
    // The scalar divisions stand before the first load, so the loads of all the fields issue together.
    [[maybe_unused]] uint64_t nb = 0;
    [[maybe_unused]] bool batch_end = false;
    if constexpr (BATCH) {
        const uint64_t r = cycle / stride, blen = ctl[3];
        nb = r / blen;
        batch_end = r % blen == 0;
    }
    const fs_pair* __restrict__ xp = reinterpret_cast<const fs_pair*>(x);
    fs_pair* __restrict__ mp = reinterpret_cast<fs_pair*>(mean);
    fs_pair* __restrict__ sp = reinterpret_cast<fs_pair*>(m2);
    const long long cp = cs / 2;
    const long long q0 = (long long)blockIdx.x * (FS_NT * FS_PAIRS) + threadIdx.x;
    fs_pair m[FS_PAIRS], s[FS_PAIRS];
#pragma unroll
    for (int u = 0; u < FS_PAIRS; ++u) {
        const long long q = q0 + u * FS_NT;
        if (q < npairs) {
            m[u] = __builtin_nontemporal_load(mp + q);
            s[u] = __builtin_nontemporal_load(sp + q);
        }
    }
    [[maybe_unused]] fs_pair bs[FS_PAIRS], bm[FS_PAIRS], bq[FS_PAIRS];
    [[maybe_unused]] fs_pair* __restrict__ bsp = reinterpret_cast<fs_pair*>(bsum);
    [[maybe_unused]] fs_pair* __restrict__ bmp = reinterpret_cast<fs_pair*>(bmean);
    [[maybe_unused]] fs_pair* __restrict__ bqp = reinterpret_cast<fs_pair*>(bm2);
    if constexpr (BATCH) {
#pragma unroll
        for (int u = 0; u < FS_PAIRS; ++u) {
            const long long q = q0 + u * FS_NT;
            if (q < npairs) {
                bs[u] = __builtin_nontemporal_load(bsp + q);
                if (batch_end) {
                    bm[u] = __builtin_nontemporal_load(bmp + q);
                    bq[u] = __builtin_nontemporal_load(bqp + q);
                }
            }
        }
    }
    for (int c = 0; c < nch; ++c) {
        const double cnt = (double)(n0 + (uint64_t)c + 1);
#pragma unroll
        for (int u = 0; u < FS_PAIRS; ++u) {
            const long long q = q0 + u * FS_NT;
            if (q >= npairs) continue;
            const fs_pair v = xp[(long long)c * cp + q];
            const double d0 = v.x - m[u].x, d1 = v.y - m[u].y;
            const double a0 = m[u].x + d0 / cnt, a1 = m[u].y + d1 / cnt;
            s[u].x = s[u].x + d0 * (v.x - a0);
            s[u].y = s[u].y + d1 * (v.y - a1);
            m[u].x = a0;
            m[u].y = a1;
            if constexpr (BATCH) {
                bs[u].x = bs[u].x + v.x;
                bs[u].y = bs[u].y + v.y;
            }
        }
    }
    if constexpr (BATCH) {
        if (batch_end) {
            const double per = (double)(ctl[3] * (uint64_t)nch), cntb = (double)nb;
#pragma unroll
            for (int u = 0; u < FS_PAIRS; ++u) {
                const long long q = q0 + u * FS_NT;
                if (q >= npairs) continue;
                const double b0 = bs[u].x / per, b1 = bs[u].y / per;
                const double d0 = b0 - bm[u].x, d1 = b1 - bm[u].y;
                const double a0 = bm[u].x + d0 / cntb, a1 = bm[u].y + d1 / cntb;
                bq[u].x = bq[u].x + d0 * (b0 - a0);
                bq[u].y = bq[u].y + d1 * (b1 - a1);
                bm[u].x = a0;
                bm[u].y = a1;
                bs[u].x = 0.0;
                bs[u].y = 0.0;
                __builtin_nontemporal_store(bm[u], bmp + q);
                __builtin_nontemporal_store(bq[u], bqp + q);
            }
        }
#pragma unroll
        for (int u = 0; u < FS_PAIRS; ++u) {
            const long long q = q0 + u * FS_NT;
            if (q < npairs) __builtin_nontemporal_store(bs[u], bsp + q);
        }
    }
#pragma unroll
    for (int u = 0; u < FS_PAIRS; ++u) {
        const long long q = q0 + u * FS_NT;
        if (q < npairs) {
            __builtin_nontemporal_store(m[u], mp + q);
            __builtin_nontemporal_store(s[u], sp + q);
        }
    }
}

// one thread, launched after k_fieldstats: the cycle is counted, and its nchains states if it was recorded
static __global__ void k_fieldstats_advance(uint64_t* ctl, int nchains) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t cycle = ctl[0] + 1;
    ctl[0] = cycle;
    if (cycle % ctl[2] == 0) ctl[1] = ctl[1] + (uint64_t)nchains;
}

// bsum != nullptr: the batch instance (bsum, bmean, bm2 in the layout of mean)
inline void launch_fieldstats(const double* x, long long nstore, int nchains, double* mean, double* m2, uint64_t* ctl,
                              hipStream_t s, double* bsum = nullptr, double* bmean = nullptr, double* bm2 = nullptr) {
    const long long npairs = nstore / 2;
    const long long per_wg = (long long)FS_NT * FS_PAIRS;
    const dim3 grid((unsigned)((npairs + per_wg - 1) / per_wg));
    double* const none = nullptr;
    if (bsum && nchains == 1)
        hipLaunchKernelGGL((k_fieldstats<1, true>), grid, dim3(FS_NT), 0, s, x, nstore, nchains, mean, m2, npairs,
                           (const uint64_t*)ctl, bsum, bmean, bm2);
    else if (bsum)
        hipLaunchKernelGGL((k_fieldstats<0, true>), grid, dim3(FS_NT), 0, s, x, nstore, nchains, mean, m2, npairs,
                           (const uint64_t*)ctl, bsum, bmean, bm2);
    else if (nchains == 1)
        hipLaunchKernelGGL((k_fieldstats<1>), grid, dim3(FS_NT), 0, s, x, nstore, nchains, mean, m2, npairs,
                           (const uint64_t*)ctl, none, none, none);
    else
        hipLaunchKernelGGL((k_fieldstats<0>), grid, dim3(FS_NT), 0, s, x, nstore, nchains, mean, m2, npairs,
                           (const uint64_t*)ctl, none, none, none);
    hipLaunchKernelGGL(k_fieldstats_advance, dim3(1), dim3(64), 0, s, ctl, nchains);
}

}  // namespace mgmc
