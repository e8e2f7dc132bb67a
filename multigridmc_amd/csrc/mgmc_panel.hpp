// mgmc_panel.hpp -- the QoI panel: K <= 64 linear functionals z_k = b_k^T x of the level-0 state, recorded together
// per cycle with their joint statistics on the device (mgmc_qoi_panel_*).  The device counterpart of the
// reference's Statistics (nilsfriess/MultigridMC, src/auxilliary/statistics.{hh,cc}): a vector-valued observable,
// its running average and covariance (statistics.cc:5-18, :41-51), the autocovariance over a window (:19-38,
// :54-62) and tau_int (:65-80).
//
// Two kernels, both launched by the cycle's OP_PANEL (after OP_QOI; level 0's canonical buffer holds the state):
//   k_panel_dots    the block partials of every column and every chain in one launch.  Per column the contract is
//                   k_qoi_dot's, bit for bit: the column's entries ascending in blocks of QP_BLK, lane l of a
//                   wavefront sums entries l, l + 64, ... of its block from 0.0 as acc = acc + val * x, the 64 lanes
//                   combine by butterfly64.  Column k of the panel therefore records what MGMC_QOI_VECTOR records
//                   for that vector.
//                     entry-list columns: one wavefront per block, the loads of QP_U entries in flight;
//                     dense columns (every vertex listed): one wavefront takes block b of a group of up to QP_G
//                     dense columns, walks the block's vertices once with incremental (i, j, k) (k_lr_partials'
//                     walk) and loads each x once for the group: 8 (D + ceil(D / QP_G)) bytes per unknown and chain
//                     for D dense columns, against 16 D one column at a time.  A dense column's values lie in
//                     reference (entry) order, so they stream contiguously; a column whose values are all one
//                     number bit for bit (PanelWork::cflag / cval, as LRColMeta's) has no value array.
//                   QP_G and QP_U do not enter the order of any sum: a lane's entries and their order are fixed by
//                   QP_BLK and the wavefront width alone.
//   k_panel_record  one workgroup per chain, the only writer of the chain's counters.  Wavefront w combines the
//                   block partials of columns w, w + QP_NW, ...: lane-strided from 0.0, then the butterfly
//                   (k_qoi_record_vec's order) -> z[0 .. K).  Then, on a recorded cycle,
//                     1. the series keeps z while records < capacity (the first `capacity` records; the moments go on
//                        counting, as mgmc_energy_record_* does);
//                     2. mean and co-moments with cnt = n + 1, every delta from the old mean and every mean updated
//                        before the co-moments:
//                            delta_k = z_k - mean_k;  mean_k = mean_k + delta_k / cnt;
//                            C[k][l] = C[k][l] + delta_k * (z_l - mean_l)   for l >= k, with the new mean_l
//                        (the diagonal is k_qoi_record's M2 update, bit for bit; the host mirrors the upper triangle);
//                     3. the autocovariance per column over a window W (statistics.cc:19-38, the diagonal of S_k
//                        only): a ring of the last W recorded z; for lag j = 0 .. min(W, records) - 1 with
//                        N_j = records - j:  S[j] = z_now * z_lag if N_j == 1, else
//                        S[j] = S[j] + (z_now * z_lag - S[j]) / N_j.
//
// Counters (device memory, the graph is replayed), QP_CTL_WORDS per chain, chain c's copy written by chain c's
// workgroup only: ctl[0] cycles seen since enable / reset, ctl[1] records, ctl[2] stride, ctl[3] series capacity,
// ctl[4] window.  Cycle ctl[0] + 1 is recorded when the stride divides it; on the other cycles every workgroup of
// k_panel_dots leaves on that uniform branch and k_panel_record only counts the cycle.
//
// LDS: k_panel_record's z / delta / mean arrays are written for k < K before any read of them, and only k < K is
// read; k_panel_dots uses none.
//
// QP_BLK fixes a summation order (as mgmc_energy.hpp's shape constants it is NOT bitwise-neutral): it lives here
// and must not be derived from tune:: values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgmc_kernels.hpp"

namespace mgmc {

constexpr int QP_BLK = 4096;      // entries per dot-product block (QV_BLK, LR_BLK: the same order)
constexpr int QP_MAX_K = 64;      // columns
constexpr int QP_MAX_W = 256;     // autocovariance window
constexpr int QP_G = 8;           // dense columns per group (bitwise-neutral: which wavefront forms a partial)
constexpr int QP_U = 4;           // entries per lane whose loads are issued together (bitwise-neutral)
constexpr int QP_NT = 256;        // threads of k_panel_record
constexpr int QP_NW = QP_NT / 64;
constexpr int QP_CTL_WORDS = 8;   // per chain: [0] cycles seen [1] records [2] stride [3] capacity [4] window
static_assert(QP_BLK == QV_BLK, "the panel's columns follow k_qoi_dot's blocks");

// one wavefront's work: block b of an entry-list column, or of a group of dense columns
struct PanelWork {
    long long e0;         // the block's first entry in its column(s)
    int cnt;              // entries (<= QP_BLK)
    int ncol;             // columns: 1 (entry list), <= QP_G (dense group)
    int dense;            // a dense group
    int pad_;
    long long src[QP_G];  // entry list: the block's first entry in ent_off / ent_val ([0]); dense: the block's first
                          // value in dense_val (unused with cflag)
    int slot[QP_G];       // the column's partial for this block (chain c: + c * nslot)
    int cflag[QP_G];      // dense column whose every value is cval (bit for bit): no value array
    double cval[QP_G];
};

struct PanelColumn {      // k_panel_record: the column's partials
    int slot0, nblk;
};

// not a recorded cycle (uniform over the launch); ctl == nullptr: mgmc_qoi_panel_eval, always evaluated
__device__ __forceinline__ bool panel_skip(const uint64_t* __restrict__ ctl) {
    return ctl && (ctl[0] + 1) % ctl[2] != 0;
}

// grid (work items, chains), one wavefront each
static __global__ void __launch_bounds__(64) k_panel_dots(Layout L, const PanelWork* __restrict__ work,
                                                          const long long* __restrict__ ent_off,
                                                          const double* __restrict__ ent_val,
                                                          const double* __restrict__ dense_val,
                                                          const double* __restrict__ x, long long cs,
                                                          double* __restrict__ part, int nslot,
                                                          const uint64_t* __restrict__ ctl) {
    const int c = blockIdx.y, lane = threadIdx.x;
    if (panel_skip(ctl ? ctl + (long long)c * QP_CTL_WORDS : nullptr)) return;
    const PanelWork w = work[blockIdx.x];
    const double* __restrict__ xc = x + (long long)c * cs;
    double* __restrict__ pc = part + (long long)c * nslot;
    const int cnt = lane < w.cnt ? (w.cnt - lane + 63) / 64 : 0;  // entries of this lane
    if (!w.dense) {
        const long long q0 = w.src[0] + lane;
        double acc = 0.0;
        for (int base = 0; base < cnt; base += QP_U) {
            double a[QP_U], v[QP_U];
#pragma unroll
            for (int u = 0; u < QP_U; ++u)
                if (base + u < cnt) {
                    const long long q = q0 + 64ll * (base + u);
                    a[u] = ent_val[q];
                    v[u] = xc[ent_off[q]];
                }
#pragma unroll
            for (int u = 0; u < QP_U; ++u)
                if (base + u < cnt) acc = acc + a[u] * v[u];
        }
        acc = butterfly64(acc);
        if (lane == 0) pc[w.slot[0]] = acc;
        return;
    }
    // dense group: entry e of the block is vertex e0 + e in reference order
    const long long e1 = w.e0 + lane;
    const int nxi = L.nx - 1, nyi = L.ny - 1;
    const long long r = e1 / nxi;
    int i = (int)(e1 - r * nxi) + 1;
    int j = (int)(r % nyi) + 1;
    int kk = L.dim == 3 ? (int)(r / nyi) + 1 : 0;
    double acc[QP_G];
#pragma unroll
    for (int g = 0; g < QP_G; ++g) acc[g] = 0.0;
    for (int base = 0; base < cnt; base += QP_U) {
        long long p[QP_U];
        double v[QP_U], a[QP_G][QP_U];
#pragma unroll
        for (int u = 0; u < QP_U; ++u) {
            p[u] = L.at(i, j, kk);
            i += 64;  // advance by 64 entries (nxi may be < 64: carry repeatedly)
            while (i > nxi) {
                i -= nxi;
                if (++j > nyi) {
                    j = 1;
                    ++kk;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QP_U; ++u)
            if (base + u < cnt) {
                v[u] = xc[p[u]];
#pragma unroll
                for (int g = 0; g < QP_G; ++g)
                    if (g < w.ncol) a[g][u] = w.cflag[g] ? w.cval[g] : dense_val[w.src[g] + lane + 64ll * (base + u)];
            }
#pragma unroll
        for (int g = 0; g < QP_G; ++g)
#pragma unroll
            for (int u = 0; u < QP_U; ++u)
                if (g < w.ncol && base + u < cnt) acc[g] = acc[g] + a[g][u] * v[u];
    }
#pragma unroll
    for (int g = 0; g < QP_G; ++g) {
        const double t = butterfly64(acc[g]);
        if (lane == 0 && g < w.ncol) pc[w.slot[g]] = t;
    }
}

// What k_panel_record writes, per chain: with ctl == nullptr (mgmc_qoi_panel_eval) only out[chain][K].
struct PanelRecordArgs {
    const PanelColumn* col;  // K
    const double* part;      // [chain][nslot]
    int K, nslot;
    uint64_t* ctl;           // [chain][QP_CTL_WORDS], nullptr: evaluate only
    double* out;             // [chain][K], or nullptr
    double* series;          // [chain][capacity][K]
    double* mom;             // [chain][1 + K + K * K]: cnt, mean, C (row-major, upper triangle)
    double* ring;            // [chain][window][K]
    double* S;               // [chain][K][window]
};

static __global__ void __launch_bounds__(QP_NT) k_panel_record(PanelRecordArgs a) {
    __shared__ double z[QP_MAX_K], delta[QP_MAX_K], mean[QP_MAX_K];
    const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = a.K;
    uint64_t* ctl = a.ctl ? a.ctl + (long long)c * QP_CTL_WORDS : nullptr;
    uint64_t cycle = 0, nrec = 0, cap = 0, W = 1;
    bool rec = true;
    if (ctl) {
        cycle = ctl[0] + 1;
        nrec = ctl[1];
        rec = cycle % ctl[2] == 0;
        cap = ctl[3];
        W = ctl[4];
    }
    if (rec) {  // (uniform over the workgroup)
        const double* __restrict__ pc = a.part + (long long)c * a.nslot;
        for (int k = wave; k < K; k += QP_NW) {
            const PanelColumn pk = a.col[k];
            double acc = 0.0;
            for (int b = lane; b < pk.nblk; b += 64) acc = acc + pc[pk.slot0 + b];
            acc = butterfly64(acc);
            if (lane == 0) z[k] = acc;
        }
        __syncthreads();
        if (a.out && tid < K) a.out[(long long)c * K + tid] = z[tid];
        if (ctl) {
            double* mc = a.mom + (long long)c * (1 + K + K * K);
            const double cnt = mc[0] + 1.0;
            if (tid < K) {
                if (nrec < cap) a.series[((long long)c * cap + nrec) * K + tid] = z[tid];
                a.ring[((long long)c * W + nrec % W) * K + tid] = z[tid];
                const double d = z[tid] - mc[1 + tid];
                delta[tid] = d;
                mean[tid] = mc[1 + tid] + d / cnt;
            }
            __syncthreads();  // z, delta and the new means of every column; every thread has read mc[0]
            if (tid < K) mc[1 + tid] = mean[tid];
            if (tid == 0) mc[0] = cnt;
            double* C = mc + 1 + K;
            for (int q = tid; q < K * K; q += QP_NT) {
                const int k = q / K, l = q - k * K;
                if (l >= k) C[q] = C[q] + delta[k] * (z[l] - mean[l]);
            }
            // autocovariance: lag j reads the record written j records ago (another ring slot than this cycle's)
            const uint64_t nrecs = nrec + 1;
            const int nlag = (int)(nrecs < W ? nrecs : W);
            double* Sc = a.S + (long long)c * K * W;
            const double* rc = a.ring + (long long)c * W * K;
            for (int q = tid; q < K * nlag; q += QP_NT) {
                const int k = q / nlag, j = q - k * nlag;
                const double zl = j == 0 ? z[k] : rc[((nrec - j) % W) * K + k];
                const double prod = z[k] * zl;
                const uint64_t nj = nrecs - j;
                double* s = Sc + (long long)k * W + j;
                if (nj == 1) *s = prod;
                else *s = *s + (prod - *s) / (double)nj;
            }
        }
    }
    __syncthreads();  // every wavefront has read the counters
    if (ctl && tid == 0) {
        ctl[0] = cycle;
        if (rec) ctl[1] = nrec + 1;
    }
}

}  // namespace mgmc
