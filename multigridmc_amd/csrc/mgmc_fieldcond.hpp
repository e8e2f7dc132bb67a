// mgmc_fieldcond.hpp -- Rao-Blackwellised field statistics (mgmc_field_stats_enable_cond): instead of the level-0
// state x the running fields fold its one-vertex conditional mean
//     c_i = x_i + (f_i - y_i) / d_i,    y = Q x,    d_i = Q_ii,
// one Jacobi step applied to the sample.  For x ~ N(Q^{-1} f, Q^{-1}): E[c] = Q^{-1} f and
// diag Cov(c) = diag(Q^{-1}) - D^{-1}, so mean(c) estimates the posterior mean and 1 / d_i + var(c_i) the
// marginal variance, with only the smaller part of the variance left to Monte Carlo.
//
// The bits of c (fixed: the tests mirror them in numpy):
//     y_i   the row sum of mgmc_operator_apply on level 0 (stencil_sum / k_fapply: ascending from 0.0, separate
//           multiply and add), then the low-rank patch as launch_operator_apply adds it;
//     f     level 0's right-hand side as mgmc_set_rhs stored it, +0.0 while mgmc_handle::f0_zero holds;
//     d_i   the scalar a_cc, or the d-field of mgmc_fieldcond_host.hpp (per-vertex coefficients, a low-rank part);
//     c_i = x_i + (f_i - y_i) / d_i in plain IEEE double.
// c then takes k_fieldstats' statements (mgmc_fieldstats.hpp) in x's place, chains in order.
//
// Two paths, chosen by plan_fieldcond (mgmc_level_plan.hpp):
//   k_fieldcond_z<FZ, BATCH>  one chain on a z-sweep level with a constant stencil and no low-rank part: stencil and
//                             Welford fold in one z-march.  A tile of FC_XP x-pairs x FC_TY rows marches over FC_TZ
//                             planes; a thread keeps its pair of the planes k - 1, k, k + 1 in registers and passes
//                             the pair of plane k through LDS for the x +- 1 and y +- 1 neighbours (two buffers, one
//                             barrier per plane, as k_energy_z).  The tile's edge pairs / rows read their outer
//                             neighbour from memory: the lattice's boundary is stored (zeros), so those loads need no
//                             lattice test.  Rows past ny - 1 of an overhanging tile load and store nothing and pass
//                             zeros (= the stored boundary row ny) through LDS.  x is read
//                             (FC_TY + 2) / FC_TY x (FC_TZ + 2) / FC_TZ times (+ 2 edge doubles per 64) = 1.2 times.
//                             mean / M2 and the batch fields move as non-temporal 16-byte pairs (no reuse before the
//                             next recorded cycle), x and f with plain loads; the FZ instance does not read f.  A
//                             vertex's value does not depend on the tile it falls in: the tile constants below are
//                             bitwise-neutral.
//   two-pass                  everything else.  launch_operator_apply writes y of every chain into the handle's
//                             c buffer (nchains x nstore, zeroed once at enable: only interior vertices are ever
//                             written), k_fieldcond_c turns it into c in place, and launch_fieldstats folds that
//                             buffer as it folds x.
// Both read the counters of mgmc_fieldstats.hpp and never write them; k_fieldstats_advance follows on the stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgmc_fieldstats.hpp"
#include "mgmc_kernels.hpp"

namespace mgmc {

constexpr int FC_XP = 32;             // z-march: x-pairs per tile (the z-sweep's 64-vertex row tiles)
constexpr int FC_TY = 16;             // ... rows per tile
constexpr int FC_NT = FC_XP * FC_TY;  // ... threads per workgroup (8 wavefronts)
constexpr int FC_TZ = 32;             // ... planes per chunk

struct FieldCondZArgs {
    Layout L;
    const double* x;  // the chain's state
    const double* f;  // ... right-hand side (not read by the FZ instances)
    double a[7];      // stencil_sum<3, 7>'s coefficients in its order: z-, y-, x-, centre, x+, y+, z+
    double d;         // Q_ii
    double *mean, *m2, *bsum, *bmean, *bm2;  // the fields of k_fieldstats (the batch fields: BATCH instances)
    const uint64_t* ctl;
};

inline int fieldcond_z_chunks(const Layout& L) { return (L.nz - 1 + FC_TZ - 1) / FC_TZ; }

template <bool FZ, bool BATCH>
static __global__ void __launch_bounds__(FC_NT) k_fieldcond_z(FieldCondZArgs a) {
    const uint64_t cycle = a.ctl[0] + 1, stride = a.ctl[2];
    if (cycle % stride != 0) return;  // thinning: not a recorded cycle (uniform over the launch)
    const double cnt = (double)(a.ctl[1] + 1);
    [[maybe_unused]] bool batch_end = false;
    [[maybe_unused]] double per = 0.0, cntb = 0.0;
    if constexpr (BATCH) {
        const uint64_t r = cycle / stride, blen = a.ctl[3];
        batch_end = r % blen == 0;
        per = (double)blen;  // (one chain)
        cntb = (double)(r / blen);
    }
    __shared__ double2 rows[2][FC_TY][FC_XP];
    const Layout& L = a.L;
    const int tid = threadIdx.x, tx = tid % FC_XP, ty = tid / FC_XP;
    const int i = 1 + 2 * ((int)blockIdx.x * FC_XP + tx);  // the pair (i, i + 1), i odd, i <= nx - 1
    const int j = 1 + (int)blockIdx.y * FC_TY + ty;
    const bool act = j <= L.ny - 1;           // rows past the lattice: nothing loaded or stored
    const bool lo = act && ty == 0;           // the tile's first row reads row j - 1 (>= 0, stored) itself
    const bool hi = act && ty == FC_TY - 1;   // ... its last row reads row j + 1 (<= ny, stored)
    const bool left = act && tx == 0;         // the first pair reads column i - 1 (>= 0, stored)
    const bool right = act && tx == FC_XP - 1;  // the last pair reads column i + 2 (<= nx + 1, stored)
    const bool last = i + 1 == L.nx;          // the pair's second vertex is the boundary: its c stays +0.0
    const int k0 = 1 + (int)blockIdx.z * FC_TZ, k1 = min(k0 + FC_TZ, L.nz);  // own planes [k0, k1)
    long long p = L.at(i, j, k0);
    const double* __restrict__ x = a.x;
    const double* __restrict__ f = a.f;
    fs_pair* __restrict__ mp = reinterpret_cast<fs_pair*>(a.mean);
    fs_pair* __restrict__ sp = reinterpret_cast<fs_pair*>(a.m2);
    [[maybe_unused]] fs_pair* __restrict__ bsp = reinterpret_cast<fs_pair*>(a.bsum);
    [[maybe_unused]] fs_pair* __restrict__ bmp = reinterpret_cast<fs_pair*>(a.bmean);
    [[maybe_unused]] fs_pair* __restrict__ bqp = reinterpret_cast<fs_pair*>(a.bm2);
    const double2 zero = make_double2(0.0, 0.0);
    // planes k - 1 and k of the own pair; the edge neighbours of plane k are loaded one step ahead
    double2 prv = zero, cur = zero, yd = zero, yu = zero;
    double xl = 0.0, xr = 0.0;
    if (act) {
        prv = *reinterpret_cast<const double2*>(x + p - L.sp);
        cur = *reinterpret_cast<const double2*>(x + p);
    }
    if (lo) yd = *reinterpret_cast<const double2*>(x + p - L.sx);
    if (hi) yu = *reinterpret_cast<const double2*>(x + p + L.sx);
    if (left) xl = x[p - 1];
    if (right) xr = x[p + 2];
    int b = 0;
    for (int k = k0; k < k1; ++k) {
        const long long pn = p + L.sp;
        const bool more = k + 1 < k1;  // plane k + 1 is an own plane too: its edge neighbours
        double2 nxt = zero, ydn = zero, yun = zero, fv = zero;
        double xln = 0.0, xrn = 0.0;
        fs_pair m = {0.0, 0.0}, s = {0.0, 0.0};
        [[maybe_unused]] fs_pair bs = {0.0, 0.0}, bm = {0.0, 0.0}, bq = {0.0, 0.0};
        if (act) {
            nxt = *reinterpret_cast<const double2*>(x + pn);  // (plane k1 <= nz is stored)
            if (!FZ) fv = *reinterpret_cast<const double2*>(f + p);
            m = __builtin_nontemporal_load(mp + p / 2);
            s = __builtin_nontemporal_load(sp + p / 2);
            if constexpr (BATCH) {
                bs = __builtin_nontemporal_load(bsp + p / 2);
                if (batch_end) {
                    bm = __builtin_nontemporal_load(bmp + p / 2);
                    bq = __builtin_nontemporal_load(bqp + p / 2);
                }
            }
        }
        if (more) {
            if (lo) ydn = *reinterpret_cast<const double2*>(x + pn - L.sx);
            if (hi) yun = *reinterpret_cast<const double2*>(x + pn + L.sx);
            if (left) xln = x[pn - 1];
            if (right) xrn = x[pn + 2];
        }
        rows[b][ty][tx] = cur;
        __syncthreads();
        const double2 ym = ty > 0 ? rows[b][ty - 1][tx] : yd;
        const double2 yp = ty < FC_TY - 1 ? rows[b][ty + 1][tx] : yu;
        const double xm = tx > 0 ? rows[b][ty][tx - 1].y : xl;
        const double xp = tx < FC_XP - 1 ? rows[b][ty][tx + 1].x : xr;
        if (act) {
            // stencil_sum<3, 7>: ascending from 0.0, separate multiply and add
            double y0 = 0.0, y1 = 0.0;
            y0 += a.a[0] * prv.x;
            y1 += a.a[0] * prv.y;
            y0 += a.a[1] * ym.x;
            y1 += a.a[1] * ym.y;
            y0 += a.a[2] * xm;
            y1 += a.a[2] * cur.x;
            y0 += a.a[3] * cur.x;
            y1 += a.a[3] * cur.y;
            y0 += a.a[4] * cur.y;
            y1 += a.a[4] * xp;
            y0 += a.a[5] * yp.x;
            y1 += a.a[5] * yp.y;
            y0 += a.a[6] * nxt.x;
            y1 += a.a[6] * nxt.y;
            const double v0 = cur.x + (fv.x - y0) / a.d;
            const double v1 = last ? 0.0 : cur.y + (fv.y - y1) / a.d;
            // k_fieldstats' statements, one chain
            const double d0 = v0 - m.x, d1 = v1 - m.y;
            const double a0 = m.x + d0 / cnt, a1 = m.y + d1 / cnt;
            s.x = s.x + d0 * (v0 - a0);
            s.y = s.y + d1 * (v1 - a1);
            m.x = a0;
            m.y = a1;
            if constexpr (BATCH) {
                bs.x = bs.x + v0;
                bs.y = bs.y + v1;
                if (batch_end) {
                    const double b0 = bs.x / per, b1 = bs.y / per;
                    const double e0 = b0 - bm.x, e1 = b1 - bm.y;
                    const double g0 = bm.x + e0 / cntb, g1 = bm.y + e1 / cntb;
                    bq.x = bq.x + e0 * (b0 - g0);
                    bq.y = bq.y + e1 * (b1 - g1);
                    bm.x = g0;
                    bm.y = g1;
                    bs.x = 0.0;
                    bs.y = 0.0;
                    __builtin_nontemporal_store(bm, bmp + p / 2);
                    __builtin_nontemporal_store(bq, bqp + p / 2);
                }
                __builtin_nontemporal_store(bs, bsp + p / 2);
            }
            __builtin_nontemporal_store(m, mp + p / 2);
            __builtin_nontemporal_store(s, sp + p / 2);
        }
        prv = cur, cur = nxt, yd = ydn, yu = yun, xl = xln, xr = xrn;
        p = pn;
        b ^= 1;
    }
}

// ---- two-pass: c = x + (f - y) / d in place over y, interior vertices of every chain ----
// block (64, 4), grid (x blocks, y blocks, nchains * planes); dfield: d per stored vertex (shared by the chains),
// nullptr: the scalar dscal.  FZ: f is known to be all +0.0 and is not read.
template <int DIM, bool FZ>
static __global__ void __launch_bounds__(256) k_fieldcond_c(Layout L, const double* __restrict__ x,
                                                            const double* __restrict__ f, double* __restrict__ yc,
                                                            const double* __restrict__ dfield, double dscal,
                                                            long long cs, int nplanes,
                                                            const uint64_t* __restrict__ ctl) {
    if ((ctl[0] + 1) % ctl[2] != 0) return;  // not a recorded cycle (uniform over the launch)
    const int c = (int)blockIdx.z / nplanes;
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y * blockDim.y + threadIdx.y + 1;
    const int k = DIM == 3 ? (int)blockIdx.z % nplanes + 1 : 0;
    if (i > L.nx - 1 || j > L.ny - 1) return;
    const long long p = L.at(i, j, k), pc = (long long)c * cs + p;
    const double d = dfield ? dfield[p] : dscal;
    const double fi = FZ ? 0.0 : f[pc];
    yc[pc] = x[pc] + (fi - yc[pc]) / d;
}

// the centre coefficient of every interior vertex of a per-vertex-coefficient level, into a zeroed padded vector
template <int DIM>
static __global__ void __launch_bounds__(256) k_fieldcond_diag(Layout L, FieldArg F, double* __restrict__ dg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y * blockDim.y + threadIdx.y + 1;
    const int k = DIM == 3 ? (int)blockIdx.z + 1 : 0;
    if (i > L.nx - 1 || j > L.ny - 1) return;
    dg[L.at(i, j, k)] = F.coef[field_row<DIM>(F, i, j, k) * F.np + F.diag];
}

// the fused launch and the counters' advance (one chain)
inline void launch_fieldcond_z(const FieldCondZArgs& a, bool fz, uint64_t* ctl, hipStream_t s) {
    const dim3 grid((a.L.nx / 2) / FC_XP, (a.L.ny - 1 + FC_TY - 1) / FC_TY, fieldcond_z_chunks(a.L));
    const bool batch = a.bsum != nullptr;
    if (fz && batch) hipLaunchKernelGGL((k_fieldcond_z<true, true>), grid, dim3(FC_NT), 0, s, a);
    else if (fz) hipLaunchKernelGGL((k_fieldcond_z<true, false>), grid, dim3(FC_NT), 0, s, a);
    else if (batch) hipLaunchKernelGGL((k_fieldcond_z<false, true>), grid, dim3(FC_NT), 0, s, a);
    else hipLaunchKernelGGL((k_fieldcond_z<false, false>), grid, dim3(FC_NT), 0, s, a);
    hipLaunchKernelGGL(k_fieldstats_advance, dim3(1), dim3(64), 0, s, ctl, 1);
}

}  // namespace mgmc
