// mgmc_energy.hpp -- the whole-field energy of the level-0 state, reduced on the device: per chain
//     xqx = x^T A x + sum_k (B_k^T x)^2 / Sigma_k      and      fx = f^T x,
// so that E = xqx - 2 fx (+ f^T Q^{-1} f) is the chi-square observable of the chain and -E / 2 its Gaussian
// log-density up to a constant (Goodman & Sokal's slow-mode observable).  mgmc_energy evaluates the current
// state; mgmc_energy_record_* records (xqx, fx) per cycle from an op of the cycle graph (OP_ENERGY).
//
// Three reduction kernels, chosen by plan_energy (mgmc_level_plan.hpp):
//   k_energy_z<FZ, VD>     z-sweep levels (constant symmetric 7-point stencil, VD: the diagonal streamed from the
//                          vector k_vardiag_fill wrote).  With a symmetric stencil
//                              x^T A x = sum_i x_i (a_c x_i + 2 (a_x x_{i+1} + a_y x_{j+1} + a_z x_{k+1})),
//                          forward neighbours only: a tile of EN_XP x-pairs x EN_TY rows marches over EN_TZ planes,
//                          holds plane k + 1 in registers for the next step and passes row j + 1 through LDS (two
//                          buffers, one barrier per plane).  Only the tile's last row reads its y neighbour from
//                          memory (1 / EN_TY more rows) and only a chunk's last plane is read twice (1 / EN_TZ): x is
//                          read 1.13 times, against the 1.19 (y) x 2-plane halo of k_zresrestrict<7>'s staging, and
//                          the kernel needs no backward neighbour, so no halo ring at all.  The boundary (i = nx,
//                          j = ny, k = nz) and the padding are stored zeros: a forward neighbour past the lattice
//                          adds +0.0, rows past ny - 1 of an overhanging tile are not loaded and count nothing, and
//                          every interior vertex belongs to exactly one (tile, chunk).
//   k_energy_general       every other constant-stencil level: stencil_sum<DIM, NPTS> (the order of
//                          k_operator_apply), times x_i.
//   k_energy_field         per-vertex coefficients (mgmc_create_csr, reach 2 included): the row sum of k_fapply,
//                          times x_i.
// FZ: level 0's f is known to be all +0.0 (mgmc_handle::f0_zero): f is not loaded and fx = +0.0.
//
// Summation order (fixed: no atomics, nothing depends on scheduling).  A thread adds its terms in the order it
// visits them (z-march: planes ascending, the pair's first vertex then its second; general / field: EN_GZ planes
// ascending); the 64 lanes of a wavefront combine by butterfly64; lane 0 of each wavefront stores to LDS and
// thread 0 adds the wavefronts in order; the workgroup stores one (xqx, fx) partial into its own slot.  More than
// EN_RBLK partials per chain are first combined in blocks of EN_RBLK (k_energy_reduce: lane-strided from 0.0,
// butterfly).  k_energy_record, one wavefront per chain, combines the (block) partials lane-strided + butterfly,
// adds the low-rank term w_k w_k / Sigma_k, k ascending, from lr_dots' w = B^T x, and -- when recording -- appends
// (xqx, fx) to the series, folds E = xqx - 2 fx into the Welford moments and advances the counters.
//
// Counters (device memory: the graph is replayed): ctl[0] = cycles seen since enable / reset, ctl[1] = records,
// ctl[2] = stride, ctl[3] = series capacity.  Cycle ctl[0] + 1 is recorded when the stride divides it; on the
// other cycles every workgroup of the reduction kernels leaves on that uniform branch (as k_fieldstats does) and
// k_energy_record, the only writer of the counters, only counts the cycle.
//
// The shape constants below fix a summation order: unlike mgmc_tuning.hpp's they are NOT bitwise-neutral, so they
// live here and must not be derived from tune:: values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgmc_field.hpp"
#include "mgmc_kernels.hpp"

namespace mgmc {

constexpr int EN_XP = 32;               // z-march: x-pairs per tile (the z-sweep's 64-vertex row tiles)
constexpr int EN_TY = 16;               // ... rows per tile
constexpr int EN_NT = EN_XP * EN_TY;    // ... threads per workgroup (8 wavefronts)
constexpr int EN_TZ = 32;               // ... planes per chunk
constexpr int EN_GX = 64, EN_GY = 4;    // general / field: one vertex per thread, 64 x 4 per plane
constexpr int EN_GZ = 8;                // ... planes per workgroup
constexpr int EN_RBLK = 4096;           // partials per block of the second stage
constexpr int EN_CTL_WORDS = 4;         // ctl[0] cycles seen, ctl[1] records, ctl[2] stride, ctl[3] capacity

// not a recorded cycle (uniform over the launch); ctl == nullptr: mgmc_energy, always evaluated
__device__ __forceinline__ bool energy_skip(const uint64_t* __restrict__ ctl) {
    return ctl && (ctl[0] + 1) % ctl[2] != 0;
}

// the workgroup's partial: butterfly per wavefront, the wavefronts in order through LDS, one store
template <int NWAVES>
__device__ __forceinline__ void energy_store_partial(double q, double g, double (*wsum)[NWAVES], int tid,
                                                     double2* __restrict__ slot) {
    q = butterfly64(q);
    g = butterfly64(g);
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = q;
        wsum[1][tid >> 6] = g;
    }
    __syncthreads();
    if (tid == 0) {
        double sq = wsum[0][0], sg = wsum[1][0];
#pragma unroll
        for (int w = 1; w < NWAVES; ++w) {
            sq = sq + wsum[0][w];
            sg = sg + wsum[1][w];
        }
        *slot = make_double2(sq, sg);
    }
}

struct EnergyZArgs {
    Layout L;
    const double* x;    // chain 0's state, chain c's cs doubles on
    const double* f;    // ... right-hand side (not read by the FZ instances)
    const double* dg;   // VD: the level's diagonal vector (shared by the chains)
    double ac, ax, ay, az;  // centre and the three forward couplings
    long long cs;
    double2* part;      // [chain][slot]
    int nchunk;         // z chunks; blockIdx.z = chain * nchunk + chunk
    const uint64_t* ctl;
};

inline int energy_z_chunks(const Layout& L) { return (L.nz - 1 + EN_TZ - 1) / EN_TZ; }
inline long long energy_z_slots(const Layout& L) {
    return (long long)((L.nx / 2) / EN_XP) * ((L.ny - 1 + EN_TY - 1) / EN_TY) * energy_z_chunks(L);
}

template <bool FZ, bool VD>
static __global__ void __launch_bounds__(EN_NT) k_energy_z(EnergyZArgs a) {
    if (energy_skip(a.ctl)) return;
    __shared__ double2 rows[2][EN_TY][EN_XP];
    __shared__ double wsum[2][EN_NT / 64];
    const Layout& L = a.L;
    const int tid = threadIdx.x, tx = tid % EN_XP, ty = tid / EN_XP;
    const int c = (int)blockIdx.z / a.nchunk, chunk = (int)blockIdx.z % a.nchunk;
    const int i = 1 + 2 * ((int)blockIdx.x * EN_XP + tx);  // the pair (i, i + 1), i odd, i <= nx - 1
    const int j = 1 + (int)blockIdx.y * EN_TY + ty;
    const bool act = j <= L.ny - 1;              // rows past the lattice: nothing loaded, zeros counted
    const bool top = act && ty == EN_TY - 1;     // the tile's last row reads row j + 1 (<= ny, stored) itself
    const bool edge = act && tx == EN_XP - 1;    // the tile's last pair reads column i + 2 (<= nx + 1, stored) itself
    const int k0 = 1 + chunk * EN_TZ, k1 = min(k0 + EN_TZ, L.nz);  // own planes [k0, k1); plane k1 <= nz is stored
    long long p = L.at(i, j, k0);
    const double* __restrict__ xc = a.x + (long long)c * a.cs;
    const double* __restrict__ fc = a.f + (long long)c * a.cs;
    const double2 zero = make_double2(0.0, 0.0);
    // everything of plane k is loaded one step ahead
    double2 cur = zero, hy = zero, fv = zero, dv = zero;
    double xe = 0.0;
    if (act) cur = *reinterpret_cast<const double2*>(xc + p);
    if (top) hy = *reinterpret_cast<const double2*>(xc + p + L.sx);
    if (edge) xe = xc[p + 2];
    if (!FZ && act) fv = *reinterpret_cast<const double2*>(fc + p);
    if (VD && act) dv = *reinterpret_cast<const double2*>(a.dg + p);
    double accq = 0.0, accf = 0.0;
    int b = 0;
    for (int k = k0; k < k1; ++k) {
        const long long pn = p + L.sp;
        const bool more = k + 1 < k1;  // plane k + 1 is an own plane too: its row / column neighbours, f and diagonal
        double2 nxt = zero, hyn = zero, fvn = zero, dvn = zero;
        double xen = 0.0;
        if (act) nxt = *reinterpret_cast<const double2*>(xc + pn);
        if (more) {
            if (top) hyn = *reinterpret_cast<const double2*>(xc + pn + L.sx);
            if (edge) xen = xc[pn + 2];
            if (!FZ && act) fvn = *reinterpret_cast<const double2*>(fc + pn);
            if (VD && act) dvn = *reinterpret_cast<const double2*>(a.dg + pn);
        }
        rows[b][ty][tx] = cur;
        __syncthreads();
        const double2 yn = ty < EN_TY - 1 ? rows[b][ty + 1][tx] : hy;
        const double xn = tx < EN_XP - 1 ? rows[b][ty][tx + 1].x : xe;
        const double c0 = VD ? dv.x : a.ac, c1 = VD ? dv.y : a.ac;
        const double e0 = cur.x * (c0 * cur.x + 2.0 * (a.ax * cur.y + a.ay * yn.x + a.az * nxt.x));
        const double e1 = cur.y * (c1 * cur.y + 2.0 * (a.ax * xn + a.ay * yn.y + a.az * nxt.y));
        accq = accq + e0;
        accq = accq + e1;
        if (!FZ) {
            accf = accf + fv.x * cur.x;
            accf = accf + fv.y * cur.y;
        }
        cur = nxt, hy = hyn, xe = xen, fv = fvn, dv = dvn;
        p = pn;
        b ^= 1;
    }
    const long long slot = ((long long)chunk * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long long nslot = (long long)a.nchunk * gridDim.y * gridDim.x;
    energy_store_partial<EN_NT / 64>(accq, accf, wsum, tid, a.part + (long long)c * nslot + slot);
}

// ---- general / field kernels: block (EN_GX, EN_GY), grid (x blocks, y blocks, nchains * nzb), nzb blocks of
// EN_GZ planes (2D: 1) ----
inline int energy_g_zblocks(const Layout& L) { return L.dim == 3 ? (L.nz - 1 + EN_GZ - 1) / EN_GZ : 1; }
inline long long energy_g_slots(const Layout& L) {
    return (long long)((L.nx - 1 + EN_GX - 1) / EN_GX) * ((L.ny - 1 + EN_GY - 1) / EN_GY) * energy_g_zblocks(L);
}

template <int DIM, int NPTS, bool FZ>
static __global__ void __launch_bounds__(EN_GX* EN_GY) k_energy_general(Layout L, const double* __restrict__ x,
                                                                        const double* __restrict__ f, StencilArg S,
                                                                        long long cs, double2* __restrict__ part,
                                                                        int nzb, const uint64_t* __restrict__ ctl) {
    if (energy_skip(ctl)) return;
    __shared__ double wsum[2][EN_GY];
    const int c = (int)blockIdx.z / nzb, zb = (int)blockIdx.z % nzb;
    const int i = blockIdx.x * EN_GX + threadIdx.x + 1, j = blockIdx.y * EN_GY + threadIdx.y + 1;
    const bool act = i <= L.nx - 1 && j <= L.ny - 1;
    const double* __restrict__ xc = x + (long long)c * cs;
    const double* __restrict__ fc = f + (long long)c * cs;
    const int k0 = DIM == 3 ? 1 + zb * EN_GZ : 0, k1 = DIM == 3 ? min(k0 + EN_GZ, L.nz) : 1;
    double accq = 0.0, accf = 0.0;
    if (act)
        for (int k = k0; k < k1; ++k) {
            const long long p = L.at(i, j, k);
            const double xi = xc[p];
            accq = accq + xi * stencil_sum<DIM, NPTS>(xc, p, L, S);
            if (!FZ) accf = accf + fc[p] * xi;
        }
    const long long slot = ((long long)zb * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long long nslot = (long long)nzb * gridDim.y * gridDim.x;
    energy_store_partial<EN_GY>(accq, accf, wsum, threadIdx.y * EN_GX + threadIdx.x, part + (long long)c * nslot + slot);
}

template <int DIM, bool FZ>
static __global__ void __launch_bounds__(EN_GX* EN_GY) k_energy_field(Layout L, const double* __restrict__ x,
                                                                      const double* __restrict__ f, FieldArg F,
                                                                      long long cs, double2* __restrict__ part, int nzb,
                                                                      const uint64_t* __restrict__ ctl) {
    if (energy_skip(ctl)) return;
    __shared__ double wsum[2][EN_GY];
    const int c = (int)blockIdx.z / nzb, zb = (int)blockIdx.z % nzb;
    const int i = blockIdx.x * EN_GX + threadIdx.x + 1, j = blockIdx.y * EN_GY + threadIdx.y + 1;
    const bool act = i <= L.nx - 1 && j <= L.ny - 1;
    const double* __restrict__ xc = x + (long long)c * cs;
    const double* __restrict__ fc = f + (long long)c * cs;
    const int k0 = DIM == 3 ? 1 + zb * EN_GZ : 0, k1 = DIM == 3 ? min(k0 + EN_GZ, L.nz) : 1;
    double accq = 0.0, accf = 0.0;
    if (act)
        for (int k = k0; k < k1; ++k) {
            const long long p = L.at(i, j, k);
            const double* __restrict__ coef = F.coef + field_row<DIM>(F, i, j, k) * F.np;
            double s = 0.0;  // (k_fapply's row sum)
            for (int q = 0; q < F.np; ++q) s += coef[q] * xc[p + F.off[q]];
            const double xi = xc[p];
            accq = accq + xi * s;
            if (!FZ) accf = accf + fc[p] * xi;
        }
    const long long slot = ((long long)zb * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long long nslot = (long long)nzb * gridDim.y * gridDim.x;
    energy_store_partial<EN_GY>(accq, accf, wsum, threadIdx.y * EN_GX + threadIdx.x, part + (long long)c * nslot + slot);
}

// lane-strided sum of n (xqx, fx) partials from 0.0 (the loads of U of them issued together), then the butterfly
__device__ __forceinline__ double2 energy_combine(const double2* __restrict__ v, long long n, int lane) {
    double q = 0.0, g = 0.0;
    constexpr int U = 8;
    long long b = lane;
    for (; b + (U - 1) * 64 < n; b += U * 64) {
        double2 t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = v[b + u * 64];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q = q + t[u].x;
            g = g + t[u].y;
        }
    }
    for (; b < n; b += 64) {
        const double2 t = v[b];
        q = q + t.x;
        g = g + t.y;
    }
    return make_double2(butterfly64(q), butterfly64(g));
}

// second stage, more than EN_RBLK partials per chain: grid (blocks, nchains), one wavefront per block
static __global__ void __launch_bounds__(64) k_energy_reduce(const double2* __restrict__ part, long long nslot,
                                                             double2* __restrict__ part2, int nblk,
                                                             const uint64_t* __restrict__ ctl) {
    if (energy_skip(ctl)) return;
    const int b = blockIdx.x, c = blockIdx.y;
    const long long e0 = (long long)b * EN_RBLK, n = min(nslot - e0, (long long)EN_RBLK);
    const double2 s = energy_combine(part + (long long)c * nslot + e0, n, threadIdx.x);
    if (threadIdx.x == 0) part2[(long long)c * nblk + b] = s;
}

// One wavefront per chain (block of 64 * nchains threads): combines the partials, adds the low-rank term and
// stores (xqx, fx) to out[chain]; with ctl (recording) it appends to the series, folds E = xqx - 2 fx into
// mom[chain] = (n, mean, M2, pad) and advances the counters -- on a cycle that is not recorded only ctl[0].
// w: lr_dots' B^T x (m per chain), inv_sigma: 1 / Sigma_k; m = 0: no low-rank part.
static __global__ void k_energy_record(const double2* __restrict__ part, long long n, int nchains,
                                       const double* __restrict__ w, const double* __restrict__ inv_sigma, int m,
                                       double2* __restrict__ out, uint64_t* ctl, double* __restrict__ sq,
                                       double* __restrict__ sf, double* __restrict__ mom) {
    const int c = threadIdx.x >> 6, l = threadIdx.x & 63;
    uint64_t cycle = 0, nrec = 0;
    bool rec = true;
    if (ctl) {
        cycle = ctl[0] + 1;
        nrec = ctl[1];
        rec = cycle % ctl[2] == 0;
    }
    if (rec && c < nchains) {
        const double2 s = energy_combine(part + (long long)c * n, n, l);
        if (l == 0) {
            double q = s.x;
            for (int k = 0; k < m; ++k) {
                const double wk = w[(long long)c * m + k];
                q = q + wk * wk * inv_sigma[k];
            }
            if (out) out[c] = make_double2(q, s.y);
            if (ctl) {
                const uint64_t cap = ctl[3];
                if (nrec < cap) {
                    sq[(long long)c * cap + nrec] = q;
                    sf[(long long)c * cap + nrec] = s.y;
                }
                double* mc = mom + 4 * c;
                const double e = q - 2.0 * s.y;
                const double cnt = mc[0] + 1.0;
                const double delta = e - mc[1];
                const double mean = mc[1] + delta / cnt;
                mc[2] = mc[2] + delta * (e - mean);
                mc[1] = mean;
                mc[0] = cnt;
            }
        }
    }
    __syncthreads();  // every chain has read the counters
    if (ctl && threadIdx.x == 0) {
        ctl[0] = cycle;
        if (rec) ctl[1] = nrec + 1;
    }
}

}  // namespace mgmc
