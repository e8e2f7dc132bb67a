// mgmc_level_plan.hpp -- which kernels a level runs, decided once (host logic, no HIP:
// tests/cpp/level_plan_host.cpp compiles it alone).
//
// mgmc_create fills Level::sweep (the level's noisy Gibbs sweep) and Level::res (the residual + restriction
// onto the next coarser level) from the level's shape, the handle's MGMC_DISABLE switches and the tail
// start.  Everything that needs the choice -- the launchers, the passes over the op list (build_tails_only,
// mark_zero_inputs, mark_rhs_zero, plan_drawn_noise), the layout check and mgmc_level_kernels' labels --
// reads the plan; none of them works it out again from the shapes.  A new kernel instance gets its
// condition here (plan_sweep / plan_residual) and its launch in the one switch that reads the plan
// (launch_level_sweep / launch_residual_restrict, mgmc_capi.hip).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cstddef>
#include <string>

#include "mgmc_tuning.hpp"

namespace mgmc_host {

// Kernel-path switches.  Every default fast path has a general fallback (the same arithmetic, bitwise
// equal); MGMC_DISABLE=<comma list> turns fast paths off at mgmc_create so the variant tests
// (tests/test_gpu_parity.py test_variant_cycles_bitwise, test_gpu_lowrank.py) can run the fallbacks
// on shapes where the fast path would be taken.  Read once per handle; unknown tokens are an error.
enum PathFlag : uint32_t {
    PATH_NO_TAIL = 1u << 0,               // coarsest levels as separate launches instead of k_tail
    PATH_NO_FUSE_PROLONG = 1u << 1,       // separate prolongate-add pass before the first post-sweep
    PATH_NO_QUADS = 1u << 2,              // colour-pair passes instead of two pairs per launch
    PATH_NO_RB2D = 1u << 3,               // 2D fine level: colour passes instead of k_rb2d
    PATH_NO_ZSWEEP = 1u << 4,             // 3D fine level: colour passes instead of k_zsweep_rb7
    PATH_NO_PAIRS = 1u << 5,              // Galerkin levels: per-colour passes instead of pair passes
    PATH_NO_ZRESTRICT = 1u << 6,          // residual + restriction: per-point gather kernel
    PATH_NO_LR_SMALL = 1u << 7,           // low-rank fix: generic multi-launch path instead of k_lr_small
    PATH_NO_LR_MERGE = 1u << 8,           // low-rank: separate restore / patch launches around restriction
    PATH_NO_LR_DENSE = 1u << 9,           // dense low-rank column: the row lists over every vertex
    PATH_NO_CHOL_DENSE = 1u << 10,        // coarse Cholesky: the blocked banded solves at any size
    PATH_NO_JSWEEP = 1u << 11,            // 3D Galerkin levels of 64 / 128 pairs: colour-pair passes, not j-marching halves
    PATH_NO_QRESTRICT = 1u << 12,         // 2D Galerkin levels: last pre-sweep and residual + restriction as two launches
    PATH_NO_PROLONG_Z = 1u << 13,         // big 3D levels: the per-point prolongation instead of the z-marching one
    PATH_NO_XZERO = 1u << 14,             // the restriction zeroes x_{l+1} and its first pre-sweep loads it
    PATH_NO_FOLD = 1u << 15,              // 3D fold levels: residuals in the reference's CSR order, not fold27's
    PATH_NO_POST_NOISE = 1u << 16,        // every sweep draws its own noise (none drawn by a restriction / tail launch)
};

struct PathToken {
    const char* name;
    uint32_t flag;
};
constexpr PathToken kPathTokens[] = {
    {"tail", PATH_NO_TAIL},           {"fuse_prolong", PATH_NO_FUSE_PROLONG},
    {"quads", PATH_NO_QUADS},         {"rb2d", PATH_NO_RB2D},
    {"zsweep", PATH_NO_ZSWEEP},       {"pairs", PATH_NO_PAIRS},
    {"zrestrict", PATH_NO_ZRESTRICT}, {"lr_small", PATH_NO_LR_SMALL},
    {"lr_merge", PATH_NO_LR_MERGE},   {"lr_dense", PATH_NO_LR_DENSE},
    {"chol_dense", PATH_NO_CHOL_DENSE}, {"jsweep", PATH_NO_JSWEEP},
    {"qrestrict", PATH_NO_QRESTRICT}, {"prolong_z", PATH_NO_PROLONG_Z},
    {"xzero", PATH_NO_XZERO},         {"fold", PATH_NO_FOLD},
    {"post_noise", PATH_NO_POST_NOISE},
};

// parse MGMC_DISABLE; returns false (and the offending token in *bad) for an unknown token
inline bool read_path_flags(uint32_t* flags, std::string* bad) {
    *flags = 0;
    const char* e = getenv("MGMC_DISABLE");
    if (!e) return true;
    std::string list(e);
    size_t pos = 0;
    while (pos <= list.size()) {
        size_t end = list.find(',', pos);
        if (end == std::string::npos) end = list.size();
        const std::string tok = list.substr(pos, end - pos);
        if (!tok.empty()) {
            bool found = false;
            for (const PathToken& t : kPathTokens)
                if (tok == t.name) {
                    *flags |= t.flag;
                    found = true;
                }
            if (!found) {
                *bad = tok;
                return false;
            }
        }
        pos = end + 1;
    }
    return true;
}

// x-pairs per tile of the z-marching sweep (mgmc_zsweep.hpp; the other tile constants: mgmc_internal.hpp)
constexpr int ZS_XP = 32;

// what the plan of one level depends on
struct LevelShape {
    int dim;
    int npoints;       // stencil size: 5 / 7 on a fine FD level, 9 / 27 on Galerkin levels
    int nx, ny, nz;    // cells per direction (nz = 0 in 2D)
    bool field;        // per-vertex coefficients (mgmc_create_csr)
    bool fd_symmetric; // the stencil's -x / +x, -y / +y, -z / +z couplings are equal (the z-sweep folds a
                       // symmetric 7-point FD stencil to 4 coefficients)
    bool fold;         // reflection-symmetric 27-point stencil whose residuals take the class-folded sum (Level::fold)
    bool has_coarser;  // not the coarsest level
    bool vardiag = false;  // a field level whose matrix is a constant symmetric axis-neighbour stencil plus a diagonal
                           // field (mgmc_vardiag_of_csr; st = the six couplings): the shifted-Laplace FD operator
                           // with any correlation-length model
};

// A variable-diagonal fine level runs the z-marching kernels' VD instances (mgmc_zsweep.hpp, mgmc_zrestrict.hpp):
// the constant 7-point stencil with the centre coefficient, omega / a_cc and the noise scale streamed per vertex.
// The z-sweep's conditions (below) on a field level; MGMC_DISABLE=zsweep leaves the level to the field
// kernels.
inline bool vardiag_eligible(const LevelShape& sh, uint32_t paths) {
    return sh.field && sh.vardiag && sh.dim == 3 && sh.npoints == 7 && sh.fd_symmetric && sh.has_coarser &&
           (sh.nx % (2 * ZS_XP)) == 0 && !(paths & PATH_NO_ZSWEEP);
}

// ---- the level's noisy Gibbs sweep ----
enum class SweepKernel {
    COLOUR,  // one launch per colour (k_sweep_rb / k_sweep_mc), in place
    FIELD,   // ... of a per-vertex-coefficient level (k_fsweep), in place
    PAIRS,   // Galerkin level swept in colour-pair passes (k_sweep_pairs, mgmc_gsweep.hpp), in place
    QUADS,   // ... two pairs per launch, out of place (k_sweep_quads)
    JSWEEP,  // ... j-marching half-sweeps, out of place (k_jsweep_half, mgmc_jsweep.hpp)
    RB2D,    // 2D 5-point level: one-launch red-black sweep, out of place (k_rb2d)
    ZSWEEP,  // fused z-marching red-black sweep, out of place (k_zsweep_rb7)
};

// out-of-place sweeps: x <-> x2
inline bool sweep_pingpong(SweepKernel k) {
    return k == SweepKernel::ZSWEEP || k == SweepKernel::QUADS || k == SweepKernel::JSWEEP || k == SweepKernel::RB2D;
}
// the kernels that address a level in x-pairs (the layout check's LF_PAIRS family)
inline bool sweep_pair_items(SweepKernel k) {
    return k == SweepKernel::PAIRS || k == SweepKernel::QUADS || k == SweepKernel::JSWEEP;
}

// colour-pair passes of a Galerkin 9/27-point level (in place): forward colours (0,1), (2,3), ...,
// backward (7,6), (5,4), ... -- 2^(d-1) passes per sweep
inline bool pairs_eligible(const LevelShape& sh) {
    return (sh.npoints == 27 || sh.npoints == 9) && sh.nx / 2 >= 1 && sh.nx / 2 <= 256 && sh.nx % 2 == 0;
}

// both colour pairs of a k-parity half per launch (k_sweep_quads): on levels with rows of <= 64
// pairs, where each pair pass is launch-latency bound and halving the launches pays (256^3: 63^3
// level 4 x 5.0 -> 2 x 7.6 us, 31^3 level 4 x 4.8 -> 2 x 6.3 us per sweep; round 4, 127^3 level with
// the folded stencil and xzero: 8 x 8 -> 61 us per cycle, 256^3 cycle -8 us), and on every 2D pair-pass
// level (2D 1024^2 FD cycle 0.135 -> 0.129 ms, FEM 0.147 -> 0.139 ms; A/B in one box call).  On the
// large 3D levels it loses (512^3 level 1: 2 x 105 us against 4 x 41 us per sweep): the
// second pair's loads wait for the first pair's rows.  Levels that k_tail runs are left to it (plan_sweep).
inline bool quads_eligible(const LevelShape& sh, uint32_t paths) {
    if (!pairs_eligible(sh) || (paths & PATH_NO_QUADS)) return false;
    return sh.dim == 2 || sh.nx / 2 <= mgmc::tune::QUADS_MAXPAIR;
}

// j-marching half-sweeps (k_jsweep_half): 3D 27-point levels with rows of 128 or 256 pairs (nx = 256: level 1
// at 512^3; nx = 512: the FEM prior's fine level at 512^3), x read about 1.5 times per half instead of once
// per colour-pair pass (DESIGN.md sections 3a, 3c; 512^3 FEM cycle 4.65 -> 3.76 ms).
// With 64-pair rows (512^3 level 2, 256^3 level 1) the kernel is slower than the pair passes (2 x 21 against
// 4 x 8 us per sweep at 127^3, 256^3 cycle 0.484 -> 0.503 ms): those levels are latency-bound, and the
// march's chunks are short.
inline bool jsweep_eligible(const LevelShape& sh, uint32_t paths) {
    return sh.dim == 3 && sh.npoints == 27 && (sh.nx == 256 || sh.nx == 512) &&
           sh.ny >= 2 && sh.nz >= 2 &&
           !(paths & PATH_NO_JSWEEP);
}

// 3D quad-pass rows of npair dividing 64 (127^3 / 63^3 / 31^3 ...): whole rows per wavefront, the window's outer
// columns by lane shifts (k_sweep_quads LANES); every other row length takes the three-load window
// (mgmc_level_kernels: quads=window)
inline bool quads_lanes(int dim, int npair) { return dim == 3 && 64 % npair == 0 && mgmc::tune::QUADS_LANES != 0; }

// ---- launch plan of one k_jsweep_half launch (launch_jsweep; replayed by mgmc_layout_check.hpp) ----
// LDS of a workgroup: JSWEEP_RING_ROWS rows x 3 planes of 2 np + 8 doubles and the Box-Muller tables
// (log reduction (rc, hi, lo) x 64 + cos / sin 130)
constexpr int JSWEEP_RING_ROWS = 8;
constexpr int JSWEEP_TAB_DOUBLES = 322;
inline size_t jsweep_lds_bytes(int np) {
    return (size_t)(JSWEEP_RING_ROWS * 3 * (2 * np + 8) + JSWEEP_TAB_DOUBLES) * sizeof(double);
}
struct JSweepPlan {
    int kp, jA, nk, nsteps, spc, nchunk, nb;
};
// the half's nk own planes, each cut into nchunk chunks of spc steps: as many chunks as `rounds` rounds of the
// resident workgroup slots (LDS-bound, 160 KB per CU) hold, at most one per step
inline JSweepPlan jsweep_plan_dims(int ny, int nz, bool forward, int half, int num_cu, size_t lds_bytes, int rounds) {
    JSweepPlan p;
    const int slots = (int)std::max<size_t>(1, (160 * 1024) / lds_bytes) * num_cu * rounds;
    p.jA = forward ? 0 : 1;
    p.nsteps = (ny - p.jA) / 2 + 1;
    p.kp = forward ? half : 1 - half;
    const int first = 2 - p.kp;
    p.nk = first > nz - 1 ? 0 : (nz - 1 - first) / 2 + 1;
    p.spc = p.nchunk = p.nb = 0;
    if (p.nk == 0) return p;
    const int nchunk = std::max(1, std::min(p.nsteps, slots / p.nk));
    p.spc = (p.nsteps + nchunk - 1) / nchunk;
    p.nchunk = (p.nsteps + p.spc - 1) / p.spc;
    p.nb = (p.nk * p.nchunk + 7) / 8 * 8;
    return p;
}

// level: the level's index; tail_start: the first level k_tail can take by size (tail_start_by_size; -1 none):
// the levels from there on keep in-place sweeps (no quads, no j-marching), so the tail can run them
inline SweepKernel plan_sweep(const LevelShape& sh, uint32_t paths, int level, int tail_start) {
    if (vardiag_eligible(sh, paths)) return SweepKernel::ZSWEEP;  // (its VD instance: Level::vardiag)
    if (sh.field) return SweepKernel::FIELD;
    // fused z-marching sweep: fine 3D 7-point levels whose row splits into 64-pair tiles
    if (sh.dim == 3 && sh.npoints == 7 && sh.fd_symmetric && sh.has_coarser && (sh.nx % (2 * ZS_XP)) == 0 &&
        !(paths & PATH_NO_ZSWEEP))
        return SweepKernel::ZSWEEP;
    if (sh.dim == 2 && sh.npoints == 5 && sh.has_coarser && !(paths & PATH_NO_RB2D)) return SweepKernel::RB2D;
    if (!pairs_eligible(sh) || (paths & PATH_NO_PAIRS)) return SweepKernel::COLOUR;
    const bool before_tail = tail_start < 0 || level < tail_start;
    if (before_tail && jsweep_eligible(sh, paths)) return SweepKernel::JSWEEP;
    if (before_tail && quads_eligible(sh, paths)) return SweepKernel::QUADS;
    return SweepKernel::PAIRS;
}

// ---- the residual + restriction from a level onto the next coarser one ----
enum class ResidualKind {
    NONE,    // the coarsest level
    FIELD,   // per-vertex coefficients: k_fresidual into the level's scratch, then k_restrict
    GATHER,  // one thread per coarse point (k_residual_restrict<dim, npoints>)
    ZMARCH,  // z-marching tiles of cx x cy coarse points, nt threads (k_zresrestrict, mgmc_zrestrict.hpp)
};

struct ResidualPlan {
    ResidualKind kind = ResidualKind::NONE;
    int npoints = 0;          // the fine level's stencil size
    int cx = 0, cy = 0, nt = 0;  // ZMARCH: coarse points per tile in x and y, threads per workgroup
    bool small = false;       // ZMARCH: the one-wavefront 16 x 4 tiles
    bool sym = false;         // the fold instance (27-point: fold27's residual)
    bool lrf = false;         // has an LRF instance: a low-rank level's right-hand side can be read in place
    bool fz = false;          // has an FZ instance: a known-zero right-hand side is not loaded (7-point, not small)
    bool pre_noise = false;   // can draw the coarse level's first pre-sweep's Box-Muller pairs (27-point, not small)
    bool tail_noise = false;  // the small kernel, whose spare workgroups can draw a tail's noise
    bool vardiag = false;     // the VD instance: the centre coefficient from the level's diagonal vector (7-point, not small)
};

static_assert(mgmc::tune::ZR_SMALL_NX >= 8, "coarse levels below 8 cells per row take the gather kernel");

// cnx, cny, cnz: cells per direction of the coarser level
inline ResidualPlan plan_residual(const LevelShape& sh, uint32_t paths, int cnx, int cny, int cnz) {
    ResidualPlan p;
    if (!sh.has_coarser) return p;
    p.npoints = sh.npoints;
    p.sym = sh.fold;
    if (vardiag_eligible(sh, paths) && !(paths & PATH_NO_ZRESTRICT)) {
        // the 7-point tile rule below; never the one-wavefront instance (64-wide tiles take any level) and no
        // LRF / FZ instances
        p.kind = ResidualKind::ZMARCH;
        p.vardiag = true;
        p.cx = 64, p.cy = 4, p.nt = 256;
        const long long wide_tiles = (long long)((cnx + 62) / 64) * ((cny + 6) / 8) * (cnz - 1);
        if (wide_tiles >= mgmc::tune::ZR7_WIDE_MIN_TILES) p.cy = 8, p.nt = 512;
        return p;
    }
    if (sh.field) {
        p.kind = ResidualKind::FIELD;
        return p;
    }
    // z-marching kernel on every 3D level with coarse n >= 8: 64 x 4 coarse points per workgroup from
    // coarse n = ZR_SMALL_NX up, 16 x 4 points (one wavefront) below, where the wide tiles would leave
    // most of the chip idle (the 27-point gather kernel took 24 us per launch on the 15^3 / 7^3 levels)
    if (sh.dim != 3 || (paths & PATH_NO_ZRESTRICT) || cnx < 8) {
        p.kind = ResidualKind::GATHER;
        return p;
    }
    p.kind = ResidualKind::ZMARCH;
    p.small = cnx < mgmc::tune::ZR_SMALL_NX;
    p.cx = 64, p.cy = 4, p.nt = 256;
    if (p.small) {
        p.cx = 16, p.nt = 64;
        p.tail_noise = true;
    } else if (sh.npoints == 7) {
        // 64 x 8 coarse points, 512 threads, 80 KB of LDS (2 workgroups per CU): half the y halo
        // of 64 x 4 (19 x planes rows per 16 fine rows instead of 11 per 8); 512^3 with kz 32:
        // 505-525 -> 488-502 us (interleaved A/B); at 256^3 too few tiles (73 against 66 us)
        const long long wide_tiles = (long long)((cnx + 62) / 64) * ((cny + 6) / 8) * (cnz - 1);
        if (wide_tiles >= mgmc::tune::ZR7_WIDE_MIN_TILES) p.cy = 8, p.nt = 512;
        p.lrf = p.fz = true;
    } else {
        // (fold levels: the SYM instances, whose residual is fold27's, in tiles of the tuned shape)
        if (sh.fold) p.cx = mgmc::tune::ZR27_CX, p.cy = mgmc::tune::ZR27_CY;
        p.pre_noise = true;
    }
    return p;
}

// ---- the whole-field energy x^T Q x, f^T x of level 0 (mgmc_energy.hpp) ----
struct EnergyPlan {
    bool zmarch = false;   // k_energy_z: the forward-neighbour z-march of a symmetric 7-point level
    bool vardiag = false;  // ... its VD instance (the diagonal streamed per vertex)
    bool field = false;    // the general kernel of a per-vertex-coefficient level (k_energy_field); neither:
                           // k_energy_general<dim, npoints>
};
// The z-march goes wherever level 0 runs the z-sweep (plan_sweep's conditions: symmetric 7-point stencil, rows of
// whole 64-vertex tiles, MGMC_DISABLE=zsweep leaves it to the general kernels); force_general: mgmc_energy's
// flag, the general kernel on a z-sweep level (how the two are compared).
inline EnergyPlan plan_energy(const LevelShape& sh, uint32_t paths, bool force_general) {
    EnergyPlan p;
    p.zmarch = !force_general && plan_sweep(sh, paths, 0, -1) == SweepKernel::ZSWEEP;
    p.vardiag = p.zmarch && sh.field;
    p.field = !p.zmarch && sh.field;
    return p;
}

// ---- the Rao-Blackwellised field statistics of level 0 (mgmc_fieldcond.hpp) ----
enum class FieldCondPath {
    FUSED = 1,     // k_fieldcond_z: stencil and Welford fold in one z-march
    TWO_PASS = 2,  // operator apply + k_fieldcond_c into the c buffer, then k_fieldstats on it
};
// The fused z-march goes where level 0 runs the z-sweep with a constant stencil (not the variable-diagonal
// instance), has no low-rank part and the handle one chain; force_two_pass: MGMC_FIELD_COND_TWO_PASS, the two-pass
// path on such a level (how the two are compared).
inline FieldCondPath plan_fieldcond(const LevelShape& sh, uint32_t paths, int nchains, bool lowrank,
                                    bool force_two_pass) {
    const bool fused = plan_sweep(sh, paths, 0, -1) == SweepKernel::ZSWEEP && !sh.field && !lowrank && nchains == 1 &&
                       !force_two_pass;
    return fused ? FieldCondPath::FUSED : FieldCondPath::TWO_PASS;
}

// ---- the coarsest levels' sub-cycle in one workgroup (k_tail) ----
// (tail_start below; without a run_ops argument it plans for the default cycle)
constexpr size_t TAIL_LDS_LIMIT = 150 * 1024;

// 3D plane stride padded to sp = 8 (mod 16) doubles: k_tail's colour passes give the two halves of a
// half-wave the planes k and k+2, whose ds_read_b64 bank pairs (d mod 32) then sit 16 apart, so the
// stride-2 class access is 2-way (the least a stride-2 access allows) instead of 4-way with sx odd
// and unpadded planes (MI355X_MICROARCH.md LDS banking)
inline long long tail_plane_stride(int nx, int ny) {
    const long long sp = (long long)(nx + 1) * (ny + 1);
    return sp + ((8 - sp % 16) + 16) % 16;
}
// doubles of one level vector in k_tail's LDS layout (tail_layout(L).nstore)
inline size_t tail_level_doubles(int dim, int nx, int ny, int nz) {
    return dim == 3 ? (size_t)tail_plane_stride(nx, ny) * (nz + 1) : (size_t)(nx + 1) * (ny + 1);
}

// k_tail's argument block (TailArgs, mgmc_tail.hpp) holds this many levels and this many ops; tail_start keeps
// every tail within both
constexpr int TAIL_MAX_LEVELS = 4;
constexpr int TAIL_MAX_OPS = 96;

// The ops of one run of the tail: one call of build_ops_level (mgmc_capi.hip) on the first of ntail >= 1 levels
// that end at the coarsest, which is always a level > 0 and so repeats its body `cycle` times.  Per visit of a
// level that has a coarser one: k sweeps per smoothing step (k = 2 with the SSOR smoother: forward, backward),
// the residual + restriction, the coarser level's run, the prolongation (an op of its own on the tail's in-place
// levels); the coarsest level is coarsest_ops ops (1: the coarse SSOR sampler in one op; otherwise its sweeps).
//   run(coarsest) = coarsest_ops,  run(l) = cycle (k npre + 1 + run(l + 1) + 1 + k npost)
// 4 levels: SOR 1/1 V-cycle 13, W-cycle 64, cycle = 3 183; SSOR 1/1 W-cycle 92, SSOR 2/1 W-cycle 120.
// Exact up to 2^40 and saturated there (the counts grow like cycle^ntail).
inline long long tail_run_ops(int ntail, int cycle, int npre, int npost, bool ssor, int coarsest_ops = 1) {
    const long long cap = 1LL << 40;
    const long long k = ssor ? 2 : 1;
    long long run = std::max(coarsest_ops, 0);
    for (int l = 1; l < ntail; ++l) {
        const long long visit = k * std::max(npre, 0) + 2 + run + k * std::max(npost, 0);
        run = std::min(cap, std::min<long long>(std::max(cycle, 1), 1 << 20) * visit);
    }
    return run;
}
inline bool tail_run_fits(long long run_ops) { return run_ops <= TAIL_MAX_OPS; }

// smallest level lt >= 1 whose levels lt .. nlevels-1
//  * are at most TAIL_MAX_LEVELS,
//  * make a run of at most TAIL_MAX_OPS ops (run_ops(ntail): the ops of a run of ntail levels, tail_run_ops), and
//  * all fit one workgroup's LDS (x, f per level + one scratch of the largest + what else a level keeps there);
// -1 if none or only the coarsest level is left (the coarse LDS kernel covers that).  A hierarchy that is too
// deep or a cycle that is too long for one launch starts its tail later: a run of the levels from a later start
// is a whole call of build_ops_level too, entered and left at its first level with nothing live below.
// level_size(l, &v, &extra): whether the tail can run level l, the doubles v of one of its vectors and the
// doubles it keeps besides x and f
template <class LevelSize, class RunOps>
int tail_start(int nlevels, uint32_t paths, LevelSize level_size, RunOps run_ops) {
    if (paths & PATH_NO_TAIL) return -1;
    for (int lt = std::max(1, nlevels - TAIL_MAX_LEVELS); lt + 1 < nlevels; ++lt) {
        if (!tail_run_fits(run_ops(nlevels - lt))) continue;
        bool ok = true;
        size_t tot = 0, vmax = 0;
        for (int l = lt; l < nlevels && ok; ++l) {
            size_t v = 0, extra = 0;
            ok = level_size(l, &v, &extra);
            tot += 2 * v + extra;
            vmax = std::max(vmax, v);
        }
        if (ok && (tot + vmax) * sizeof(double) <= TAIL_LDS_LIMIT) return lt;
    }
    return -1;
}
// ... for the default cycle (V-cycle, one SOR pre- and post-sweep: a run of n levels is 4 n - 3 ops, 13 at most)
template <class LevelSize>
int tail_start(int nlevels, uint32_t paths, LevelSize level_size) {
    return tail_start(nlevels, paths, level_size, [](int ntail) { return tail_run_ops(ntail, 1, 1, 1, false); });
}

}  // namespace mgmc_host
