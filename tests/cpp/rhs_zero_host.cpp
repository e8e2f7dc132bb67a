// Host logic of the zero-right-hand-side path (multigridmc_amd/csrc/mgmc_rhs_zero.hpp), compiled alone by
// tests/test_rhs_zero_host.py (g++, AddressSanitizer + UBSan): what counts as a zero right-hand side and which
// ops of the cycle may take it as a constant.  Prints one "ok <name>" line per check; exits 1 on a failure.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "mgmc_level_plan.hpp"
#include "mgmc_rhs_zero.hpp"

using namespace mgmc_host;

// ResidualPlan::fz of a 3D FD level of npoints points onto a coarse level of coarse_nx^3 cells (mgmc_level_plan.hpp)
static bool residual_fz(int npoints, bool zrestrict, int coarse_nx) {
    const LevelShape fine{3, npoints, 2 * coarse_nx, 2 * coarse_nx, 2 * coarse_nx, false, true, false, true};
    return plan_residual(fine, zrestrict ? 0 : PATH_NO_ZRESTRICT, coarse_nx, coarse_nx, coarse_nx).fz;
}

static int failures = 0;
static void check(bool ok, const char* name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) ++failures;
}

int main() {
    // ---- detection: the OR of the bit patterns ----
    const size_t n = 1000;
    std::vector<double> f(n, 0.0);
    check(rhs_bits_all_zero(rhs_or_bits(f.data(), n)), "zeros");
    check(rhs_bits_all_zero(rhs_or_bits(f.data(), 0)), "empty");
    struct Case {
        const char* name;
        double value;
    };
    const Case cases[] = {{"minus_zero", -0.0},
                          {"denormal", std::numeric_limits<double>::denorm_min()},
                          {"nan", std::numeric_limits<double>::quiet_NaN()},
                          {"inf", std::numeric_limits<double>::infinity()},
                          {"one", 1.0},
                          {"tiny_negative", -1e-300}};
    for (const Case& c : cases)
        for (size_t pos : {(size_t)0, n / 2 + 1, n - 1}) {
            std::vector<double> g(n, 0.0);
            g[pos] = c.value;
            check(!rhs_bits_all_zero(rhs_or_bits(g.data(), n)), c.name);
        }
    {  // values that cancel in a sum do not cancel in the OR
        std::vector<double> g(n, 0.0);
        g[3] = 1.5;
        g[4] = -1.5;
        check(!rhs_bits_all_zero(rhs_or_bits(g.data(), n)), "cancelling_pair");
    }

    // ---- selection ----
    // the 512^3 benchmark's level 0: z-sweep, 7-point, coarse nx 256
    const RhsZeroOp fine{0, true, 0, residual_fz(7, true, 256), 0};
    check(rhs_zero_sweep_ok(true, fine) && rhs_zero_residual_ok(true, fine), "fine_level_zero_f");
    check(!rhs_zero_sweep_ok(false, fine) && !rhs_zero_residual_ok(false, fine), "fine_level_nonzero_f");
    RhsZeroOp o = fine;
    o.level = 1;  // coarse levels: f is the restricted residual
    check(!rhs_zero_sweep_ok(true, o) && !rhs_zero_residual_ok(true, o), "coarse_level");
    o = fine;
    o.lr_m = 3;  // a posterior level patches f
    check(!rhs_zero_sweep_ok(true, o) && !rhs_zero_residual_ok(true, o), "lowrank_level");
    o = fine;
    o.zsweep = false;  // colour-pass kernels (MGMC_DISABLE=zsweep, nx % 64 != 0): general
    check(!rhs_zero_sweep_ok(true, o) && !rhs_zero_residual_ok(true, o), "no_zsweep");
    o = fine;
    // MGMC_DISABLE=zrestrict: the gather residual kernel has no zero instance; the sweeps keep theirs
    o.residual_fz = residual_fz(7, false, 256);
    check(rhs_zero_sweep_ok(true, o) && !rhs_zero_residual_ok(true, o), "no_zrestrict");
    o = fine;
    o.residual_fz = residual_fz(27, true, 256);
    check(!rhs_zero_residual_ok(true, o), "residual_27_point");
    o = fine;
    o.residual_fz = residual_fz(7, true, 16);  // the small 16 x 4 residual kernel
    check(!rhs_zero_residual_ok(true, o), "small_residual_kernel");
    o = fine;
    o.residual_fz = residual_fz(7, true, 32);  // the smallest z-sweep level (nx 64): the 64 x 4 kernel
    check(rhs_zero_residual_ok(true, o), "nx64_level");
    o = fine;
    o.zpre = 1;  // its spare workgroups draw a tail's noise: general
    check(rhs_zero_sweep_ok(true, o) && !rhs_zero_residual_ok(true, o), "residual_draws_tail_noise");
    return failures ? 1 : 0;
}
