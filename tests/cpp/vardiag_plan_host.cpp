// The level plan of a variable-diagonal fine level (multigridmc_amd/csrc/mgmc_level_plan.hpp), compiled alone by
// tests/test_vardiag_host.py (g++, AddressSanitizer + UBSan): a field level whose matrix is a constant symmetric
// 7-point stencil plus a diagonal field takes the z-marching sweep and residual + restriction, every other field
// level keeps the field kernels.  Prints one "ok <name>" line per check; exits 1 on a failure.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mgmc_level_plan.hpp"

using namespace mgmc_host;
using SK = SweepKernel;
using RK = ResidualKind;

static int failures = 0;
static void check(bool ok, const std::string& name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
    if (!ok) ++failures;
}

static uint32_t flag_of(const char* token) {
    setenv("MGMC_DISABLE", token, 1);
    uint32_t f = 0;
    std::string bad;
    const bool ok = read_path_flags(&f, &bad);
    unsetenv("MGMC_DISABLE");
    return ok ? f : 0;
}

// the fine level of a matrix handle on nx x ny x nz cells
static LevelShape field_level(int dim, int np, int nx, int ny, int nz, bool has_coarser, bool vardiag) {
    LevelShape s{dim, np, nx, ny, nz, true, true, false, has_coarser};
    s.vardiag = vardiag;
    return s;
}
static ResidualPlan res_of(const LevelShape& s, uint32_t paths) {
    return plan_residual(s, paths, s.nx / 2, s.ny / 2, s.nz / 2);
}
static bool field_plan(const LevelShape& s, uint32_t paths) {
    const ResidualPlan r = res_of(s, paths);
    return plan_sweep(s, paths, 0, -1) == SK::FIELD && r.kind == (s.has_coarser ? RK::FIELD : RK::NONE) && !r.vardiag;
}

int main() {
    // the trailing member defaults to false: the nine-member initialisation of the other host tests
    const LevelShape nine{3, 7, 128, 34, 18, true, true, false, true};
    check(!nine.vardiag, "default_false");

    const uint32_t zsweep = flag_of("zsweep"), zrestrict = flag_of("zrestrict");
    check(zsweep == PATH_NO_ZSWEEP && zrestrict == PATH_NO_ZRESTRICT, "tokens");

    // the GPU cases' fine levels: 64 x 22 x 10, 128 x 34 x 18, 192 x 48 x 40
    const int shapes[3][3] = {{64, 22, 10}, {128, 34, 18}, {192, 48, 40}};
    for (const auto& n : shapes) {
        const LevelShape s = field_level(3, 7, n[0], n[1], n[2], true, true);
        const std::string tag = std::to_string(n[0]);
        const ResidualPlan r = res_of(s, 0);
        check(plan_sweep(s, 0, 0, -1) == SK::ZSWEEP, "sweep_zsweep_" + tag);
        check(r.kind == RK::ZMARCH && r.vardiag && r.npoints == 7 && r.cx == 64 && r.cy == 4 && r.nt == 256 &&
                  !r.small && !r.lrf && !r.fz && !r.tail_noise && !r.pre_noise && !r.sym,
              "residual_zmarch_" + tag);
        // MGMC_DISABLE=zsweep: the field kernels for both; zrestrict: the sweep stays, the residual is FIELD
        check(field_plan(s, zsweep), "disable_zsweep_" + tag);
        const ResidualPlan rz = res_of(s, zrestrict);
        check(plan_sweep(s, zrestrict, 0, -1) == SK::ZSWEEP && rz.kind == RK::FIELD && !rz.vardiag,
              "disable_zrestrict_" + tag);
        // the same level without the recognition plans exactly as a field level did
        check(field_plan(field_level(3, 7, n[0], n[1], n[2], true, false), 0), "not_recognised_" + tag);
    }
    // the wide 64 x 8 tiles from ZR7_WIDE_MIN_TILES 64 x 8 tiles up, as on a constant 7-point level
    {
        const LevelShape s = field_level(3, 7, 512, 512, 512, true, true);
        const ResidualPlan r = res_of(s, 0);
        const long long wide = 4LL * 32 * 255;
        check(r.kind == RK::ZMARCH && r.vardiag && r.cx == 64 && !r.lrf && !r.fz &&
                  (wide >= mgmc::tune::ZR7_WIDE_MIN_TILES ? r.cy == 8 && r.nt == 512 : r.cy == 4 && r.nt == 256),
              "wide_tiles_512");
    }
    // shapes the z-sweep does not take stay FIELD: nx = 96, 2D, 27 points, no coarser level, an asymmetric stencil
    check(field_plan(field_level(3, 7, 96, 34, 18, true, true), 0), "nx_96");
    check(field_plan(field_level(2, 5, 128, 34, 0, true, true), 0), "dim_2");
    check(field_plan(field_level(3, 27, 128, 34, 18, true, true), 0), "npoints_27");
    check(field_plan(field_level(3, 7, 128, 34, 18, false, true), 0), "no_coarser");
    {
        LevelShape s = field_level(3, 7, 128, 34, 18, true, true);
        s.fd_symmetric = false;
        check(field_plan(s, 0), "not_symmetric");
    }
    // a constant-stencil level plans as before
    {
        const LevelShape s{3, 7, 128, 34, 18, false, true, false, true};
        const ResidualPlan r = res_of(s, 0);
        check(plan_sweep(s, 0, 0, -1) == SK::ZSWEEP && r.kind == RK::ZMARCH && !r.vardiag && r.lrf && r.fz,
              "constant_level_unchanged");
    }
    return failures ? 1 : 0;
}
