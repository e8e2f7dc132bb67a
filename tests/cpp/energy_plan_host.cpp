// plan_energy (multigridmc_amd/csrc/mgmc_level_plan.hpp), compiled alone by tests/test_energy_host.py (g++,
// AddressSanitizer + UBSan): which kernel reduces x^T Q x on level 0.  The z-march goes exactly where the level
// plan picks SweepKernel::ZSWEEP; everything else takes a general kernel (the stencil's or the field's).
// Prints one "ok <name>" line per check; exits 1 on a failure.
#include <cstdio>
#include <string>

#include "mgmc_level_plan.hpp"

using namespace mgmc_host;

static int failures = 0;
static void check(bool ok, const std::string& name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
    if (!ok) ++failures;
}

// level 0 of a hierarchy with a coarser level
static LevelShape fine(int dim, int npoints, int nx, int ny, int nz, bool field, bool symmetric, bool vardiag) {
    LevelShape s;
    s.dim = dim;
    s.npoints = npoints;
    s.nx = nx, s.ny = ny, s.nz = nz;
    s.field = field;
    s.fd_symmetric = symmetric;
    s.fold = false;
    s.has_coarser = true;
    s.vardiag = vardiag;
    return s;
}

static bool is(const EnergyPlan& p, bool zmarch, bool vardiag, bool field) {
    return p.zmarch == zmarch && p.vardiag == vardiag && p.field == field;
}

int main() {
    const LevelShape z = fine(3, 7, 64, 22, 10, false, true, false);
    const LevelShape vd = fine(3, 7, 128, 34, 18, true, true, true);
    check(is(plan_energy(z, 0, false), true, false, false), "zmarch_64x22x10");
    check(is(plan_energy(vd, 0, false), true, true, false), "zmarch_vardiag_128x34x18");
    // the flag of mgmc_energy, and MGMC_DISABLE=zsweep: the general kernels on the same levels
    check(is(plan_energy(z, 0, true), false, false, false), "forced_general_64x22x10");
    check(is(plan_energy(vd, 0, true), false, false, true), "forced_general_vardiag_is_field");
    check(is(plan_energy(z, PATH_NO_ZSWEEP, false), false, false, false), "disable_zsweep_64x22x10");
    check(is(plan_energy(vd, PATH_NO_ZSWEEP, false), false, false, true), "disable_zsweep_vardiag");
    // the plan follows plan_sweep
    check((plan_sweep(z, 0, 0, -1) == SweepKernel::ZSWEEP) == plan_energy(z, 0, false).zmarch, "follows_plan_sweep");
    // rows that are no whole 64-vertex tiles, 2D, FEM (27 points), field levels, a one-level hierarchy
    check(is(plan_energy(fine(3, 7, 24, 20, 12, false, true, false), 0, false), false, false, false), "general_24x20x12");
    check(is(plan_energy(fine(2, 5, 48, 40, 0, false, true, false), 0, false), false, false, false), "general_2d_48x40");
    check(is(plan_energy(fine(2, 5, 64, 64, 0, false, true, false), 0, false), false, false, false), "general_2d_64x64");
    check(is(plan_energy(fine(3, 27, 64, 64, 64, false, false, false), 0, false), false, false, false), "general_fem_64");
    check(is(plan_energy(fine(3, 7, 32, 16, 16, true, true, true), 0, false), false, false, true), "field_periodic_32x16x16");
    check(is(plan_energy(fine(2, 13, 32, 32, 0, true, false, false), 0, false), false, false, true), "field_2d_squared");
    check(is(plan_energy(fine(3, 7, 64, 22, 10, true, true, false), 0, false), false, false, true), "field_not_vardiag_64x22x10");
    LevelShape one = z;
    one.has_coarser = false;
    check(is(plan_energy(one, 0, false), false, false, false), "general_one_level");
    LevelShape asym = z;
    asym.fd_symmetric = false;
    check(is(plan_energy(asym, 0, false), false, false, false), "general_unsymmetric_stencil");
    return failures ? 1 : 0;
}
