// plan_fieldcond (multigridmc_amd/csrc/mgmc_level_plan.hpp) and the host-only builder of the conditional
// precision d (mgmc_fieldcond_host.hpp), compiled alone by tests/test_field_cond_host.py (g++, AddressSanitizer +
// UBSan).  The fused z-march goes exactly where level 0 runs the z-sweep with a constant stencil, no low-rank part
// and one chain; everything else takes the two passes.
// Prints one "ok <name>" line per plan check.  With a file argument (text: n m, then n diagonal values, m + 1
// column pointers, the rows, the values and m Sigma values; floating-point numbers as C99 hex) it also prints
// "d <i> <hex>" for every vertex.  Exits 1 on a failure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mgmc_fieldcond_host.hpp"
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

static bool read_double(FILE* in, double* v) {
    char tok[64];
    if (std::fscanf(in, "%63s", tok) != 1) return false;
    char* end = nullptr;
    *v = std::strtod(tok, &end);
    return end != tok && *end == 0;
}

static int print_d(const char* path) {
    FILE* in = std::fopen(path, "r");
    if (!in) return 1;
    long long n = 0, m = 0;
    bool ok = std::fscanf(in, "%lld %lld", &n, &m) == 2 && n > 0 && m >= 0;
    std::vector<double> d, vals, sigma;
    std::vector<int64_t> colptr, rows;
    if (ok) {
        d.resize((size_t)n);
        for (double& v : d) ok = ok && read_double(in, &v);
        colptr.resize((size_t)m + 1);
        for (int64_t& c : colptr) {
            long long t = 0;
            ok = ok && std::fscanf(in, "%lld", &t) == 1;
            c = t;
        }
        ok = ok && colptr[0] == 0 && colptr[(size_t)m] >= 0;
    }
    if (ok) {
        rows.resize((size_t)colptr[(size_t)m]);
        vals.resize(rows.size());
        sigma.resize((size_t)m);
        for (int64_t& r : rows) {
            long long t = 0;
            ok = ok && std::fscanf(in, "%lld", &t) == 1 && t >= 0 && t < n;
            r = t;
        }
        for (double& v : vals) ok = ok && read_double(in, &v);
        for (double& v : sigma) ok = ok && read_double(in, &v);
    }
    std::fclose(in);
    if (!ok) return 1;
    fieldcond_precision(d.data(), d.size(), (int)m, colptr.data(), rows.data(), vals.data(), sigma.data());
    for (size_t i = 0; i < d.size(); ++i) std::printf("d %zu %a\n", i, d[i]);
    return 0;
}

int main(int argc, char** argv) {
    const LevelShape z = fine(3, 7, 64, 22, 10, false, true, false);
    const auto F = FieldCondPath::FUSED, T = FieldCondPath::TWO_PASS;
    check(plan_fieldcond(z, 0, 1, false, false) == F, "fused_64x22x10");
    check(plan_fieldcond(z, 0, 3, false, false) == T, "two_pass_three_chains");
    check(plan_fieldcond(z, 0, 1, true, false) == T, "two_pass_lowrank");
    check(plan_fieldcond(z, 0, 1, false, true) == T, "two_pass_forced");
    check(plan_fieldcond(z, PATH_NO_ZSWEEP, 1, false, false) == T, "two_pass_disable_zsweep");
    // a variable-diagonal level runs the z-sweep, but d is a field
    const LevelShape vd = fine(3, 7, 128, 34, 18, true, true, true);
    check(plan_sweep(vd, 0, 0, -1) == SweepKernel::ZSWEEP, "vardiag_runs_the_zsweep");
    check(plan_fieldcond(vd, 0, 1, false, false) == T, "two_pass_vardiag");
    // rows that are no whole 64-vertex tiles, 2D, FEM (27 points), the squared operator's field level
    check(plan_fieldcond(fine(3, 7, 24, 20, 12, false, true, false), 0, 1, false, false) == T, "two_pass_24x20x12");
    check(plan_fieldcond(fine(2, 5, 48, 40, 0, false, true, false), 0, 1, false, false) == T, "two_pass_2d_48x40");
    check(plan_fieldcond(fine(3, 27, 16, 16, 16, false, false, false), 0, 1, false, false) == T, "two_pass_fem_16");
    check(plan_fieldcond(fine(2, 13, 32, 32, 0, true, false, false), 0, 1, false, false) == T, "two_pass_2d_squared");
    // the fused path follows plan_sweep: a one-level hierarchy and an unsymmetric stencil have no z-sweep
    LevelShape one = z;
    one.has_coarser = false;
    check(plan_fieldcond(one, 0, 1, false, false) == T, "two_pass_one_level");
    LevelShape asym = z;
    asym.fd_symmetric = false;
    check(plan_fieldcond(asym, 0, 1, false, false) == T, "two_pass_unsymmetric_stencil");
    check(plan_fieldcond(fine(3, 7, 128, 34, 18, false, true, false), 0, 1, false, false) == F, "fused_128x34x18");
    // the d builder: no columns leave the diagonal alone; a vertex meets its columns in ascending k
    {
        double d[3] = {4.0, 5.0, 6.0};
        const int64_t none[1] = {0};
        fieldcond_precision(d, 3, 0, none, nullptr, nullptr, nullptr);
        check(d[0] == 4.0 && d[1] == 5.0 && d[2] == 6.0, "d_without_lowrank");
        const int64_t colptr[3] = {0, 2, 3}, rows[3] = {0, 2, 2};
        const double vals[3] = {0.1, 0.3, 0.7}, sigma[2] = {0.5, 0.25};
        fieldcond_precision(d, 3, 2, colptr, rows, vals, sigma);
        check(d[0] == 4.0 + (0.1 * 0.1) / 0.5 && d[1] == 5.0 && d[2] == (6.0 + (0.3 * 0.3) / 0.5) + (0.7 * 0.7) / 0.25,
              "d_two_columns");
    }
    if (argc > 1 && print_d(argv[1]) != 0) {
        std::printf("FAIL reading %s\n", argv[1]);
        ++failures;
    }
    return failures ? 1 : 0;
}
