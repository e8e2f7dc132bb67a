// The host-side level plan (multigridmc_amd/csrc/mgmc_level_plan.hpp), compiled alone by
// tests/test_level_plan_host.py (g++, AddressSanitizer + UBSan): which sweep and which residual + restriction
// kernel each level of a hierarchy gets, and where k_tail starts.  The expected plans are the labels the merged
// GPU tests assert for the same shapes (named at each block), not values taken from the header.  Prints one
// "ok <name>" line per check; exits 1 on a failure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mgmc_level_plan.hpp"

using namespace mgmc_host;
using SK = SweepKernel;
using RK = ResidualKind;

static int failures = 0;
static void check(bool ok, const std::string& name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
    if (!ok) ++failures;
}

struct Hier {
    std::vector<LevelShape> sh;
    std::vector<SK> sweep;
    std::vector<ResidualPlan> res;
    int tail = -1;
};

// The hierarchy of an n[0] x n[1] x n[2] lattice by halving, as mgmc_create builds it: the FD prior's fine level
// has the symmetric 5 / 7-point stencil and Galerkin levels of 9 / 27 points whose 3D stencils are
// reflection-symmetric (fold); the FEM prior has 9 / 27 points on every level, not symmetric bit for bit.
// the cycle's shape, which bounds the tail by the ops of its run (tail_run_ops); the default is the V-cycle with
// one SOR pre- and post-sweep
struct Cycle {
    int cycle = 1, npre = 1, npost = 1;
    bool ssor = false;
};
// matrix: a matrix handle (mgmc_create_csr) whose fine matrix is a constant symmetric 7-point stencil plus a diagonal
// field: every level a field level, the fine one variable-diagonal, no tail
static Hier walk(int dim, int nx, int ny, int nz, int nlevel, bool fem, uint32_t paths, Cycle cy = Cycle(),
                 bool matrix = false) {
    Hier H;
    for (int l = 0; l < nlevel; ++l) {
        const bool galerkin = fem || l > 0;
        LevelShape s;
        s.dim = dim;
        s.npoints = dim == 3 ? (galerkin ? 27 : 7) : (galerkin ? 9 : 5);
        s.nx = nx >> l;
        s.ny = ny >> l;
        s.nz = dim == 3 ? nz >> l : 0;
        s.field = matrix;
        s.vardiag = matrix && l == 0;
        s.fd_symmetric = !fem;
        s.fold = dim == 3 && !fem && !matrix && l > 0 && !(paths & PATH_NO_FOLD);
        s.has_coarser = l + 1 < nlevel;
        H.sh.push_back(s);
    }
    H.tail = tail_start(
        nlevel, paths,
        [&](int l, size_t* v, size_t*) {
            const LevelShape& s = H.sh[l];
            *v = tail_level_doubles(s.dim, s.nx, s.ny, s.nz);
            return !s.field && s.npoints == (s.dim == 3 ? 27 : 9);
        },
        [&](int ntail) { return tail_run_ops(ntail, cy.cycle, cy.npre, cy.npost, cy.ssor); });
    for (int l = 0; l < nlevel; ++l) {
        H.sweep.push_back(plan_sweep(H.sh[l], paths, l, H.tail));
        H.res.push_back(l + 1 < nlevel ? plan_residual(H.sh[l], paths, H.sh[l + 1].nx, H.sh[l + 1].ny, H.sh[l + 1].nz)
                                       : ResidualPlan());
    }
    return H;
}

// the levels from lt on keep in-place sweeps, so k_tail can run them
static bool in_place_from(const Hier& H, int lt) {
    bool ok = true;
    for (size_t l = (size_t)lt; l < H.sweep.size(); ++l) ok = ok && !sweep_pingpong(H.sweep[l]);
    return ok;
}

static bool zmarch(const ResidualPlan& p, int np, int cx, int cy) {
    return p.kind == RK::ZMARCH && p.npoints == np && p.cx == cx && p.cy == cy;
}

// a 7-point level's plan onto a coarse level of cnx x cny x cnz cells
static ResidualPlan fine_res(int cnx, int cny, int cnz, uint32_t paths = 0) {
    const LevelShape s{3, 7, 2 * cnx, 2 * cny, 2 * cnz, false, true, false, true};
    return plan_residual(s, paths, cnx, cny, cnz);
}

static uint32_t flag_of(const char* token) {
    setenv("MGMC_DISABLE", token, 1);
    uint32_t f = 0;
    std::string bad;
    const bool ok = read_path_flags(&f, &bad);
    unsetenv("MGMC_DISABLE");
    return ok ? f : 0;
}

// "plan" mode (tests/test_tuning_host.py, compiled against a re-tuned mgmc_tuning.hpp):
//   level_plan_host plan <nx> <ny> <nz> <nlevel> [MGMC_DISABLE list] [vardiag]   (nz = 0: a 2D lattice; FD prior)
// (vardiag: the matrix handle of the periodic-kappa^2 FD operator instead) prints one line per level,
//   level <l> sweep <KIND> [rows <z-sweep tile rows of the VD instance>] [lanes|window] [js <chunks per plane>x<steps per chunk>] residual <KIND> [np <n> cx <n> cy <n> nt <n>] [small] [sym] [vd] tail <lt>
static int print_plan(int argc, char** argv) {
    if (argc < 6) return 2;
    const int nx = atoi(argv[2]), ny = atoi(argv[3]), nz = atoi(argv[4]), nlevel = atoi(argv[5]);
    const uint32_t paths = argc > 6 && argv[6][0] ? flag_of(argv[6]) : 0;
    if (argc > 6 && argv[6][0] && !paths) return 2;
    const int dim = nz > 0 ? 3 : 2;
    const bool matrix = argc > 7 && std::string(argv[7]) == "vardiag";
    if (argc > 7 && !matrix) return 2;
    const Hier H = walk(dim, nx, ny, nz, nlevel, false, paths, Cycle(), matrix);
    static const char* const sk[] = {"COLOUR", "FIELD", "PAIRS", "QUADS", "JSWEEP", "RB2D", "ZSWEEP"};
    static const char* const rk[] = {"NONE", "FIELD", "GATHER", "ZMARCH"};
    for (int l = 0; l < nlevel; ++l) {
        const ResidualPlan& r = H.res[l];
        std::printf("level %d sweep %s", l, sk[(int)H.sweep[l]]);
        // (the VD instance of the z-sweep takes the fused-prolongation sweep's tile rows: launch_zsweep)
        if (H.sweep[l] == SK::ZSWEEP && H.sh[l].vardiag) std::printf(" rows %d", mgmc::tune::ZS_TYP);
        if (H.sweep[l] == SK::QUADS && dim == 3) std::printf(" %s", quads_lanes(dim, H.sh[l].nx / 2) ? "lanes" : "window");
        if (H.sweep[l] == SK::JSWEEP) {  // forward sweep, first half, the 256 compute units of an MI355X
            const JSweepPlan p = jsweep_plan_dims(H.sh[l].ny, H.sh[l].nz, true, 0, 256, jsweep_lds_bytes(H.sh[l].nx / 2),
                                                  mgmc::tune::JS_ROUNDS);
            std::printf(" js %dx%d", p.nchunk, p.spc);
        }
        std::printf(" residual %s", rk[(int)r.kind]);
        if (r.kind == RK::ZMARCH) std::printf(" np %d cx %d cy %d nt %d", r.npoints, r.cx, r.cy, r.nt);
        if (r.small) std::printf(" small");
        if (r.sym) std::printf(" sym");
        if (r.vardiag) std::printf(" vd");
        std::printf(" tail %d\n", H.tail);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "plan") return print_plan(argc, argv);
    {  // 512^3, 7 levels: tests/test_gpu_headline.py test_headline_kernel_instances
        const Hier H = walk(3, 512, 512, 512, 7, false, 0);
        check(H.sweep[0] == SK::ZSWEEP, "headline_l0_zsweep");
        const ResidualPlan& r0 = H.res[0];
        check(zmarch(r0, 7, 64, 8) && r0.nt == 512 && !r0.small && !r0.sym, "headline_l0_residual_7_64_8");
        check(r0.fz && r0.lrf && !r0.pre_noise && !r0.tail_noise, "headline_l0_residual_fz_lrf");
        check(H.sweep[1] == SK::JSWEEP && H.sh[1].nx / 2 == 128, "headline_l1_jsweep_128");
        const ResidualPlan& r1 = H.res[1];
        check(zmarch(r1, 27, 64, 4) && r1.nt == 256 && r1.sym && !r1.small, "headline_l1_residual_27_64_4_sym");
        check(r1.pre_noise && !r1.fz && !r1.lrf && !r1.tail_noise, "headline_l1_residual_pre_noise");
        check(H.sweep[2] == SK::QUADS && quads_lanes(3, H.sh[2].nx / 2), "headline_l2_quads_lanes");
        check(H.sweep[3] == SK::QUADS && H.sweep[4] == SK::QUADS, "headline_l3_l4_quads");
        check(H.tail == 5 && in_place_from(H, 5), "headline_tail_from_5");
        check(H.res[4].small && H.res[4].tail_noise, "headline_restriction_before_tail_small");
        check(H.res[6].kind == RK::NONE, "headline_coarsest_no_residual");
    }
    {  // 256^3, 6 levels: tests/test_gpu_config3.py (2 * 16 * 127 = 4,064 wide tiles: 64 x 4)
        const Hier H = walk(3, 256, 256, 256, 6, false, 0);
        check(H.sweep[0] == SK::ZSWEEP && zmarch(H.res[0], 7, 64, 4) && H.res[0].nt == 256 && H.res[0].fz,
              "config3_l0_residual_7_64_4");
        check(H.sweep[1] == SK::QUADS && zmarch(H.res[1], 27, 64, 4) && H.res[1].pre_noise, "config3_l1_quads");
        check(H.sweep[2] == SK::QUADS && H.sweep[3] == SK::QUADS && H.tail == 4 && in_place_from(H, 4),
              "config3_quads_then_tail");
    }
    {  // 24 x 20 x 12: tests/test_gpu_parity.py ROW_LENGTH_LABELS
        const Hier H = walk(3, 24, 20, 12, 3, false, 0);
        const ResidualPlan& r0 = H.res[0];
        check(H.sweep[0] == SK::COLOUR, "24x20x12_l0_colour");
        check(zmarch(r0, 7, 16, 4) && r0.nt == 64 && r0.small && r0.tail_noise && !r0.fz && !r0.lrf && !r0.pre_noise,
              "24x20x12_l0_residual_7_16_4_small");
        check(H.tail == 1 && in_place_from(H, 1), "24x20x12_tail_from_1");
    }
    {  // 96^3, 5 levels: ROW_LENGTH_LABELS
        const Hier H = walk(3, 96, 96, 96, 5, false, 0);
        check(H.sweep[0] == SK::COLOUR, "96_l0_colour");  // nx % 64 != 0
        check(zmarch(H.res[0], 7, 64, 4) && !H.res[0].small, "96_l0_residual_7_64_4");
        check(H.sweep[1] == SK::QUADS && !quads_lanes(3, H.sh[1].nx / 2), "96_l1_quads_window");
        check(H.sweep[2] == SK::QUADS && !quads_lanes(3, H.sh[2].nx / 2), "96_l2_quads_window");
        check(H.tail == 3 && in_place_from(H, 3), "96_tail_from_3");
    }
    {  // 320 x 24 x 16: ROW_LENGTH_LABELS (80-pair rows: pair passes)
        const Hier H = walk(3, 320, 24, 16, 3, false, 0);
        check(H.sweep[0] == SK::ZSWEEP, "320_l0_zsweep");
        check(H.sweep[1] == SK::PAIRS && H.sh[1].nx / 2 == 80, "320_l1_pairs_80");
        check(zmarch(H.res[1], 27, 64, 4) && H.res[1].sym && H.res[1].pre_noise, "320_l1_residual_27_64_4");
    }
    {  // 2D 200 x 120, 4 levels and 2D 100 x 60: ROW_LENGTH_LABELS, test_qrestrict_labels (k_residual_restrict<2,5>)
        const Hier H = walk(2, 200, 120, 0, 4, false, 0);
        check(H.sweep[0] == SK::RB2D, "200x120_l0_rb2d");
        check(H.res[0].kind == RK::GATHER && H.res[0].npoints == 5 && H.res[0].cx == 0, "200x120_l0_gather_2_5");
        check(H.sweep[1] == SK::QUADS && H.res[1].kind == RK::GATHER, "200x120_l1_quads");  // (k_quads_restrict2d)
        check(H.tail == 2 && in_place_from(H, 2), "200x120_tail_from_2");
        const Hier G = walk(2, 100, 60, 0, 3, false, 0);
        check(G.sweep[0] == SK::RB2D && G.res[0].kind == RK::GATHER && G.res[0].npoints == 5, "100x60_l0_rb2d_gather");
        check(G.tail == 1 && in_place_from(G, 1), "100x60_tail_from_1");
    }
    {  // FEM 512^3: tests/test_gpu_fem.py (k_jsweep_half<256>, k_jsweep_half<128>: no sym instance)
        const Hier H = walk(3, 512, 512, 512, 7, true, 0);
        check(H.sweep[0] == SK::JSWEEP && H.sh[0].nx / 2 == 256 && !H.res[0].sym, "fem_l0_jsweep_256_not_sym");
        check(H.sweep[1] == SK::JSWEEP && H.sh[1].nx / 2 == 128, "fem_l1_jsweep_128");
        check(zmarch(H.res[0], 27, 64, 4) && H.res[0].pre_noise, "fem_l0_residual_27_64_4");
    }

    // ---- boundaries ----
    check(fine_res(7, 7, 7).kind == RK::GATHER && fine_res(7, 7, 7).cx == 0, "coarse_nx_7_gather");
    check(zmarch(fine_res(8, 8, 8), 7, 16, 4) && fine_res(8, 8, 8).small, "coarse_nx_8_small");
    check(zmarch(fine_res(31, 32, 32), 7, 16, 4) && fine_res(31, 32, 32).small && !fine_res(31, 32, 32).fz,
          "coarse_nx_31_small");
    check(zmarch(fine_res(32, 32, 32), 7, 64, 4) && !fine_res(32, 32, 32).small && fine_res(32, 32, 32).fz,
          "coarse_nx_32_wide_tiles");
    // 64 x 8 tiles of the coarse level: 4 * 32 * 255 = 32,640 at 512^3; 4 * 32 * 128 = 16,384 is the threshold
    check(zmarch(fine_res(256, 256, 129), 7, 64, 8) && fine_res(256, 256, 129).nt == 512, "wide_tiles_at_threshold");
    check(zmarch(fine_res(256, 256, 128), 7, 64, 4) && fine_res(256, 256, 128).nt == 256, "wide_tiles_below_threshold");

    // ---- MGMC_DISABLE tokens: each moves the plan to the fallback its PathFlag names ----
    {
        const uint32_t zs = flag_of("zsweep"), pa = flag_of("pairs"), qu = flag_of("quads"), js = flag_of("jsweep"),
                       rb = flag_of("rb2d"), zr = flag_of("zrestrict"), ta = flag_of("tail");
        check(zs && pa && qu && js && rb && zr && ta && flag_of("no_such_path") == 0, "tokens_parse");
        const Hier Z = walk(3, 512, 512, 512, 7, false, zs);
        check(Z.sweep[0] == SK::COLOUR && Z.sweep[1] == SK::JSWEEP && zmarch(Z.res[0], 7, 64, 8), "token_zsweep");
        const Hier P = walk(3, 512, 512, 512, 7, false, pa);
        bool colour = P.sweep[0] == SK::ZSWEEP;
        for (int l = 1; l < 7; ++l) colour = colour && P.sweep[l] == SK::COLOUR;
        check(colour, "token_pairs");
        const Hier Q = walk(3, 512, 512, 512, 7, false, qu);
        check(Q.sweep[1] == SK::JSWEEP && Q.sweep[2] == SK::PAIRS && Q.sweep[3] == SK::PAIRS && Q.sweep[4] == SK::PAIRS,
              "token_quads");
        const Hier J = walk(3, 512, 512, 512, 7, false, js);
        check(J.sweep[1] == SK::PAIRS && J.sweep[2] == SK::QUADS, "token_jsweep");  // 128-pair rows: no quads
        const Hier R = walk(2, 200, 120, 0, 4, false, rb);
        check(R.sweep[0] == SK::COLOUR && R.sweep[1] == SK::QUADS, "token_rb2d");
        const Hier G = walk(3, 512, 512, 512, 7, false, zr);
        bool gather = true;
        for (int l = 0; l < 6; ++l)
            gather = gather && G.res[l].kind == RK::GATHER && G.res[l].cx == 0 && !G.res[l].fz && !G.res[l].lrf &&
                     !G.res[l].pre_noise && !G.res[l].tail_noise;
        check(gather && G.res[1].sym && G.sweep[0] == SK::ZSWEEP, "token_zrestrict");
        const Hier T = walk(3, 512, 512, 512, 7, false, ta);
        check(T.tail == -1 && T.sweep[5] == SK::QUADS && T.sweep[6] == SK::QUADS, "token_tail");
    }

    // ---- the tail's limits: TailArgs (mgmc_tail.hpp) holds 4 levels and 96 ops ----
    check(TAIL_MAX_LEVELS == 4 && TAIL_MAX_OPS == 96, "tail_limits_4_levels_96_ops");
    {  // deep hierarchies.  By LDS size alone the 2D tails below would start at level 1, 1, 1, 2 and 4 and hold 5, 5,
       // 6, 6 and 5 levels; in 3D the LDS limit (16^3 is the largest level that fits) stops at 4 on its own
        struct Deep {
            const char* name;
            int dim, nx, ny, nz, nlevel, tail;
        };
        const Deep deep[] = {{"2d64_6lvl", 2, 64, 64, 0, 6, 2},         {"2d96x64_6lvl", 2, 96, 64, 0, 6, 2},
                             {"2d128_7lvl", 2, 128, 128, 0, 7, 3},      {"2d256_8lvl", 2, 256, 256, 0, 8, 4},
                             {"2d1024_9lvl", 2, 1024, 1024, 0, 9, 5},   {"3d32_5lvl", 3, 32, 32, 32, 5, 1},
                             {"3d64_6lvl", 3, 64, 64, 64, 6, 2},        {"3d512_9lvl", 3, 512, 512, 512, 9, 5}};
        for (const Deep& d : deep) {
            const Hier H = walk(d.dim, d.nx, d.ny, d.nz, d.nlevel, false, 0);
            check(H.tail >= 1 && d.nlevel - H.tail <= 4, std::string(d.name) + "_tail_at_most_4_levels");
            check(H.tail == d.tail && in_place_from(H, H.tail), std::string(d.name) + "_tail_start_in_place");
            bool before = true;  // ... and the Galerkin levels before it are not left to it
            for (int l = 1; l < H.tail; ++l) before = before && H.sweep[l] != SK::PAIRS;
            check(before, std::string(d.name) + "_levels_before_tail_not_pairs");
        }
    }
    {  // without a cycle shape tail_start plans for the default cycle: the same depth bound
        const Hier H = walk(2, 64, 64, 0, 6, false, 0);
        const int t = tail_start(6, 0, [&](int l, size_t* v, size_t*) {
            *v = tail_level_doubles(2, H.sh[l].nx, H.sh[l].ny, 0);
            return H.sh[l].npoints == 9;
        });
        check(t == 2 && t == H.tail, "tail_start_default_cycle");
    }
    {  // the ops of one run: cycle (k npre + 1 + run(l + 1) + 1 + k npost), k = 2 with SSOR, the coarsest level 1
        check(tail_run_ops(1, 3, 1, 1, false) == 1 && tail_run_ops(2, 1, 1, 1, false) == 5 &&
                  tail_run_ops(4, 1, 1, 1, false) == 13 && tail_run_ops(4, 2, 1, 1, false) == 64,
              "run_ops_sor_v_and_w");
        check(tail_run_ops(4, 3, 1, 1, false) == 183 && !tail_run_fits(tail_run_ops(4, 3, 1, 1, false)),
              "run_ops_sor_cycle3_183_too_long");
        check(tail_run_ops(4, 2, 2, 1, true) == 120 && !tail_run_fits(tail_run_ops(4, 2, 2, 1, true)),
              "run_ops_ssor_2_1_w_120_too_long");
        check(tail_run_ops(4, 2, 1, 1, true) == 92 && tail_run_fits(tail_run_ops(4, 2, 1, 1, true)),
              "run_ops_ssor_1_1_w_92_fits");
        check(tail_run_ops(3, 3, 1, 1, false) == 57 && tail_run_ops(3, 2, 2, 1, true) == 52, "run_ops_3_levels");
        check(tail_run_ops(3, 1, 0, 0, false) == 5 && tail_run_ops(2, 1, 0, 2, true, 4) == 10, "run_ops_zero_sweeps");
        check(tail_run_fits(96) && !tail_run_fits(97), "run_fits_at_96");
        check(tail_run_ops(4, 1 << 30, 1 << 30, 1 << 30, true) > 96 && tail_run_ops(24, 1000, 9, 9, true) > 96,
              "run_ops_saturates_without_overflow");
    }
    {  // a run too long for one launch: the tail starts a level later, where a whole run fits (183 -> 57, 120 -> 52),
       // and the level it leaves takes the quad passes; 92 ops stay in one launch from level 1
        const Hier A = walk(3, 32, 32, 32, 5, false, 0, Cycle{3, 1, 1, false});
        check(A.tail == 2 && in_place_from(A, 2) && A.sweep[1] == SK::QUADS, "3d32_cycle3_tail_from_2");
        const Hier B = walk(2, 64, 64, 0, 5, false, 0, Cycle{3, 1, 1, false});
        check(B.tail == 2 && in_place_from(B, 2) && B.sweep[1] == SK::QUADS, "2d64_cycle3_tail_from_2");
        const Hier C = walk(3, 32, 32, 32, 5, false, 0, Cycle{2, 2, 1, true});
        check(C.tail == 2 && in_place_from(C, 2) && C.sweep[1] == SK::QUADS, "3d32_ssor_2_1_w_tail_from_2");
        const Hier D = walk(3, 32, 32, 32, 5, false, 0, Cycle{2, 1, 1, true});
        check(D.tail == 1 && in_place_from(D, 1) && D.sweep[1] == SK::PAIRS, "3d32_ssor_1_1_w_tail_from_1");
        // no two levels' run fits (100 + 2 + 1 + 1 ops): no tail, every level on its own kernels
        const Hier E = walk(3, 32, 32, 32, 5, false, 0, Cycle{1, 100, 1, false});
        check(E.tail == -1 && E.sweep[3] == SK::QUADS, "3d32_100_presweeps_no_tail");
        const Hier F = walk(3, 32, 32, 32, 5, false, 0, Cycle{1, 0, 0, false});
        check(F.tail == 1 && in_place_from(F, 1), "3d32_no_sweeps_tail_from_1");
    }
    return failures ? 1 : 0;
}
