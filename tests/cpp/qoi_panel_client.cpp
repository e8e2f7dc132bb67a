// C++ client of the QoI-panel methods of include/mgmc_sampler.hh, compiled by tests/test_qoi_panel_host.py (g++,
// -Wall -Werror, also with AddressSanitizer + UBSan on the client).  Modes:
//   qoi_panel_client link          host only: the nine C entry points link and refuse a null handle
//   qoi_panel_client record N      a 2D 32 x 24 3-level sampler, a panel of two columns (one vertex, a dense
//                                  constant column), N recorded cycles; prints the series, the moments and S
// On a host without a GPU `record` prints the library's error and exits with -1 (reference convention).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mgmc_sampler.hh"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "link")) {
        int K = -1, nlags = -1;
        double d = 0.0;
        const int64_t colptr[2] = {0, 1}, rows[1] = {0};
        const double vals[1] = {1.0};
        int bad = 0;
        bad += mgmc_qoi_panel_set(nullptr, 1, colptr, rows, vals) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_eval(nullptr, &d) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_record_enable(nullptr, 1, 32, 16) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_record_disable(nullptr) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_record_reset(nullptr) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_info(nullptr, &K, nullptr, nullptr, nullptr, nullptr, nullptr) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_get_series(nullptr, 0, &d, 1) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_moments(nullptr, 0, &d, &d, &d) == MGMC_E_INVALID;
        bad += mgmc_qoi_panel_autocov(nullptr, 0, &d, &nlags) == MGMC_E_INVALID;
        std::printf("abi %d refused %d\n", mgmc_abi_version(), bad);
        return bad == 9 ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "record")) {
        const int nsteps = argc > 2 ? std::atoi(argv[2]) : 4;
        mgmc::MultigridParameters p;
        p.nlevel = 3;
        const mgmc_config c = mgmc::make_config(2, 32, 24, 0, 25.0, p);
        mgmc::HipMultigridMCSampler s(c, 0, 5418513ull, 0);
        const int64_t N = 31 * 23;
        std::vector<int64_t> colptr = {0, 1, 1 + N}, rows = {11 * 31 + 15};
        std::vector<double> vals = {1.0};
        for (int64_t e = 0; e < N; ++e) {
            rows.push_back(e);
            vals.push_back(1.0 / (32.0 * 24.0));
        }
        s.set_qoi_panel(2, colptr.data(), rows.data(), vals.data());
        const int window = 4;
        s.qoi_panel_record(1, window, 64);
        s.sample(nsteps, -1);
        const size_t n = (size_t)s.qoi_panel_recorded();
        const int K = s.qoi_panel_size();
        std::vector<double> z(n * K), mean(K), C((size_t)K * K), S((size_t)K * window);
        double cnt = 0.0;
        s.qoi_panel_series(0, z.data(), n);
        s.qoi_panel_moments(0, &cnt, mean.data(), C.data());
        const int nlags = s.qoi_panel_autocovariance(0, S.data());
        const std::vector<double> now = s.qoi_panel_eval();
        std::printf("records %zu K %d count %.17g nlags %d\n", n, K, cnt, nlags);
        for (size_t r = 0; r < n; ++r) std::printf("z %.17g %.17g\n", z[r * K], z[r * K + 1]);
        std::printf("now %.17g %.17g\n", now[0], now[1]);
        std::printf("mean %.17g %.17g\nC %.17g %.17g %.17g %.17g\n", mean[0], mean[1], C[0], C[1], C[2], C[3]);
        s.reset_qoi_panel();
        s.qoi_panel_off();
        s.set_qoi_panel(0, nullptr, nullptr, nullptr);
        std::printf("after K %d\n", s.qoi_panel_size());
        return 0;
    }
    return 2;
}
