// mgmc_rhs_zero.hpp -- when the cycle takes level 0's right-hand side as the constant +0.0 (host logic, no HIP:
// tests/cpp/rhs_zero_host.cpp compiles it alone).
//
// Prior sampling has f = A 0 = 0 on level 0 (the reference fixes it once, Sampler::fix_rhs).  mgmc_create
// zeroes f; mgmc_set_rhs -- the only writer of level 0's f, mgmc_apply included -- takes the bit-pattern OR
// of the uploaded vector (k_or_bits, mgmc_kernels.hpp; rhs_or_bits below is its host statement) and keeps
// mgmc_handle::f0_zero.  While it holds, the cycle's ops on level 0 that run the z-marching sweep / the
// 7-point z-marching residual + restriction run their FZ instances (mgmc_zsweep.hpp, mgmc_zrestrict.hpp),
// which do not load f: 8 B per unknown less per pass, the same bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mgmc_host {

// all-bits-zero: +0.0 only.  -0.0 (sign bit), denormals and NaN have bits set and count as non-zero.
inline bool rhs_bits_all_zero(uint64_t or_bits) { return or_bits == 0; }

inline uint64_t rhs_or_bits(const double* v, size_t n) {
    uint64_t acc = 0;
    for (size_t q = 0; q < n; ++q) {
        uint64_t b;
        std::memcpy(&b, v + q, sizeof(b));
        acc |= b;
    }
    return acc;
}

// what the choice depends on, for one op of the cycle
struct RhsZeroOp {
    int level;         // the op's level
    bool zsweep;       // the level runs k_zsweep_rb7 (Level::sweep)
    int lr_m;          // low-rank columns of the level (a posterior level patches f: never zero)
    bool residual_fz;  // the level's residual + restriction has an FZ instance (ResidualPlan::fz, mgmc_level_plan.hpp:
                       // the 7-point z-marching kernel, not the small 16 x 4 one -- a z-sweep level has nx >= 64, so
                       // its coarse level has nx >= 32 and never is small -- and not the gather kernel)
    int zpre;          // Op::zpre of a residual + restriction (its spare workgroups draw a tail's noise: small kernel)
};

inline bool rhs_zero_sweep_ok(bool f0_zero, const RhsZeroOp& o) {
    return f0_zero && o.level == 0 && o.zsweep && o.lr_m == 0;
}

inline bool rhs_zero_residual_ok(bool f0_zero, const RhsZeroOp& o) {
    return f0_zero && o.level == 0 && o.zsweep && o.lr_m == 0 && o.residual_fz && o.zpre == 0;
}

}  // namespace mgmc_host
