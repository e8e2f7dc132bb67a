// mgmc_fieldcond_host.hpp -- the conditional precision d_i = Q_ii of the Rao-Blackwellised field statistics
// (mgmc_fieldcond.hpp), built on the host (no HIP: tests/cpp/fieldcond_plan_host.cpp compiles it alone).
//
// Q = A + B Sigma^{-1} B^T with B in CSC form (column k: rows[colptr[k] .. colptr[k + 1]), ascending, and their
// values) and Sigma diagonal.  Per vertex i
//     d_i = a_ii;   for k = 0 .. m - 1 ascending, where B_ik is stored:   d_i = d_i + (B_ik * B_ik) / Sigma_k
// in plain IEEE double.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mgmc_host {

// d: on entry the diagonal of A (n values, the reference's vertex order), on return d
inline void fieldcond_precision(double* d, size_t n, int m, const int64_t* colptr, const int64_t* rows,
                                const double* vals, const double* sigma) {
    for (int k = 0; k < m; ++k)  // (column by column: every vertex meets its columns in ascending k)
        for (int64_t q = colptr[k]; q < colptr[k + 1]; ++q) {
            const size_t i = (size_t)rows[q];
            if (i >= n) continue;
            d[i] = d[i] + (vals[q] * vals[q]) / sigma[k];  // (product -> quotient -> sum: nothing to contract)
        }
}

}  // namespace mgmc_host
