// socp_equil.hpp — SOCP_F_EQUILIBRATE (include/socp.h): the
// arguments and host launchers of the two scaling kernels in socp_equil.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "socp_small.hpp"  // ConeTable, MAXC, POC_K, SOC_K

namespace socp {

constexpr int EQUIL_CLAMP = 256;     // every exponent stays in [-256, 256]
constexpr int EQUIL_MAX_PASSES = 64;  // socp_ctx_set_equilibration_passes' upper bound
constexpr int EQUIL_EF_LDS = 4096;   // F's exponents live in LDS up to this k, in `ex` above it
constexpr size_t EQUIL_LDS_BUDGET = 64 * 1024;

// One workgroup per matrix set.  Matrices are column-major (include/socp.h);
// A and P may be NULL (m = 0, no quadratic term).  Every output may be NULL
// and may be its input (in-place scaling of a staged copy).
struct EquilArgs {
  const double* A;  // MB x (m x n)
  const double* G;  // MB x (k x n)
  const double* P;  // MB x (n x n) or NULL
  double* As;
  double* Gs;
  double* Ps;
  double* D;        // MB x n, 2^ed
  double* E;        // MB x m, 2^ee
  double* F;        // MB x k, 2^ef
  int32_t* ex;      // MB x (n + m + k): ed, ee, ef of every set (always written)
  int32_t n, m, k, nc;
  int32_t passes;
  int32_t ef_lds;   // set by equil_launch: ef in LDS
  int32_t cache;    // set by equil_launch: bit 0 G, bit 1 A, bit 2 P are kept in LDS across the passes
  ConeTable cones;
};

// dst[p*len + i] = ldexp(src[p*len + i], sign * ex[p*exstride + i]), p < B
struct EquilVecSeg {
  double* dst;
  const double* src;
  const int32_t* ex;
  int32_t len;
  int32_t sign;
};
struct EquilVecArgs {
  EquilVecSeg seg[4];
  int64_t B;
  int64_t exstride;  // n + m + k, or 0 with one factor set for the batch
  int32_t nseg;
};

hipError_t equil_launch(EquilArgs a, int64_t MB, hipStream_t stream);
hipError_t equil_vec_launch(const EquilVecArgs& a, hipStream_t stream);

}  // namespace socp
