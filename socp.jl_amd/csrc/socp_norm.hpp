// socp_norm.hpp — SOCP_F_NORMALISE (include/socp.h): the
// arguments and host launchers of the three kernels in socp_norm.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace socp {

constexpr int NORM_CLAMP = 256;  // ec and eb stay in [-256, 256]

// The max-norms of c and of (b, h) per problem and their exponents:
// expo[2p] = ec, expo[2p+1] = eb.  b may be NULL (m = 0).  With `nrm` given
// the kernel writes the two norms' bit patterns there instead (B x 2; all ones
// for a vector that holds an Inf or a NaN) and norm_batch_launch turns them
// into one pair for the whole batch.
struct NormArgs {
  const double* c;  // B x n
  const double* b;  // B x m or NULL
  const double* h;  // B x k
  int32_t* expo;    // B x 2
  unsigned long long* nrm;  // B x 2 or NULL
  int64_t B;
  int32_t n, m, k;
};

// dst[r*len + i] = ldexp(src[r*len + i], sign * (sc * expo[2r] + sb * expo[2r+1])),
// r < rows; sign is +1 in the forward and -1 in the backward kernel.  dst may
// be src.
struct NormSeg {
  double* dst;
  const double* src;
  int64_t len;
  int64_t rows;
  int32_t sc, sb;
};
struct NormScaleArgs {
  NormSeg seg[8];
  const int32_t* expo;
  int32_t nseg;
};

hipError_t norm_launch(const NormArgs& a, hipStream_t stream);
// the second stage of the shared-P batch: the maxima of nrm over the batch, one pair in all 2B entries of expo
hipError_t norm_batch_launch(const unsigned long long* nrm, int32_t* expo, int64_t B, hipStream_t stream);
hipError_t norm_forward_launch(const NormScaleArgs& a, hipStream_t stream);
hipError_t norm_backward_launch(const NormScaleArgs& a, hipStream_t stream);

}  // namespace socp
