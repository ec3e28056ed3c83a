// socp_norm.hip — SOCP_F_NORMALISE (include/socp.h): the
// power-of-two scaling of c and of (b, h), and the exact scaling / unscaling
// of P and the iterates that goes with it.
//
// The rule.  Per problem nc = max |c_j| and nb = max(max |b_i|, max |h_i|);
// a norm v that is finite and positive gives the exponent -ilogb(v), clamped
// to +-256, every other norm (zero, or an Inf or a NaN anywhere in the vector)
// gives 0.  The max is taken on IEEE bit patterns, whose order as unsigned
// integers is the order of the non-negative values (socp_equil.hip), so it is
// the same in any order of the reduction; an Inf or a NaN is carried in a flag
// of its own beside the max.  The only floating-point operation is ldexp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "socp_norm.hpp"

namespace socp {
namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / 64;  // problems per workgroup of the norm kernel: one wavefront each
constexpr int TPB2 = 1024;     // the batch stage's one workgroup
constexpr int CHUNK = 1024;    // elements of a row that a wavefront scales at a time
constexpr uint64_t INF_BITS = 0x7ff0000000000000ull;
constexpr uint64_t BAD_BITS = ~0ull;  // the pattern stored for a vector with an Inf or a NaN

__device__ __forceinline__ uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }

// e(v) of a norm given by its bit pattern
__device__ __forceinline__ int expo_of(uint64_t u) {
  if (u == 0 || u >= INF_BITS) return 0;
  const int be = (int)(u >> 52);
  // ilogb: normal numbers from the exponent field; a subnormal is u * 2^-1074
  const int il = be ? be - 1023 : -1011 - __clzll((long long)u);
  const int e = -il;
  return e < -NORM_CLAMP ? -NORM_CLAMP : (e > NORM_CLAMP ? NORM_CLAMP : e);
}

// one lane's share of a vector: the max of the patterns, and whether one was no finite number
__device__ __forceinline__ void scan(const double* v, int len, int lane, uint64_t& mx, int& bad) {
  for (int i = lane; i < len; i += 64) {
    const uint64_t u = (uint64_t)__double_as_longlong(fabs(v[i]));
    bad |= u >= INF_BITS;
    mx = umax(mx, u);
  }
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) v = umax(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
  return v;
}

__global__ void __launch_bounds__(TPB) socp_norm_kernel(NormArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (p >= a.B) return;  // (whole wavefronts leave: the shuffles below see full ones)
  uint64_t mc = 0, mb = 0;
  int badc = 0, badb = 0;
  scan(a.c + p * a.n, a.n, lane, mc, badc);
  if (a.b) scan(a.b + p * a.m, a.m, lane, mb, badb);
  scan(a.h + p * a.k, a.k, lane, mb, badb);
  mc = __any(badc) ? BAD_BITS : wave_max(mc);
  mb = __any(badb) ? BAD_BITS : wave_max(mb);
  if (lane == 0) {
    if (a.nrm) {
      a.nrm[2 * p] = mc;
      a.nrm[2 * p + 1] = mb;
    } else {
      a.expo[2 * p] = expo_of(mc);
      a.expo[2 * p + 1] = expo_of(mb);
    }
  }
}

// the shared-P batch: the maxima of the problems' norms, and their pair for every problem
__global__ void __launch_bounds__(TPB2) socp_norm_batch_kernel(const unsigned long long* nrm, int32_t* expo, int64_t B) {
  __shared__ unsigned long long part[2][TPB2 / 64];
  const int tid = threadIdx.x;
  uint64_t mc = 0, mb = 0;
  for (int64_t p = tid; p < B; p += TPB2) {
    mc = umax(mc, nrm[2 * p]);
    mb = umax(mb, nrm[2 * p + 1]);
  }
  mc = wave_max(mc);
  mb = wave_max(mb);
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = mc;
    part[1][tid >> 6] = mb;
  }
  __syncthreads();
  mc = mb = 0;
  for (int w = 0; w < TPB2 / 64; ++w) {
    mc = umax(mc, part[0][w]);
    mb = umax(mb, part[1][w]);
  }
  const int ec = expo_of(mc), eb = expo_of(mb);
  for (int64_t p = tid; p < B; p += TPB2) {
    expo[2 * p] = ec;
    expo[2 * p + 1] = eb;
  }
}

// A segment is cut into units of one row's CHUNK consecutive elements; a wavefront takes a unit at a
// time, so the row's exponent is formed once per unit and the one division is the unit's, not an element's.
template <int SIGN>
__device__ __forceinline__ void scale_body(const NormScaleArgs& a) {
  const NormSeg s = a.seg[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const uint64_t len = (uint64_t)s.len, cpr = (len + CHUNK - 1) / CHUNK;  // chunks per row
  const uint64_t units = (uint64_t)s.rows * cpr;
  const uint64_t nw = (uint64_t)gridDim.x * WPB;
  for (uint64_t u = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6); u < units; u += nw) {
    const uint64_t r = cpr == 1 ? u : u / cpr;
    const uint64_t lo = (u - r * cpr) * CHUNK, hi = lo + CHUNK < len ? lo + CHUNK : len;
    const int e = SIGN * (s.sc * a.expo[2 * r] + s.sb * a.expo[2 * r + 1]);
    const double* src = s.src + r * len;
    double* dst = s.dst + r * len;
    for (uint64_t i = lo + lane; i < hi; i += 64) dst[i] = ldexp(src[i], e);
  }
}

__global__ void __launch_bounds__(TPB) socp_norm_forward_kernel(NormScaleArgs a) { scale_body<1>(a); }
__global__ void __launch_bounds__(TPB) socp_norm_backward_kernel(NormScaleArgs a) { scale_body<-1>(a); }

template <class K>
hipError_t scale_launch(K kern, const NormScaleArgs& a, hipStream_t stream) {
  int64_t most = 0;  // units of the largest segment
  for (int s = 0; s < a.nseg; ++s) {
    const int64_t units = a.seg[s].rows * ((a.seg[s].len + CHUNK - 1) / CHUNK);
    if (units > most) most = units;
  }
  if (a.nseg <= 0 || most == 0) return hipSuccess;
  int64_t blocks = (most + WPB - 1) / WPB;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)a.nseg), dim3(TPB), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t norm_launch(const NormArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(socp_norm_kernel, dim3((unsigned)((a.B + WPB - 1) / WPB)), dim3(TPB), 0, stream, a);
  return hipGetLastError();
}

hipError_t norm_batch_launch(const unsigned long long* nrm, int32_t* expo, int64_t B, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(socp_norm_batch_kernel, dim3(1), dim3(TPB2), 0, stream, nrm, expo, B);
  return hipGetLastError();
}

hipError_t norm_forward_launch(const NormScaleArgs& a, hipStream_t stream) {
  return scale_launch(socp_norm_forward_kernel, a, stream);
}
hipError_t norm_backward_launch(const NormScaleArgs& a, hipStream_t stream) {
  return scale_launch(socp_norm_backward_kernel, a, stream);
}

}  // namespace socp
