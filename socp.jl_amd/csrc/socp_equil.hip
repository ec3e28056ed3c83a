// socp_equil.hip — SOCP_F_EQUILIBRATE (include/socp.h): Ruiz
// equilibration of a batch with power-of-two factors, and the exact scaling /
// unscaling of the vectors.
//
// The rule.  Integer exponents ed[n], ee[m], ef[k] start at 0 (D = 2^ed,
// E = 2^ee, F = 2^ef).  Each pass takes the max-norms of the scaled
// magnitudes ldexp(|A_ij|, ee_i + ed_j), ldexp(|G_ij|, ef_i + ed_j) and
// ldexp(|P_ij|, ed_i + ed_j): per column over A, G and P, per row of A, per
// row of G; the rows of one SOC cone share the cone's largest row norm (one
// factor per cone keeps F s in K <=> s in K).  A norm v that is finite and
// positive adds t = -floor((ilogb(v) + 1) / 2) to its exponent (clamped to
// +-256); zero, Inf and NaN norms add nothing.  All exponents of a pass are
// updated from that pass's norms.
//
// Everything is integer arithmetic on IEEE bit patterns: for non-negative
// doubles the order of the values is the order of their bit patterns as
// unsigned integers, Inf is 0x7ff0... and every NaN lies above it.  So the max
// of the patterns is the NaN-propagating max of the values, it is the same
// whatever the order of the reduction, and "finite and positive" is
// 0 < pattern < Inf's.  The only floating-point operation is ldexp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "socp_equil.hpp"

namespace socp {
namespace {

constexpr int TPB = 256;
constexpr uint64_t INF_BITS = 0x7ff0000000000000ull;

// bit pattern of ldexp(|a|, e)
__device__ __forceinline__ uint64_t mag(double a, int e) {
  return (uint64_t)__double_as_longlong(ldexp(fabs(a), e));
}

// the exponent increment of a norm given by its bit pattern
__device__ __forceinline__ int incr(uint64_t u) {
  if (u == 0 || u >= INF_BITS) return 0;
  const int be = (int)(u >> 52);
  // ilogb: normal numbers from the exponent field; a subnormal is u * 2^-1074
  const int il = be ? be - 1023 : -1011 - __clzll((long long)u);
  return -((il + 1) >> 1);  // arithmetic shift: floor
}

__device__ __forceinline__ int clampe(int e) {
  return e < -EQUIL_CLAMP ? -EQUIL_CLAMP : (e > EQUIL_CLAMP ? EQUIL_CLAMP : e);
}

__device__ __forceinline__ uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }

// cone of row i (the table is contiguous from row 0)
__device__ __forceinline__ int cone_of(const int32_t* coffs, const int32_t* cdim, int nc, int i) {
  int c = 0;
  while (c + 1 < nc && i >= coffs[c] + cdim[c]) ++c;
  return c;
}

__device__ __forceinline__ void copy_in(double* dst, const double* src, int64_t cnt, int tid) {
  for (int64_t t = tid; t < cnt; t += TPB) dst[t] = src[t];
}

__global__ void __launch_bounds__(TPB) socp_equil_kernel(EquilArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = a.n, m = a.m, k = a.k, nc = a.nc;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t p = blockIdx.x;
  const int64_t S = (int64_t)n + m + k;

  // LDS: 8-byte items first (cn, cmax, the cached matrices), then the int32 tables
  unsigned long long* cn = (unsigned long long*)smem;  // column norms [n]
  unsigned long long* cmax = cn + n;                    // per-cone max of the row norms [MAXC]
  double* cache = (double*)(cmax + MAXC);
  const double* G = a.G + p * (int64_t)k * n;
  const double* A = (m > 0 && a.A) ? a.A + p * (int64_t)m * n : nullptr;
  const double* P = a.P ? a.P + p * (int64_t)n * n : nullptr;
  int64_t off = 0;
  bool all_lds = (a.cache & 1) != 0;
  if (a.cache & 1) {
    copy_in(cache + off, G, (int64_t)k * n, tid);
    G = cache + off;
    off += (int64_t)k * n;
  }
  if (A) {
    if (a.cache & 2) {
      copy_in(cache + off, A, (int64_t)m * n, tid);
      A = cache + off;
      off += (int64_t)m * n;
    } else {
      all_lds = false;
    }
  }
  if (P) {
    if (a.cache & 4) {
      copy_in(cache + off, P, (int64_t)n * n, tid);
      P = cache + off;
      off += (int64_t)n * n;
    } else {
      all_lds = false;
    }
  }
  int32_t* ed = (int32_t*)(cache + off);  // [n]
  int32_t* ee = ed + n;                   // [m]
  int32_t* coffs = ee + m;                // [MAXC]
  int32_t* cdim = coffs + MAXC;           // [MAXC]
  int32_t* ckind = cdim + MAXC;           // [MAXC]
  int32_t* chg = ckind + MAXC;            // [EQUIL_MAX_PASSES]: a pass changed an exponent
  int32_t* exg = a.ex + p * S;            // this set's exponents in global memory
  int32_t* ef = a.ef_lds ? chg + EQUIL_MAX_PASSES : exg + n + m;  // [k]

  for (int j = tid; j < n; j += TPB) ed[j] = 0;
  for (int i = tid; i < m; i += TPB) ee[i] = 0;
  for (int i = tid; i < k; i += TPB) ef[i] = 0;
  if (tid < MAXC) {
    coffs[tid] = tid < nc ? a.cones.offs[tid] : 0;
    cdim[tid] = tid < nc ? a.cones.dim[tid] : 0;
    ckind[tid] = tid < nc ? a.cones.kind[tid] : POC_K;
  }
  if (tid < EQUIL_MAX_PASSES) chg[tid] = 0;
  __syncthreads();
  // the first SOC row (POC cones come first): the cone sweep starts there
  int soc0 = k;
  for (int c = 0; c < nc; ++c)
    if (ckind[c] == SOC_K) {
      soc0 = coffs[c];
      break;
    }
  // the rows of G, A and P as one index space, a lane per row
  const int ma = A ? m : 0, R = k + ma + (P ? n : 0);

  for (int pass = 0; pass < a.passes; ++pass) {
    for (int j = tid; j < n; j += TPB) cn[j] = 0;
    if (tid < MAXC) cmax[tid] = 0;
    __syncthreads();
    // A lane walks its row over the columns, keeping the row's max in-lane; every element goes by
    // an LDS atomic max into its column's slot (an integer max: the same bits in any order).  With
    // the matrices in LDS the lanes of a wave start at different columns, so that neither the
    // reads (k or m even: the lanes' addresses are an odd number of doubles apart) nor the
    // atomics meet on one address; from global memory the lanes stay on one column, so that the
    // reads are coalesced.  A row's own exponent is read and written by its lane only, so ee and
    // the POC part of ef are updated in place; ed and the SOC part wait for the barrier.
    for (int r = tid; r < R; r += TPB) {
      const double* q;
      int64_t rows;
      int er;
      if (r < k) {
        q = G + r;
        rows = k;
        er = ef[r];
      } else if (r < k + ma) {
        q = A + (r - k);
        rows = m;
        er = ee[r - k];
      } else {
        q = P + (r - k - ma);
        rows = n;
        er = ed[r - k - ma];
      }
      uint64_t rm = 0;
      int jj = all_lds ? lane % n : 0;
      for (int j = 0; j < n; ++j) {
        const uint64_t v = mag(q[(int64_t)jj * rows], er + ed[jj]);
        rm = umax(rm, v);
        if (v) atomicMax(&cn[jj], (unsigned long long)v);
        if (++jj == n) jj = 0;
      }
      if (r < k) {
        const int c = cone_of(coffs, cdim, nc, r);
        if (ckind[c] == SOC_K) {
          atomicMax(&cmax[c], (unsigned long long)rm);
        } else {
          const int ne = clampe(er + incr(rm));
          if (ne != er) ef[r] = ne, chg[pass] = 1;
        }
      } else if (r < k + ma) {
        const int ne = clampe(er + incr(rm));
        if (ne != er) ee[r - k] = ne, chg[pass] = 1;
      }
    }
    __syncthreads();
    for (int j = tid; j < n; j += TPB) {
      const int ne = clampe(ed[j] + incr(cn[j]));
      if (ne != ed[j]) ed[j] = ne, chg[pass] = 1;
    }
    for (int i = soc0 / TPB * TPB + tid; i < k; i += TPB)  // (row i stays with lane i mod TPB)
      if (i >= soc0) {
        const int ne = clampe(ef[i] + incr(cmax[cone_of(coffs, cdim, nc, i)]));
        if (ne != ef[i]) ef[i] = ne, chg[pass] = 1;
      }
    __syncthreads();
    // a pass that moved nothing is the fixed point: every later pass would see the same norms
    if (!chg[pass]) break;
  }

  // the factors, then the scaled matrices (a lane per row, as above; an
  // output may be its own input: every element is read and written by one lane)
  for (int j = tid; j < n; j += TPB) {
    exg[j] = ed[j];
    if (a.D) a.D[p * n + j] = ldexp(1.0, ed[j]);
  }
  for (int i = tid; i < m; i += TPB) {
    exg[n + i] = ee[i];
    if (a.E) a.E[p * m + i] = ldexp(1.0, ee[i]);
  }
  for (int i = tid; i < k; i += TPB) {
    if (a.ef_lds) exg[n + m + i] = ef[i];
    if (a.F) a.F[p * k + i] = ldexp(1.0, ef[i]);
  }
  if (a.As && A) {
    double* o = a.As + p * (int64_t)m * n;
    for (int i = tid; i < m; i += TPB) {
      const int er = ee[i];
      for (int j = 0; j < n; ++j) o[(int64_t)j * m + i] = ldexp(A[(int64_t)j * m + i], er + ed[j]);
    }
  }
  if (a.Gs) {
    double* o = a.Gs + p * (int64_t)k * n;
    for (int i = tid; i < k; i += TPB) {
      const int er = ef[i];
      for (int j = 0; j < n; ++j) o[(int64_t)j * k + i] = ldexp(G[(int64_t)j * k + i], er + ed[j]);
    }
  }
  if (a.Ps && P) {
    double* o = a.Ps + p * (int64_t)n * n;
    for (int i = tid; i < n; i += TPB) {
      const int er = ed[i];
      for (int j = 0; j < n; ++j) o[(int64_t)j * n + i] = ldexp(P[(int64_t)j * n + i], er + ed[j]);
    }
  }
}

__global__ void __launch_bounds__(TPB) socp_equil_vec_kernel(EquilVecArgs a) {
  const EquilVecSeg s = a.seg[blockIdx.y];
  const int64_t total = a.B * (int64_t)s.len;
  for (int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x; t < total; t += (int64_t)gridDim.x * TPB) {
    const int64_t p = t / s.len;
    const int64_t i = t - p * s.len;
    s.dst[t] = ldexp(s.src[t], s.sign * s.ex[p * a.exstride + i]);
  }
}

}  // namespace

hipError_t equil_launch(EquilArgs a, int64_t MB, hipStream_t stream) {
  if (MB <= 0) return hipSuccess;
  const int64_t n = a.n, m = a.m, k = a.k;
  // cn, cmax; ed, ee, the cone table, the passes' change flags
  size_t lds = 8 * (size_t)(n + MAXC) + 4 * (size_t)(n + m + 3 * MAXC + EQUIL_MAX_PASSES);
  a.ef_lds = k <= EQUIL_EF_LDS;
  if (a.ef_lds) lds += 4 * (size_t)k;
  lds = (lds + 15) & ~(size_t)15;
  // the matrices stay in LDS across the passes where they fit: G, then A, then P
  a.cache = 0;
  const size_t szG = 8 * (size_t)k * n, szA = (m > 0 && a.A) ? 8 * (size_t)m * n : 0, szP = a.P ? 8 * (size_t)n * n : 0;
  if (lds + szG <= EQUIL_LDS_BUDGET) {
    a.cache |= 1;
    lds += szG;
    if (szA && lds + szA <= EQUIL_LDS_BUDGET) {
      a.cache |= 2;
      lds += szA;
    }
    if (szP && lds + szP <= EQUIL_LDS_BUDGET) {
      a.cache |= 4;
      lds += szP;
    }
  }
  hipLaunchKernelGGL(socp_equil_kernel, dim3((unsigned)MB), dim3(TPB), lds, stream, a);
  return hipGetLastError();
}

hipError_t equil_vec_launch(const EquilVecArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.nseg <= 0) return hipSuccess;
  int64_t most = 0;
  for (int s = 0; s < a.nseg; ++s)
    if (a.B * a.seg[s].len > most) most = a.B * a.seg[s].len;
  if (most == 0) return hipSuccess;
  int64_t blocks = (most + TPB - 1) / TPB;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(socp_equil_vec_kernel, dim3((unsigned)blocks, (unsigned)a.nseg), dim3(TPB), 0, stream, a);
  return hipGetLastError();
}

}  // namespace socp
