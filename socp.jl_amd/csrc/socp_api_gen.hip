// socp_api_gen.hip — the API unit with device code: the problem generator
// (socp_generate), CSC packing (socp_pack_csc, and the ingest's launches of its
// kernel) and the kernels that pack the multi-GPU gather's records.
#include <cmath>

#include "socp_host.hpp"

using namespace socp;
using namespace socp::host;

// u = splitmix64(seed ^ (p<<24 | e)), U = (u>>11)*2^-53,
// p the GLOBAL problem index.  Sequential sums without FMA contraction so the
// CPU restatement (oracle/socp_oracle.c: or_generate) is bit-identical.
namespace {
struct GenArgs {
  int64_t B, first;
  uint64_t seed;
  int32_t n, m, k, nc;
  double *c, *A, *b, *G, *h;
  ConeTable cones;
};

// The generator must round exactly like the oracle (gcc -ffp-contract=off):
// hipcc contracts a*b+c into v_fma_f64 by default, and __dadd_rn/__dmul_rn are
// plain operators, so contraction is switched off for these functions (the
// build uses -ffp-contract=fast-honor-pragmas so the pragma is obeyed).
#pragma clang fp contract(off)
// local operators: the bodies of HIP's __dadd_rn/__dmul_rn lie outside this
// pragma and would still be fused
__device__ __forceinline__ double add_rn(double x, double y) { return x + y; }
__device__ __forceinline__ double sub_rn(double x, double y) { return x - y; }
__device__ __forceinline__ double mul_rn(double x, double y) { return x * y; }
__device__ __forceinline__ double sqrt_rn(double x) { return __builtin_sqrt(x); }

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ double gen_u(uint64_t seed, uint64_t p, uint64_t e) {
  uint64_t u = splitmix64(seed ^ ((p << 24) | e));
  return mul_rn((double)(u >> 11), 0x1.0p-53);
}
__device__ __forceinline__ double gen_sym(uint64_t seed, uint64_t p, uint64_t e) {
  return sub_rn(mul_rn(2.0, gen_u(seed, p, e)), 1.0);
}

__global__ void __launch_bounds__(256) socp_generate_kernel(GenArgs a) {
  extern __shared__ double sh[];
  const int64_t p = blockIdx.x;
  const uint64_t gp = (uint64_t)(a.first + p);
  const int n = a.n, m = a.m, k = a.k;
  double* x0 = sh;
  double* y0 = x0 + n;
  double* s0 = y0 + m;
  double* z0 = s0 + k;
  const uint64_t kn = (uint64_t)k * n, mn = (uint64_t)m * n;
  double* Gp = a.G + p * (int64_t)kn;
  double* Ap = a.A + p * (int64_t)mn;
  for (uint64_t e = threadIdx.x; e < kn; e += blockDim.x) Gp[e] = gen_sym(a.seed, gp, e);
  for (uint64_t e = threadIdx.x; e < mn; e += blockDim.x) Ap[e] = gen_sym(a.seed, gp, kn + e);
  const uint64_t base = kn + mn;
  for (int j = threadIdx.x; j < n; j += blockDim.x) x0[j] = gen_sym(a.seed, gp, base + j);
  for (int i = threadIdx.x; i < m; i += blockDim.x) y0[i] = gen_sym(a.seed, gp, base + n + i);
  const uint64_t base2 = base + n + m;
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    int c = 0;
    while (!(i >= a.cones.offs[c] && i < a.cones.offs[c] + a.cones.dim[c])) ++c;
    const int o = a.cones.offs[c], d = a.cones.dim[c];
    const uint64_t es = base2 + 2 * (uint64_t)o, ez = es + d;
    if (a.cones.kind[c] == POC_K) {
      s0[i] = add_rn(0.5, gen_u(a.seed, gp, es + (i - o)));
      z0[i] = add_rn(0.5, gen_u(a.seed, gp, ez + (i - o)));
    } else if (i > o) {
      s0[i] = gen_sym(a.seed, gp, es + (i - o - 1));
      z0[i] = gen_sym(a.seed, gp, ez + (i - o - 1));
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < a.nc; c += blockDim.x) {
    if (a.cones.kind[c] != SOC_K) continue;
    const int o = a.cones.offs[c], d = a.cones.dim[c];
    const uint64_t es = base2 + 2 * (uint64_t)o, ez = es + d;
    double qs = 0.0, qz = 0.0;
    for (int i = 1; i < d; ++i) {
      qs = add_rn(qs, mul_rn(s0[o + i], s0[o + i]));
      qz = add_rn(qz, mul_rn(z0[o + i], z0[o + i]));
    }
    s0[o] = add_rn(add_rn(sqrt_rn(qs), 0.5), gen_u(a.seed, gp, es + d - 1));
    z0[o] = add_rn(add_rn(sqrt_rn(qz), 0.5), gen_u(a.seed, gp, ez + d - 1));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j)
      acc = add_rn(acc, mul_rn(gen_sym(a.seed, gp, (uint64_t)j * k + i), x0[j]));
    a.h[p * k + i] = add_rn(acc, s0[i]);
  }
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j)
      acc = add_rn(acc, mul_rn(gen_sym(a.seed, gp, kn + (uint64_t)j * m + i), x0[j]));
    a.b[p * m + i] = acc;
  }
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    double t = 0.0, u = 0.0;
    for (int i = 0; i < m; ++i)
      t = add_rn(t, mul_rn(gen_sym(a.seed, gp, kn + (uint64_t)j * m + i), y0[i]));
    for (int i = 0; i < k; ++i)
      u = add_rn(u, mul_rn(gen_sym(a.seed, gp, (uint64_t)j * k + i), z0[i]));
    a.c[p * n + j] = -add_rn(t, u);
  }
}
#pragma clang fp contract(on)
}  // namespace

extern "C" int socp_generate(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                             const int32_t* cone_offs, const int32_t* cone_dim, uint64_t seed,
                             int64_t first_problem, double* c, double* A, double* b, double* G,
                             double* h) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  GenArgs a;
  memset(&a, 0, sizeof(a));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree));
  if (dims->batch == 0) return 0;
  if (first_problem < 0) return fail(SOCP_E_INVALID, "negative first_problem");
  if (!c || !G || !h || (dims->m > 0 && (!A || !b))) return fail(SOCP_E_INVALID, "NULL data pointer");
  if ((uint64_t)dims->k * dims->n + (uint64_t)dims->m * dims->n + dims->n + dims->m + 2 * dims->k >= (1ull << 24))
    return fail(SOCP_E_UNSUPPORTED, "problem too large for the 24-bit element counter");
  HIPCHK(hipSetDevice(ctx->device));
  a.B = dims->batch;
  a.first = first_problem;
  a.seed = seed;
  a.n = dims->n;
  a.m = dims->m;
  a.k = dims->k;
  a.nc = dims->ncones;
  a.c = c;
  a.A = A;
  a.b = b;
  a.G = G;
  a.h = h;
  size_t sh = sizeof(double) * (size_t)(a.n + a.m + 2 * a.k);
  if (sh > 64 * 1024) return fail(SOCP_E_UNSUPPORTED, "generator LDS too large");
  void* kargs[] = {&a};
  HIPCHK(hipLaunchKernel((const void*)&socp_generate_kernel, dim3((unsigned)a.B), dim3(256), kargs,
                         sh, ctx->stream));
  return 0;
}

// --------------------------------------------------------------- ingest
// socp_pack_csc: one workgroup per problem; the problem's dense block is
// zeroed by the workgroup, then every thread scatters a strided share of the
// nonzeros (column by column: the column of nonzero e is found by a binary
// search of colptr, so the scatter is one pass over nz).  A first pass checks
// that every column's row indices are strictly increasing; a problem where one
// is not (duplicates, or unsorted indices as a hand-built CSC may have) is
// packed a thread per column instead, each column's entries summed in input
// order, so repeated (i, j) entries add up as sparse() does and the result is
// deterministic bit for bit.
namespace {
__device__ __forceinline__ int csc_col(const int64_t* cp, int cols, int64_t base, int64_t e) {
  int lo = 0, hi = cols;  // invariant: cp[lo] - base <= e < cp[hi] - base
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cp[mid] - base <= e) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ void __launch_bounds__(256) socp_pack_csc_kernel(int32_t rows, int32_t cols, const int64_t* nz_offs,
                                                           const int64_t* colptr, const int64_t* rowval,
                                                           const double* nzval, int64_t base, double* dense,
                                                           int32_t* err) {
  __shared__ int unsorted;
  const int64_t p = blockIdx.x;
  const int64_t rc = (int64_t)rows * cols;
  double* D = dense + p * rc;
  if (threadIdx.x == 0) unsorted = 0;
  for (int64_t e = threadIdx.x; e < rc; e += blockDim.x) D[e] = 0.0;
  const int64_t* cp = colptr + p * (int64_t)(cols + 1);
  const int64_t n0 = nz_offs[p], nnz = nz_offs[p + 1] - n0;
  __syncthreads();
  if (cp[0] - base != 0 || cp[cols] - base != nnz) {
    if (threadIdx.x == 0) atomicOr(err, 1);
    return;
  }
  for (int64_t e = threadIdx.x; e + 1 < nnz; e += blockDim.x) {
    const int j = csc_col(cp, cols, base, e);
    if (e + 1 < cp[j + 1] - base && rowval[n0 + e + 1] <= rowval[n0 + e]) unsorted = 1;
  }
  __syncthreads();
  if (unsorted == 0) {  // canonical CSC (SparseMatrixCSC): one store per nonzero
    for (int64_t e = threadIdx.x; e < nnz; e += blockDim.x) {
      const int j = csc_col(cp, cols, base, e);
      const int64_t i = rowval[n0 + e] - base;
      if (i < 0 || i >= rows) {
        atomicOr(err, 2);
        continue;
      }
      D[(int64_t)j * rows + i] = nzval[n0 + e];
    }
    return;
  }
  // unsorted or duplicate row indices: a thread per column sums its entries in
  // input order (sparse()'s combine), so the result is deterministic bit for bit
  for (int j = threadIdx.x; j < cols; j += blockDim.x) {
    for (int64_t e = cp[j] - base; e < cp[j + 1] - base; ++e) {
      const int64_t i = rowval[n0 + e] - base;
      if (i < 0 || i >= rows) {
        atomicOr(err, 2);
        continue;
      }
      D[(int64_t)j * rows + i] += nzval[n0 + e];
    }
  }
}
}  // namespace

void host::pack_csc_launch(hipStream_t stream, int64_t batch, int32_t rows, int32_t cols, const int64_t* nz_offs,
                           const int64_t* colptr, const int64_t* rowval, const double* nzval, int64_t base,
                           double* dense, int32_t* err) {
  hipLaunchKernelGGL(socp_pack_csc_kernel, dim3((unsigned)batch), dim3(256), 0, stream, rows, cols, nz_offs, colptr,
                     rowval, nzval, base, dense, err);
}

extern "C" int socp_pack_csc(socp_ctx* ctx, int64_t batch, int32_t rows, int32_t cols, const int64_t* nz_offs,
                             const int64_t* colptr, const int64_t* rowval, const double* nzval,
                             int32_t index_base, double* dense) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  if (batch < 0 || rows < 0 || cols < 0 || (index_base != 0 && index_base != 1))
    return fail(SOCP_E_INVALID, "bad batch/rows/cols/index_base");
  if (batch > kMaxBatch) return fail(SOCP_E_INVALID, "batch above 2^31-1 (one workgroup per problem)");
  if (batch == 0 || (int64_t)rows * cols == 0) return 0;
  if (!nz_offs || !colptr || !dense) return fail(SOCP_E_INVALID, "NULL pointer");
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->buf[socp_ctx::B_ERR].ensure(256)) return fail(SOCP_E_NOMEM, "device allocation failed");
  int32_t* err = (int32_t*)ctx->buf[socp_ctx::B_ERR].p;
  HIPCHK(hipMemsetAsync(err, 0, sizeof(int32_t), ctx->stream));
  pack_csc_launch(ctx->stream, batch, rows, cols, nz_offs, colptr, rowval, nzval, index_base, dense, err);
  HIPCHK(hipGetLastError());
  int32_t herr = 0;
  HIPCHK(hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (herr & 1) return fail(SOCP_E_INVALID, "colptr does not span the problem's nonzeros");
  if (herr & 2) return fail(SOCP_E_INVALID, "row index out of range");
  return 0;
}

// ------------------------------------------- the gather's records (socp_api_comm.hip)
namespace {
// 32-byte outcome record (include/socp.h socp_outcome): status, iters, and the
// exit-test quantities ||rd||, ||rp||, z's (solver.jl:109-122)
__global__ void socp_outcome_kernel(int64_t B, const int32_t* __restrict__ status, const int32_t* __restrict__ iters,
                                    const double* __restrict__ res, socp_outcome* __restrict__ rec) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < B) {
    socp_outcome o;
    o.status = status[p];
    o.iters = iters[p];
    o.res_dual = res ? res[3 * p] : NAN;
    o.res_primal = res ? res[3 * p + 1] : NAN;
    o.gap = res ? res[3 * p + 2] : NAN;
    rec[p] = o;
  }
}

__global__ void socp_pair_kernel(int64_t B, const int32_t* __restrict__ status, const int32_t* __restrict__ iters,
                                 int32_t* __restrict__ pairs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < B) {
    pairs[2 * p] = status[p];
    pairs[2 * p + 1] = iters[p];
  }
}
}  // namespace

void host::pair_launch(hipStream_t stream, int64_t B, const int32_t* status, const int32_t* iters, int32_t* pairs) {
  hipLaunchKernelGGL(socp_pair_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, status, iters,
                     pairs);
}
void host::outcome_launch(hipStream_t stream, int64_t B, const int32_t* status, const int32_t* iters,
                          const double* res, socp_outcome* rec) {
  hipLaunchKernelGGL(socp_outcome_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, status, iters,
                     res, rec);
}
