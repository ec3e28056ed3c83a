// socp_vjp.hip — the kernels of socp_batch_centre and socp_batch_vjp
// (include/socp.h).  One 256-thread workgroup (four wave64
// wavefronts) per problem; strided loops and 64-bit matrix offsets, so every
// shape socp_supported accepts runs (n, m <= 2048, k <= 2^21).  The KKT solve
// between centre_rhs and centre_update, and between vjp_rhs and vjp_assemble,
// is the fused plugin entry's own launch (socp_api_vjp.hip); the last centring
// pass refines its step by a second one (centre_refine, centre_add).
// socp_batch_vjp_sum's two kernels (vjp_sum_partial, vjp_sum_combine) are at the
// end: the batch is their inner dimension, not their grid.
//
// Matrices are column-major: a column's dot product with a vector (G'z, A'y,
// Px with P symmetric, G'gs) is one column per wavefront, lanes down the column,
// and a wave reduction; a row's (Gx, Ax) is one row per lane, the lanes of a
// wavefront reading consecutive rows of the same column.  The reductions are in
// a fixed order, so a result does not depend on where the problem sits in the
// batch or on SOCP_F_SHARED_MATRICES.
#include "socp_vjp.hpp"

namespace socp {
namespace {

constexpr int NT = VJP_THREADS;
constexpr int NW = NT / 64;

// every lane gets the same bits: a + b == b + a at each level of the butterfly
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a workgroup's LDS: the reductions' slots, and per cone z0^2 - |z1|^2, s0^2 - |s1|^2 and zbar'sbar
struct Scratch {
  double red[NW];
  double onrm[3 * MAXC];
};

// the sum over the workgroup, the same bits in every thread
__device__ inline double block_sum(double v, Scratch* sc) {
  double* red = sc->red;
  v = wave_sum(v);
  __syncthreads();  // (the last call's readers are done with red)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}

struct Problem {
  const double *P, *A, *G;
  int64_t p;
};
__device__ inline Problem problem_of(const CentreArgs& a) {
  Problem q;
  q.p = (int64_t)blockIdx.x;
  const int64_t mp = a.shared ? 0 : q.p;
  q.P = a.P ? a.P + mp * a.n * a.n : nullptr;
  q.A = a.m > 0 ? a.A + mp * a.m * a.n : nullptr;
  q.G = a.G + mp * a.k * a.n;
  return q;
}

__device__ void form_ds(const CentreArgs& a, const double* z, const double* s, double* ds, double mu, Scratch* red);

// The three linear block rows at (x, y, z, s):
//   dx = -(Px + A'y + G'z + csign c), dy = -(Ax - b), dz = -(Gx + s - h).
// An output may be its own c, b or h (each element is read and written by one lane).
// Returns the thread's share of s'z.
__device__ double linear_rows(const Problem& q, int n, int m, int k, const double* x, const double* y,
                              const double* z, const double* s, const double* c, double csign, const double* b,
                              const double* h, double* dx, double* dy, double* dz) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int j = w; j < n; j += NW) {
    const double* g = q.G + (int64_t)j * k;
    double acc = 0.0;
    for (int i = lane; i < k; i += 64) acc += g[i] * z[i];
    if (m > 0) {
      const double* ac = q.A + (int64_t)j * m;
      for (int i = lane; i < m; i += 64) acc += ac[i] * y[i];
    }
    if (q.P) {
      const double* pc = q.P + (int64_t)j * n;
      for (int i = lane; i < n; i += 64) acc += pc[i] * x[i];
    }
    acc = wave_sum(acc);
    if (lane == 0) dx[j] = -(acc + csign * c[j]);
  }
  for (int i = tid; i < m; i += NT) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc += q.A[(int64_t)j * m + i] * x[j];
    dy[i] = -(acc - b[i]);
  }
  double sz = 0.0;
  for (int i = tid; i < k; i += NT) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc += q.G[(int64_t)j * k + i] * x[j];
    dz[i] = -(acc + s[i] - h[i]);
    sz += s[i] * z[i];
  }
  return sz;
}

// The centring step's right-hand side at the iterate (x, y, z, s):
//   dx = -(Px + c + A'y + G'z), dy = -(Ax - b), dz = -(Gx + s - h), ds = mu e - lam o lam
// with mu = s'z / deg and lam compute_scaling's l (scalings.jl:22-99).  lam is formed without
// fused multiply-adds, and a cone's three sums z0^2 - |z1|^2, s0^2 - |s1|^2 and zbar'sbar --
// which cancel to about mu of their terms near a solution, so that their rounding is the
// whole error of lam -- in the reference's own sequential order, one cone per thread: lam is
// then compute_scaling's at the same point, and so is the off-centre measure in res.  Returns s'z;
// *mu_out = mu.  Ends without a barrier: the caller synchronises before reading dx .. ds.
__device__ double form_rhs(const CentreArgs& a, const Problem& q, Scratch* red, double* mu_out) {
  const int n = a.n, m = a.m, k = a.k;
  const double* z = a.z + q.p * k;
  const double* s = a.s + q.p * k;
  double* ds = a.ds + q.p * k;
  double sz = linear_rows(q, n, m, k, a.x + q.p * n, m > 0 ? a.y + q.p * m : nullptr, z, s, a.c + q.p * n, 1.0,
                          m > 0 ? a.b + q.p * m : nullptr, a.h + q.p * k, a.dx + q.p * n,
                          m > 0 ? a.dy + q.p * m : nullptr, a.dz + q.p * k);
  sz = block_sum(sz, red);
  const double mu = sz / (double)a.deg;
  *mu_out = mu;
  form_ds(a, z, s, ds, mu, red);
  return sz;
}

// ds = mu e - lam o lam (form_rhs)
__device__ void form_ds(const CentreArgs& a, const double* z, const double* s, double* ds, double mu, Scratch* red) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (int cn = tid; cn < a.nc; cn += NT) {
    if (a.cones.kind[cn] == POC_K) continue;
    const int o = a.cones.offs[cn], d = a.cones.dim[cn];
    double oz = z[o] * z[o], os = s[o] * s[o];
    for (int i = 1; i < d; ++i) {
      oz -= z[o + i] * z[o + i];
      os -= s[o + i] * s[o + i];
    }
    const double fz = 1.0 / sqrt(oz), fs = 1.0 / sqrt(os);
    double ns = 0.0;
    for (int i = 0; i < d; ++i) ns += (z[o + i] * fz) * (s[o + i] * fs);
    red->onrm[3 * cn] = oz;
    red->onrm[3 * cn + 1] = os;
    red->onrm[3 * cn + 2] = ns;
  }
  __syncthreads();
  for (int cn = 0; cn < a.nc; ++cn) {
    const int o = a.cones.offs[cn], d = a.cones.dim[cn];
    if (a.cones.kind[cn] == POC_K) {
      for (int i = tid; i < d; i += NT) {
        const double l = sqrt(s[o + i] * z[o + i]);
        ds[o + i] = mu - l * l;
      }
      continue;
    }
    const double nrmz = sqrt(red->onrm[3 * cn]), nrms = sqrt(red->onrm[3 * cn + 1]), ns = red->onrm[3 * cn + 2];
    const double fz = 1.0 / nrmz, fs = 1.0 / nrms;
    const double gamma = sqrt((1.0 + ns) / 2.0);
    const double zb0 = z[o] * fz, sb0 = s[o] * fs;
    const double tmv1 = sqrt(nrms * nrmz);
    const double mult = tmv1 / (zb0 + sb0 + 2.0 * gamma);
    const double gs = gamma + zb0, gz = gamma + sb0;
    const double l0 = gamma * tmv1;
    double ll = 0.0;
    for (int i = 1 + tid; i < d; i += NT) {
      const double l = ((s[o + i] * fs) * gs + (z[o + i] * fz) * gz) * mult;
      ll += l * l;
      ds[o + i] = -(2.0 * l0 * l);
    }
    ll = block_sum(ll, red);
    if (tid == 0) ds[o] = mu - (l0 * l0 + ll);
  }
}

__global__ __launch_bounds__(NT) void centre_rhs_kernel(const CentreArgs a) {
  __shared__ Scratch red;
  const Problem q = problem_of(a);
  double mu;
  form_rhs(a, q, &red, &mu);
}

// One step of iterative refinement of the last pass's KKT solve, on the three linear rows:
// (dx, dy, dz) becomes the residual (dx - (P cx + A'cy + G'cz), dy - A cx, dz - (G cx + cs))
// of the solution (cx, cy, cz, cs); the host zeroes ds and solves again.
__global__ __launch_bounds__(NT) void centre_refine_kernel(const CentreArgs a) {
  const Problem q = problem_of(a);
  const int n = a.n, m = a.m, k = a.k;
  linear_rows(q, n, m, k, a.cx + q.p * n, m > 0 ? a.cy + q.p * m : nullptr, a.cz + q.p * k, a.cs + q.p * k,
              a.dx + q.p * n, -1.0, m > 0 ? a.dy + q.p * m : nullptr, a.dz + q.p * k, a.dx + q.p * n,
              m > 0 ? a.dy + q.p * m : nullptr, a.dz + q.p * k);
}

// c += e on the four vectors of a step (e: the refinement's solution, in dx .. ds's place in the arguments)
__global__ __launch_bounds__(NT) void centre_add_kernel(double* cx, double* cy, double* cz, double* cs,
                                                        const double* ex, const double* ey, const double* ez,
                                                        const double* es, const int32_t* kst, int n, int m, int k) {
  const int64_t p = (int64_t)blockIdx.x;
  if (kst[p]) return;  // (a failed solve's vectors are not read)
  const int tid = threadIdx.x;
  for (int j = tid; j < n; j += NT) cx[p * n + j] += ex[p * n + j];
  for (int i = tid; i < m; i += NT) cy[p * m + i] += ey[p * m + i];
  for (int i = tid; i < k; i += NT) {
    cz[p * k + i] += ez[p * k + i];
    cs[p * k + i] += es[p * k + i];
  }
}

// whether v + t dv is interior: POC entries > 0, SOC heads > sqrt(sum of the tail's squares)
__device__ bool interior(const CentreArgs& a, const double* v, const double* dv, double t, Scratch* red) {
  const int tid = threadIdx.x;
  double bad = 0.0;
  for (int cn = 0; cn < a.nc; ++cn) {
    const int o = a.cones.offs[cn], d = a.cones.dim[cn];
    if (a.cones.kind[cn] == POC_K) {
      for (int i = tid; i < d; i += NT)
        if (!(v[o + i] + t * dv[o + i] > 0.0)) bad += 1.0;
      continue;
    }
    double qd = 0.0;
    for (int i = 1 + tid; i < d; i += NT) {
      const double u = v[o + i] + t * dv[o + i];
      qd += u * u;
    }
    qd = block_sum(qd, red);
    if (!(v[o] + t * dv[o] > sqrt(qd))) bad += 1.0;  // (every thread: NaN counts as outside)
  }
  return block_sum(bad, red) == 0.0;
}

// The step of one centring pass: t = 1, halved while z + t cz or s + t cs is not
// interior (status SOCP_DOMAIN_ERROR below 2^-30), then the four vectors move by
// t times the step.  A problem whose KKT solve failed, or that stopped in an
// earlier pass, keeps its iterate.  `last`: res at the returned point.
__global__ __launch_bounds__(NT) void centre_update_kernel(const CentreArgs a, int last) {
  __shared__ Scratch scratch;
  Scratch* red = &scratch;
  const int tid = threadIdx.x;
  const Problem q = problem_of(a);
  const int n = a.n, m = a.m, k = a.k;
  if (a.cx) {
    const int st = a.status[q.p], kst = a.kst[q.p];
    __syncthreads();  // every thread has read the status before thread 0 may write it
    if (st == 0 && kst != 0) {
      if (tid == 0) a.status[q.p] = kst;
    } else if (st == 0) {
      double* z = a.z + q.p * k;
      double* s = a.s + q.p * k;
      const double* cz = a.cz + q.p * k;
      const double* cs = a.cs + q.p * k;
      double t = 1.0;
      bool found = false;
      for (int e = 0; e >= CENTRE_MIN_STEP_EXP; --e, t *= 0.5) {
        found = interior(a, z, cz, t, red) && interior(a, s, cs, t, red);
        if (found) break;
      }
      __syncthreads();
      if (!found) {
        if (tid == 0) a.status[q.p] = ST_DOMAIN;
      } else {
        double* x = a.x + q.p * n;
        const double* cx = a.cx + q.p * n;
        for (int j = tid; j < n; j += NT) x[j] = x[j] + t * cx[j];
        if (m > 0) {
          double* y = a.y + q.p * m;
          const double* cy = a.cy + q.p * m;
          for (int i = tid; i < m; i += NT) y[i] = y[i] + t * cy[i];
        }
        for (int i = tid; i < k; i += NT) {
          z[i] = z[i] + t * cz[i];
          s[i] = s[i] + t * cs[i];
        }
      }
    }
  }
  if (!last || !a.res) return;
  __syncthreads();  // the workgroup's own update is visible to all of it
  double mu;
  const double sz = form_rhs(a, q, red, &mu);
  __syncthreads();
  const double* dx = a.dx + q.p * n;
  const double* ds = a.ds + q.p * k;
  double rd = 0.0, rp = 0.0, oc = 0.0;
  for (int j = tid; j < n; j += NT) rd += dx[j] * dx[j];
  if (m > 0) {
    const double* dy = a.dy + q.p * m;
    for (int i = tid; i < m; i += NT) rp += dy[i] * dy[i];
  }
  for (int i = tid; i < k; i += NT) oc += ds[i] * ds[i];
  rd = block_sum(rd, red);
  rp = block_sum(rp, red);
  oc = block_sum(oc, red);
  if (tid < 4) {
    const double v = tid == 0 ? sqrt(rd) : tid == 1 ? sqrt(rp) : tid == 2 ? sz : sqrt(oc) / mu;
    a.res[q.p * 4 + tid] = v;
  }
}

// rx = gx - G'gs (either may be NULL: zero)
__global__ __launch_bounds__(NT) void vjp_rhs_kernel(const VjpArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t p = (int64_t)blockIdx.x;
  const int n = a.n, k = a.k;
  const double* G = a.G + (a.shared ? 0 : p) * k * n;
  const double* gs = a.gs ? a.gs + p * k : nullptr;
  const double* gx = a.gx ? a.gx + p * n : nullptr;
  double* rx = a.rx + p * n;
  for (int j = w; j < n; j += NW) {
    double acc = 0.0;
    if (gs) {
      const double* g = G + (int64_t)j * k;
      for (int i = lane; i < k; i += 64) acc += g[i] * gs[i];
      acc = wave_sum(acc);
    }
    if (lane == 0) rx[j] = (gx ? gx[j] : 0.0) - acc;
  }
}

// out[j * rows + i] = f(i, j): consecutive threads write consecutive addresses
template <class F>
__device__ inline void write_matrix(double* out, int rows, int cols, F f) {
  const int tid = threadIdx.x;
  if (rows >= 64) {
    const int lane = tid & 63, w = tid >> 6;
    for (int j = w; j < cols; j += NW) {
      double* col = out + (int64_t)j * rows;
      for (int i = lane; i < rows; i += 64) col[i] = f(i, j);
    }
  } else {  // short columns: the matrix as one run (below 64 * 2048 elements)
    const int total = rows * cols;
    for (int idx = tid; idx < total; idx += NT) out[idx] = f(idx % rows, idx / rows);
  }
}

// the six gradients and the adjoint variables from the KKT solution; a masked
// problem (skip[p] != 0, or a failed KKT solve) writes zeros
__global__ __launch_bounds__(NT) void vjp_assemble_kernel(const VjpArgs a) {
  const int tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x;
  const int n = a.n, m = a.m, k = a.k;
  const int sk = a.skip ? a.skip[p] : 0;
  const int st = sk ? sk : a.kst[p];
  const bool on = st == 0;
  if (tid == 0) a.status[p] = st;
  const double* ux = a.ux + p * n;
  const double* uy = m > 0 ? a.uy + p * m : nullptr;
  const double* uz = a.uz + p * k;
  const double* gs = a.gs ? a.gs + p * k : nullptr;
  const double* x = a.x + p * n;
  const double* y = m > 0 ? a.y + p * m : nullptr;
  const double* z = a.z + p * k;
  if (a.dc || a.oux)
    for (int j = tid; j < n; j += NT) {
      const double u = on ? ux[j] : 0.0;
      if (a.dc) a.dc[p * n + j] = on ? -u : 0.0;
      if (a.oux) a.oux[p * n + j] = u;
    }
  if (m > 0 && (a.db || a.ouy))
    for (int i = tid; i < m; i += NT) {
      const double u = on ? uy[i] : 0.0;
      if (a.db) a.db[p * m + i] = u;
      if (a.ouy) a.ouy[p * m + i] = u;
    }
  if (a.dh || a.ouz)
    for (int i = tid; i < k; i += NT) {
      const double u = on ? uz[i] : 0.0;
      if (a.dh) a.dh[p * k + i] = on ? u + (gs ? gs[i] : 0.0) : 0.0;
      if (a.ouz) a.ouz[p * k + i] = u;
    }
  if (a.dP) {
    double* o = a.dP + p * n * n;
    if (on)
      write_matrix(o, n, n, [=](int i, int j) { return -(ux[i] * x[j] + x[i] * ux[j]) * 0.5; });
    else
      write_matrix(o, n, n, [](int, int) { return 0.0; });
  }
  if (a.dA && m > 0) {
    double* o = a.dA + p * m * n;
    if (on)
      write_matrix(o, m, n, [=](int i, int j) { return -(y[i] * ux[j] + uy[i] * x[j]); });
    else
      write_matrix(o, m, n, [](int, int) { return 0.0; });
  }
  if (a.dG) {
    double* o = a.dG + p * k * n;
    if (on)
      write_matrix(o, k, n, [=](int i, int j) {
        const double wi = uz[i] + (gs ? gs[i] : 0.0);
        return -(z[i] * ux[j] + wi * x[j]);
      });
    else
      write_matrix(o, k, n, [](int, int) { return 0.0; });
  }
}

// ------------------------------------------------------- socp_batch_vjp_sum
// The sums over the batch (socp_vjp.hpp).  The three outputs are one stack of
// 16-row tiles: dG's ceil(k/16), dA's ceil(m/16), M's ceil(n/16), by ceil(n/16)
// column tiles.  A wavefront owns one 16 x 16 tile of one slab and walks the
// slab four problems per v_mfma_f64_16x16x4_f64: the batch is the inner
// dimension, so lane (r = lane & 15, q = lane >> 4) holds row i0 + r of problem
// p0 + q's column vector as the A operand and column j0 + r of its row vector as
// the B operand -- one 128-byte run per problem and tile edge.  A tile of dG is
// two chains, (z, ux) and (w, x); of dA, (y, ux) and (uy, x); of M, (ux, x).
// The four wavefronts of a workgroup are CW column tiles by 4 / CW row tiles
// (CW = 4, 2, 1 as n > 32, n > 16, else), so that a row tile's operands are
// fetched from memory once per workgroup and the other wavefronts hit the cache.
// Rows, columns and problems out of range, and problems that do not count, are
// 0.0 by selection: a failed solve's NaN is never an operand.
constexpr int SUM_STEPS = 4;  // steps of four problems whose loads are in flight together

struct SumTile {
  const double *a0, *a1;  // the two chains' column vectors (a0 NULL: one chain); both chains' row vectors are ux, x
  const double* a1b;      // added to a1's elements when not NULL (w = uz + gs)
  int rows, lda;          // rows of the output, elements per problem of a0 / a1
  int64_t off;            // the output's place in a slab's partials
};

__device__ inline bool sum_tile_of(const VjpSumArgs& a, int rt, SumTile* t) {
  const int KT = (a.k + 15) >> 4, MT = (a.m + 15) >> 4;
  t->a1b = nullptr;
  if (rt < KT) {
    if (!a.dG) return false;
    *t = SumTile{a.z, a.uz, a.gs, a.k, a.k, 0};
  } else if (rt < KT + MT) {
    if (!a.dA) return false;
    *t = SumTile{a.y, a.uy, nullptr, a.m, a.m, (int64_t)a.k * a.n};
  } else {
    if (!a.dP) return false;
    *t = SumTile{nullptr, a.ux, nullptr, a.n, a.n, ((int64_t)a.k + a.m) * a.n};
  }
  return true;
}

__global__ __launch_bounds__(NT) void vjp_sum_partial_kernel(const VjpSumArgs a, int64_t items, int RG, int CG,
                                                             int CW) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n = a.n, RW = NW / CW;
  const int KT = (a.k + 15) >> 4, MT = (a.m + 15) >> 4, RT = KT + MT + ((n + 15) >> 4), CT = (n + 15) >> 4;
  const int64_t out = ((int64_t)a.k + a.m + n) * n;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int rg = (int)(item % RG), cg = (int)(item / RG % CG);
    const int64_t slab = item / RG / CG;
    const int rt = rg * RW + w / CW, ct = cg * CW + w % CW;
    if (rt >= RT || ct >= CT) continue;
    SumTile t;
    if (!sum_tile_of(a, rt, &t)) continue;
    const int i0 = (rt - (rt < KT ? 0 : rt < KT + MT ? KT : KT + MT)) << 4, j0 = ct << 4;
    const bool rin = i0 + r < t.rows, cin = j0 + r < n;
    const int64_t pbeg = slab * a.slab, pend = pbeg + a.slab < a.B ? pbeg + a.slab : a.B;
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    // SUM_STEPS steps' operands are loaded before their matrix instructions issue: a step alone would wait
    // one memory latency per four problems.  The accumulation order is the problems' order either way.
    for (int64_t p0 = pbeg; p0 < pend; p0 += 4 * SUM_STEPS) {
      double va0[SUM_STEPS], va1[SUM_STEPS], vux[SUM_STEPS], vx[SUM_STEPS];
#pragma unroll
      for (int u = 0; u < SUM_STEPS; ++u) {
        // every load is from a valid address (a lane out of range reads its slab's first element) and does
        // not wait for the status; what does not count is dropped by selection afterwards
        const int64_t p = p0 + 4 * u + q;
        const bool inb = p < pend;
        const int64_t ps = inb ? p : pbeg;
        const int st = a.status[ps];
        const int64_t ea = ps * t.lda + (rin ? i0 + r : 0), eb = ps * n + (cin ? j0 + r : 0);
        const double la0 = t.a0 ? t.a0[ea] : 0.0, la1 = t.a1[ea], lab = t.a1b ? t.a1b[ea] : 0.0;
        const double lux = t.a0 ? a.ux[eb] : 0.0, lx = a.x[eb];
        const bool on = inb && st == 0;
        va0[u] = on && rin ? la0 : 0.0;
        va1[u] = on && rin ? la1 + lab : 0.0;
        vux[u] = on && cin ? lux : 0.0;
        vx[u] = on && cin ? lx : 0.0;
      }
#pragma unroll
      for (int u = 0; u < SUM_STEPS; ++u) {
        if (t.a0) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va0[u], vux[u], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va1[u], vx[u], acc1, 0, 0, 0);
      }
    }
    // C/D layout: lane (q, r) holds row q + 4 s, column r in register s
    double* o = a.part + slab * out + t.off;
    if (cin) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int i = i0 + q + 4 * s;
        if (i < t.rows) o[(int64_t)(j0 + r) * t.rows + i] = t.a0 ? acc0[s] + acc1[s] : acc1[s];
      }
    }
  }
}

// One thread per output element: the slabs' partials in ascending order, then the sign, and for dP
// the mean of M's (i, j) and (j, i) sums -- the same expression for both, so dP is symmetric in bits.
__global__ __launch_bounds__(NT) void vjp_sum_combine_kernel(const VjpSumArgs a) {
  const int n = a.n;
  const int64_t kn = (int64_t)a.k * n, mn = (int64_t)a.m * n, out = kn + mn + (int64_t)n * n;
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < out; e += (int64_t)gridDim.x * NT) {
    if (e < kn ? !a.dG : e < kn + mn ? !a.dA : !a.dP) continue;
    const double* src = a.part + e;
    double sum = 0.0;
    if (e < kn + mn) {
#pragma unroll 8
      for (int64_t s = 0; s < a.slabs; ++s) sum += src[s * out];
      if (e < kn)
        a.dG[e] = 0.0 - sum;
      else
        a.dA[e - kn] = 0.0 - sum;
    } else {
      const int64_t f = e - kn - mn;
      const int i = (int)(f % n), j = (int)(f / n);
      const double* mir = a.part + kn + mn + (int64_t)i * n + j;
      double tsum = 0.0;
#pragma unroll 8
      for (int64_t s = 0; s < a.slabs; ++s) {
        sum += src[s * out];
        tsum += mir[s * out];
      }
      a.dP[f] = 0.0 - (sum + tsum) * 0.5;
    }
  }
}

}  // namespace

hipError_t vjp_sum_partial_launch(const VjpSumArgs& a, hipStream_t stream) {
  const int CT = (a.n + 15) >> 4, RT = ((a.k + 15) >> 4) + ((a.m + 15) >> 4) + CT;
  const int CW = CT >= 3 ? 4 : CT, RW = NW / CW;
  const int RG = (RT + RW - 1) / RW, CG = (CT + CW - 1) / CW;
  const int64_t items = a.slabs * RG * CG;
  const int64_t grid = items < ((int64_t)1 << 20) ? items : (int64_t)1 << 20;  // (the kernel strides over the rest)
  hipLaunchKernelGGL(vjp_sum_partial_kernel, dim3((unsigned)grid), dim3(NT), 0, stream, a, items, RG, CG, CW);
  return hipGetLastError();
}
hipError_t vjp_sum_combine_launch(const VjpSumArgs& a, hipStream_t stream) {
  const int64_t out = ((int64_t)a.k + a.m + a.n) * a.n;
  const int64_t blocks = (out + NT - 1) / NT;
  const int64_t grid = blocks < ((int64_t)1 << 20) ? blocks : (int64_t)1 << 20;
  hipLaunchKernelGGL(vjp_sum_combine_kernel, dim3((unsigned)grid), dim3(NT), 0, stream, a);
  return hipGetLastError();
}

hipError_t centre_rhs_launch(const CentreArgs& a, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(centre_rhs_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a);
  return hipGetLastError();
}
hipError_t centre_update_launch(const CentreArgs& a, int64_t B, bool last, hipStream_t stream) {
  hipLaunchKernelGGL(centre_update_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a, last ? 1 : 0);
  return hipGetLastError();
}
hipError_t centre_refine_launch(const CentreArgs& a, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(centre_refine_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a);
  return hipGetLastError();
}
hipError_t centre_add_launch(const CentreArgs& a, const double* ex, const double* ey, const double* ez,
                             const double* es, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(centre_add_kernel, dim3((unsigned)B), dim3(NT), 0, stream, const_cast<double*>(a.cx),
                     const_cast<double*>(a.cy), const_cast<double*>(a.cz), const_cast<double*>(a.cs), ex, ey, ez, es,
                     a.kst, a.n, a.m, a.k);
  return hipGetLastError();
}
hipError_t vjp_rhs_launch(const VjpArgs& a, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(vjp_rhs_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a);
  return hipGetLastError();
}
hipError_t vjp_assemble_launch(const VjpArgs& a, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(vjp_assemble_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace socp
