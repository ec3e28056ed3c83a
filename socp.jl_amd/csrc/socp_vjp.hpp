// socp_vjp.hpp — differentiable solves (include/socp.h socp_batch_centre,
// socp_batch_vjp, socp_batch_vjp_sum): the arguments and host
// launchers of the kernels in socp_vjp.hip.  Every pointer is a device pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "socp_small.hpp"  // ConeTable, MAXC, POC_K, SOC_K

namespace socp {

constexpr int VJP_THREADS = 256;          // four wavefronts per problem
constexpr int CENTRE_MAX_STEPS = 16;      // socp_batch_centre's upper bound on `steps`
constexpr int CENTRE_MIN_STEP_EXP = -30;  // the halving loop gives up below 2^-30

// One workgroup per problem.  P, A, G and sing are per problem, or the batch's
// one with `shared`; P may be NULL (no quadratic term), A, b, y are NULL when m = 0.
struct CentreArgs {
  const double* P;  // n x n
  const double* c;
  const double* A;  // m x n
  const double* b;
  const double* G;  // k x n
  const double* h;
  double *x, *y, *z, *s;          // the iterate, updated in place by centre_update
  double *dx, *dy, *dz, *ds;      // the right-hand side (centre_rhs, and centre_update's final pass)
  const double *cx, *cy, *cz, *cs;  // the KKT solve's step; cx == NULL: centre_update takes no step
  const int32_t* kst;             // the KKT solve's status per problem
  int32_t* status;                // per problem: 0, or what stopped it (it then keeps its last good iterate)
  double* res;                    // 4 per problem or NULL: |rd|, |rp|, z's, |lam o lam - mu e| / mu
  int32_t n, m, k, nc, deg;
  int32_t shared;
  ConeTable cones;
};

struct VjpArgs {
  const double* G;  // k x n (vjp_rhs)
  const double *x, *y, *z;         // the point (vjp_assemble; y NULL when m = 0)
  const double *gx, *gs;           // upstream gradients, NULL meaning zero
  double* rx;                      // vjp_rhs: gx - G'gs
  const double *ux, *uy, *uz;      // the KKT solve's solution
  const int32_t* kst;              // its status
  const int32_t* skip;             // NULL, or per problem: nonzero masks the problem
  int32_t* status;                 // skip[p] where nonzero, else kst[p]
  double *dc, *db, *dh, *dP, *dA, *dG, *oux, *ouy, *ouz;  // outputs, each may be NULL
  int32_t n, m, k;
  int32_t shared;
};

// plain launches on `stream`; the caller checks the returned error
hipError_t centre_rhs_launch(const CentreArgs& a, int64_t B, hipStream_t stream);
// last: also form the right-hand side at the updated point and, from it, res
hipError_t centre_update_launch(const CentreArgs& a, int64_t B, bool last, hipStream_t stream);
// the last pass's refinement: dx, dy, dz become the linear rows' residual of (cx, cy, cz, cs) ...
hipError_t centre_refine_launch(const CentreArgs& a, int64_t B, hipStream_t stream);
// ... and the second solve's (ex, ey, ez, es) is added to the step where the KKT status is 0
hipError_t centre_add_launch(const CentreArgs& a, const double* ex, const double* ey, const double* ez,
                             const double* es, int64_t B, hipStream_t stream);
hipError_t vjp_rhs_launch(const VjpArgs& a, int64_t B, hipStream_t stream);
hipError_t vjp_assemble_launch(const VjpArgs& a, int64_t B, hipStream_t stream);

// socp_batch_vjp_sum: the gradients of a batch's one P, A and G as sums over the
// problems with status 0,
//   dG = -sum (z ux' + w x'), dA = -sum (y ux' + uy x'), dP = -(M + M')/2, M = sum ux x',
// w = uz + gs.  The batch is cut into `slabs` runs of `slab` consecutive problems
// (vjp_sum_plan); vjp_sum_partial writes one partial sum per slab and output into
// `part`, slab s at part + s * (k n + m n + n^2): dG's k x n, dA's m x n, M's n x n,
// column-major; vjp_sum_combine adds them in ascending slab order.
constexpr int64_t VJP_SUM_SLAB = 512;               // problems per slab ...
constexpr int64_t VJP_SUM_WS_CAP = (int64_t)64 << 20;  // ... doubled while the partials would pass this many bytes

struct VjpSumArgs {
  const double *x, *y, *z;     // the point (y NULL when m = 0)
  const double *ux, *uy, *uz;  // the KKT solve's solution: NaN where it failed, never read there
  const double* gs;            // NULL: zero
  const int32_t* status;       // vjp_assemble's: a problem counts where it is 0
  double* part;                // slabs * (k n + m n + n^2) doubles
  double *dP, *dA, *dG;        // ONE n x n, m x n, k x n; each may be NULL and is then skipped
  int64_t B, slab, slabs;
  int32_t n, m, k;
};

// the slab rule, a pure function of (B, n, m, k); B >= 1
inline void vjp_sum_plan(int64_t B, int n, int m, int k, int64_t* slabs, int64_t* slab) {
  const int64_t out = ((int64_t)k + m + n) * n;
  int64_t s = VJP_SUM_SLAB;
  while ((B + s - 1) / s > 1 && (B + s - 1) / s * out * (int64_t)sizeof(double) > VJP_SUM_WS_CAP) s *= 2;
  *slab = s;
  *slabs = (B + s - 1) / s;
}

hipError_t vjp_sum_partial_launch(const VjpSumArgs& a, hipStream_t stream);
hipError_t vjp_sum_combine_launch(const VjpSumArgs& a, hipStream_t stream);

}  // namespace socp
