// socp_vjp.hpp — differentiable solves (include/socp.h socp_batch_centre,
// socp_batch_vjp): the arguments and host launchers of the four
// kernels in socp_vjp.hip.  Every pointer is a device pointer.
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

}  // namespace socp
