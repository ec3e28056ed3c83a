// socp_api_vjp.hip — differentiable solves (include/socp.h):
// socp_batch_centre, socp_batch_vjp and socp_batch_vjp_sum.  Host code only; the kernels are
// socp_vjp.hip's, and every KKT solve is the fused plugin entry itself
// (socp_batch_kkt_solve_qp on device buffers: choose_engine and the kernels of
// a caller's own call), so no solver or plugin kernel is launched differently.
// That entry uses the context's B_C, B_CNT and B_LWS buffers; what is staged
// here stays clear of them.  socp_batch_vjp_sum's partial sums live in B_VSUM.
#include "socp_host.hpp"
#include "socp_vjp.hpp"

using namespace socp;
using namespace socp::host;

namespace {

constexpr int32_t kKktFlags = SOCP_F_FORCE_LARGE | SOCP_F_SHARED_MATRICES;

// the flags both entries take; `who` names the entry in the error text
int check_flags(int32_t flags, const char* who) {
  if (flags & SOCP_F_EXPLICIT_INVERSE)
    return fail(SOCP_E_UNSUPPORTED, std::string(who) + " with SOCP_F_EXPLICIT_INVERSE: the QP plugin-entry kernels "
                                                       "are not compiled in the explicit-inverse operation order");
  if (flags & ~(SOCP_F_DEVICE_PTRS | kKktFlags))
    return fail(SOCP_E_INVALID, std::string(who) + ": flags other than SOCP_F_DEVICE_PTRS | SOCP_F_FORCE_LARGE | "
                                                   "SOCP_F_SHARED_MATRICES");
  return 0;
}

// `count` doubles of zeros in ctx->buf[slot]
int zeros(socp_ctx* ctx, int slot, size_t count, const double** o) {
  *o = nullptr;
  if (count == 0) return 0;
  if (ctx->buf[slot].ensure(count * sizeof(double))) return fail(SOCP_E_NOMEM, "device allocation failed");
  HIPCHK(hipMemsetAsync(ctx->buf[slot].p, 0, count * sizeof(double), ctx->stream));
  *o = (const double*)ctx->buf[slot].p;
  return 0;
}

}  // namespace

extern "C" int socp_batch_centre(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                 const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm,
                                 const double* c, const double* A, const double* b, const double* G,
                                 const double* h, const uint8_t* sing, int32_t steps, int32_t flags, double* x,
                                 double* y, double* z, double* s, int32_t* status, double* res) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  TRY(check_flags(flags, "socp_batch_centre"));
  if (steps < 0 || steps > CENTRE_MAX_STEPS) return fail(SOCP_E_INVALID, "socp_batch_centre: steps must be 0..16");
  CentreArgs a;
  memset(&a, 0, sizeof(a));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree));
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B == 0) return 0;
  if (!c || !G || !h || !x || !z || !s || !status || (m > 0 && (!A || !b || !y)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  const SmallVariant* v = nullptr;
  TRY(choose_engine(*dims, flags, Pm ? KIND_QP_KKT : KIND_KKT, &v));
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const size_t MB = (flags & SOCP_F_SHARED_MATRICES) ? 1 : (size_t)B;
  a.n = n;
  a.m = m;
  a.k = k;
  a.nc = dims->ncones;
  a.deg = degree;
  a.shared = MB == 1 && (flags & SOCP_F_SHARED_MATRICES) ? 1 : 0;
  typedef socp_ctx X;
  const uint8_t* singd = nullptr;
  TRY(st.in(X::B_P, Pm, MB * n * n, &a.P));
  TRY(st.in(X::B_EC, c, (size_t)B * n, &a.c));
  TRY(st.in(X::B_A, m > 0 ? A : nullptr, MB * m * n, &a.A));
  TRY(st.in(X::B_B, m > 0 ? b : nullptr, (size_t)B * m, &a.b));
  TRY(st.in(X::B_G, G, MB * k * n, &a.G));
  TRY(st.in(X::B_H, h, (size_t)B * k, &a.h));
  TRY(st.in(X::B_SING, sing, MB, &singd));
  TRY(st.out(X::B_X, x, (size_t)B * n, true, &a.x));
  TRY(st.out(X::B_Y, m > 0 ? y : nullptr, (size_t)B * m, true, &a.y));
  TRY(st.out(X::B_Z, z, (size_t)B * k, true, &a.z));
  TRY(st.out(X::B_S, s, (size_t)B * k, true, &a.s));
  TRY(st.out(X::B_ST, status, (size_t)B, false, &a.status));
  TRY(st.out(X::B_RES, res, (size_t)B * 4, false, &a.res));
  HIPCHK(hipMemsetAsync(a.status, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  // the right-hand side, the step and the KKT status: context buffers with device pointers too
  const int rslot[8] = {X::B_DX, X::B_DY, X::B_DZ, X::B_DS, X::B_CX, X::B_CY, X::B_CZ, X::B_CS};
  const size_t rcnt[8] = {(size_t)B * n, (size_t)B * m, (size_t)B * k, (size_t)B * k,
                          (size_t)B * n, (size_t)B * m, (size_t)B * k, (size_t)B * k};
  double* r[8];
  for (int i = 0; i < 8; ++i) {
    TRY(st.reserve(rslot[i], rcnt[i] * sizeof(double)));
    r[i] = rcnt[i] ? (double*)ctx->buf[rslot[i]].p : nullptr;
  }
  TRY(st.reserve(X::B_VST, (size_t)B * sizeof(int32_t)));
  int32_t* kst = (int32_t*)ctx->buf[X::B_VST].p;
  a.dx = r[0];
  a.dy = r[1];
  a.dz = r[2];
  a.ds = r[3];
  a.kst = kst;
  for (int it = 0; it < steps; ++it) {
    a.cx = nullptr;
    HIPCHK(centre_rhs_launch(a, B, ctx->stream));
    TRY(socp_batch_kkt_solve_qp(ctx, dims, cone_kind, cone_offs, cone_dim, a.P, a.A, a.G, singd, a.s, a.z, a.dx, a.dy,
                                a.dz, a.ds, r[4], r[5], r[6], r[7], kst,
                                SOCP_F_DEVICE_PTRS | (flags & kKktFlags)));
    a.cx = r[4];
    a.cy = r[5];
    a.cz = r[6];
    a.cs = r[7];
    if (it == steps - 1) {
      // The last pass refines its step once on the three linear rows: the kernels' solve leaves them a residual
      // of its own accuracy times the step, and the point returned should satisfy them to rounding.  Same
      // (s, z), so the same factorisation and status; the right-hand side is the residual and ds = 0.
      const int eslot[4] = {X::B_EA, X::B_EB, X::B_EG, X::B_EH};
      double* e[4];
      for (int i = 0; i < 4; ++i) {
        TRY(st.reserve(eslot[i], rcnt[i] * sizeof(double)));
        e[i] = rcnt[i] ? (double*)ctx->buf[eslot[i]].p : nullptr;
      }
      HIPCHK(centre_refine_launch(a, B, ctx->stream));
      HIPCHK(hipMemsetAsync(a.ds, 0, rcnt[3] * sizeof(double), ctx->stream));
      TRY(socp_batch_kkt_solve_qp(ctx, dims, cone_kind, cone_offs, cone_dim, a.P, a.A, a.G, singd, a.s, a.z, a.dx,
                                  a.dy, a.dz, a.ds, e[0], e[1], e[2], e[3], kst,
                                  SOCP_F_DEVICE_PTRS | (flags & kKktFlags)));
      HIPCHK(centre_add_launch(a, e[0], e[1], e[2], e[3], B, ctx->stream));
    }
    HIPCHK(centre_update_launch(a, B, it == steps - 1, ctx->stream));
  }
  if (steps == 0 && a.res) {  // no step: res at the inputs
    a.cx = nullptr;
    HIPCHK(centre_update_launch(a, B, true, ctx->stream));
  }
  TRY(st.back(x, a.x, (size_t)B * n));
  TRY(st.back(m > 0 ? y : nullptr, a.y, (size_t)B * m));
  TRY(st.back(z, a.z, (size_t)B * k));
  TRY(st.back(s, a.s, (size_t)B * k));
  TRY(st.back(status, a.status, (size_t)B));
  TRY(st.back(res, a.res, (size_t)B * 4));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

namespace {

// Both adjoint entries after their flag checks.  `sum`: dP, dA and dG are ONE matrix each, the
// sums over the batch (socp_batch_vjp_sum); the per-problem path is launched as without it.
int vjp_run(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind, const int32_t* cone_offs,
            const int32_t* cone_dim, const double* Pm, const double* A, const double* G, const uint8_t* sing,
            const double* x, const double* y, const double* z, const double* s, const double* gx, const double* gy,
            const double* gz, const double* gs, const int32_t* skip, int32_t flags, double* dc, double* db,
            double* dh, double* dP, double* dA, double* dG, double* ux, double* uy, double* uz, int32_t* status,
            bool sum) {
  ConeTable cones;
  memset(&cones, 0, sizeof(cones));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &cones, &degree));
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B == 0) return 0;
  if (!G || !x || !z || !s || !status || (m > 0 && (!A || !y))) return fail(SOCP_E_INVALID, "NULL data pointer");
  const SmallVariant* v = nullptr;
  TRY(choose_engine(*dims, flags, Pm ? KIND_QP_KKT : KIND_KKT, &v));
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const size_t MB = (flags & SOCP_F_SHARED_MATRICES) ? 1 : (size_t)B;
  const size_t Bn = (size_t)B * n, Bm = (size_t)B * m, Bk = (size_t)B * k;
  VjpArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.m = m;
  a.k = k;
  a.shared = (flags & SOCP_F_SHARED_MATRICES) ? 1 : 0;
  typedef socp_ctx X;
  const double *Pd = nullptr, *Ad = nullptr, *sd = nullptr, *gyd = nullptr, *gzd = nullptr;
  const uint8_t* singd = nullptr;
  TRY(st.in(X::B_P, Pm, MB * n * n, &Pd));
  TRY(st.in(X::B_A, m > 0 ? A : nullptr, MB * m * n, &Ad));
  TRY(st.in(X::B_G, G, MB * k * n, &a.G));
  TRY(st.in(X::B_SING, sing, MB, &singd));
  TRY(st.in(X::B_X, x, Bn, &a.x));
  TRY(st.in(X::B_Y, m > 0 ? y : nullptr, Bm, &a.y));
  TRY(st.in(X::B_Z, z, Bk, &a.z));
  TRY(st.in(X::B_S, s, Bk, &sd));
  TRY(st.in(X::B_EC, gx, Bn, &a.gx));
  TRY(st.in(X::B_EB, m > 0 ? gy : nullptr, Bm, &gyd));
  TRY(st.in(X::B_EH, gz, Bk, &gzd));
  TRY(st.in(X::B_RES, gs, Bk, &a.gs));
  TRY(st.in(X::B_IT, skip, (size_t)B, &a.skip));
  TRY(st.out(X::B_ST, status, (size_t)B, false, &a.status));
  // dP, dA, dG: per problem, written by vjp_assemble; or the batch's one, written by vjp_sum_combine
  const size_t GB = sum ? 1 : (size_t)B;
  double *dPd = nullptr, *dAd = nullptr, *dGd = nullptr;
  TRY(st.out(X::B_EP, dP, GB * n * n, false, &dPd));
  TRY(st.out(X::B_EA, m > 0 ? dA : nullptr, GB * m * n, false, &dAd));
  TRY(st.out(X::B_EG, dG, GB * k * n, false, &dGd));
  if (!sum) {
    a.dP = dPd;
    a.dA = dAd;
    a.dG = dGd;
  }
  // the six vector outputs: with host pointers, one run of the staging buffer each
  double* const vuser[6] = {dc, m > 0 ? db : nullptr, dh, ux, m > 0 ? uy : nullptr, uz};
  const size_t vcnt[6] = {Bn, Bm, Bk, Bn, Bm, Bk};
  double* vdev[6];
  {
    size_t total = 0;
    for (int i = 0; i < 6; ++i) total += vuser[i] ? vcnt[i] : 0;
    if (!dev && total) TRY(st.reserve(X::B_VOUT, total * sizeof(double)));
    size_t off = 0;
    for (int i = 0; i < 6; ++i) {
      vdev[i] = vuser[i];
      if (dev || !vuser[i]) continue;
      vdev[i] = (double*)ctx->buf[X::B_VOUT].p + off;
      off += vcnt[i];
    }
  }
  a.dc = vdev[0];
  a.db = vdev[1];
  a.dh = vdev[2];
  a.oux = vdev[3];
  a.ouy = vdev[4];
  a.ouz = vdev[5];
  // the right-hand side (gx - G'gs, gy, gz, 0), the solution and its status
  TRY(st.reserve(X::B_DX, Bn * sizeof(double)));
  a.rx = (double*)ctx->buf[X::B_DX].p;
  if (!gyd) TRY(zeros(ctx, X::B_DY, Bm, &gyd));
  if (!gzd) TRY(zeros(ctx, X::B_DZ, Bk, &gzd));
  const double* zero_ds = nullptr;
  TRY(zeros(ctx, X::B_DS, Bk, &zero_ds));
  const int uslot[4] = {X::B_CX, X::B_CY, X::B_CZ, X::B_CS};
  const size_t ucnt[4] = {Bn, Bm, Bk, Bk};
  double* u[4];
  for (int i = 0; i < 4; ++i) {
    TRY(st.reserve(uslot[i], ucnt[i] * sizeof(double)));
    u[i] = ucnt[i] ? (double*)ctx->buf[uslot[i]].p : nullptr;
  }
  TRY(st.reserve(X::B_VST, (size_t)B * sizeof(int32_t)));
  int32_t* kst = (int32_t*)ctx->buf[X::B_VST].p;
  HIPCHK(vjp_rhs_launch(a, B, ctx->stream));
  TRY(socp_batch_kkt_solve_qp(ctx, dims, cone_kind, cone_offs, cone_dim, Pd, Ad, a.G, singd, sd, a.z, a.rx, gyd, gzd,
                              zero_ds, u[0], u[1], u[2], u[3], kst, SOCP_F_DEVICE_PTRS | (flags & kKktFlags)));
  a.ux = u[0];
  a.uy = u[1];
  a.uz = u[2];
  a.kst = kst;
  HIPCHK(vjp_assemble_launch(a, B, ctx->stream));
  if (sum && (dPd || dAd || dGd)) {
    // the partials' size and the slab rule depend on (B, n, m, k) alone, not on which sums are asked for
    VjpSumArgs q;
    memset(&q, 0, sizeof(q));
    q.x = a.x;
    q.y = a.y;
    q.z = a.z;
    q.ux = u[0];
    q.uy = u[1];
    q.uz = u[2];
    q.gs = a.gs;
    q.status = a.status;
    q.dP = dPd;
    q.dA = dAd;
    q.dG = dGd;
    q.B = B;
    q.n = n;
    q.m = m;
    q.k = k;
    vjp_sum_plan(B, n, m, k, &q.slabs, &q.slab);
    TRY(st.reserve(X::B_VSUM, (size_t)q.slabs * ((size_t)k + m + n) * n * sizeof(double)));
    q.part = (double*)ctx->buf[X::B_VSUM].p;
    HIPCHK(vjp_sum_partial_launch(q, ctx->stream));
    HIPCHK(vjp_sum_combine_launch(q, ctx->stream));
  }
  for (int i = 0; i < 6; ++i) TRY(st.back(vuser[i], vdev[i], vcnt[i]));
  TRY(st.back(dP, dPd, GB * n * n));
  TRY(st.back(m > 0 ? dA : nullptr, dAd, GB * m * n));
  TRY(st.back(dG, dGd, GB * k * n));
  TRY(st.back(status, a.status, (size_t)B));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace

extern "C" int socp_batch_vjp(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                              const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm, const double* A,
                              const double* G, const uint8_t* sing, const double* x, const double* y,
                              const double* z, const double* s, const double* gx, const double* gy,
                              const double* gz, const double* gs, const int32_t* skip, int32_t flags, double* dc,
                              double* db, double* dh, double* dP, double* dA, double* dG, double* ux, double* uy,
                              double* uz, int32_t* status) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  TRY(check_flags(flags, "socp_batch_vjp"));
  if ((flags & SOCP_F_SHARED_MATRICES) && (dP || dA || dG))
    return fail(SOCP_E_UNSUPPORTED,
                "socp_batch_vjp: dP, dA and dG with SOCP_F_SHARED_MATRICES are sums over the batch, which this "
                "entry does not form (socp_batch_vjp_sum does)");
  return vjp_run(ctx, dims, cone_kind, cone_offs, cone_dim, Pm, A, G, sing, x, y, z, s, gx, gy, gz, gs, skip, flags,
                 dc, db, dh, dP, dA, dG, ux, uy, uz, status, false);
}

extern "C" int socp_batch_vjp_sum(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                  const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm,
                                  const double* A, const double* G, const uint8_t* sing, const double* x,
                                  const double* y, const double* z, const double* s, const double* gx,
                                  const double* gy, const double* gz, const double* gs, const int32_t* skip,
                                  int32_t flags, double* dc, double* db, double* dh, double* dP, double* dA,
                                  double* dG, double* ux, double* uy, double* uz, int32_t* status) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  TRY(check_flags(flags, "socp_batch_vjp_sum"));
  if (!(flags & SOCP_F_SHARED_MATRICES))
    return fail(SOCP_E_INVALID, "socp_batch_vjp_sum: SOCP_F_SHARED_MATRICES must be set (dP, dA and dG are the "
                                "gradients of the batch's one P, A and G)");
  return vjp_run(ctx, dims, cone_kind, cone_offs, cone_dim, Pm, A, G, sing, x, y, z, s, gx, gy, gz, gs, skip, flags,
                 dc, db, dh, dP, dA, dG, ux, uy, uz, status, true);
}

extern "C" int socp_debug_vjp_sum_plan(const socp_dims* dims, int64_t* slabs, int64_t* slab_problems) {
  if (!dims || !slabs || !slab_problems) return fail(SOCP_E_INVALID, "socp_debug_vjp_sum_plan: NULL pointer");
  if (dims->batch < 1 || dims->batch > kMaxBatch || dims->n < 1 || dims->m < 0 || dims->k < 1)
    return fail(SOCP_E_INVALID, "socp_debug_vjp_sum_plan: batch, n and k must be at least 1 and m at least 0");
  vjp_sum_plan(dims->batch, dims->n, dims->m, dims->k, slabs, slab_problems);
  return 0;
}
