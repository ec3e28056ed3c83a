// socp_api_sqr.hip — the rank-update handles (socp_sqr_*): setup_iter and
// solve_kkt on socp_sqr.hip's kernels, and socp_sqr_solve_socp, the host-driven
// IPM over them (socp_sqr_ipm.hip).  Host code only.
#include "socp_host.hpp"
#include "socp_sqr.hpp"

using namespace socp;
using namespace socp::host;

// SparseSolver (spsolver.jl:1-130) with SqrScaling (sqrscalings.jl): the
// handle keeps A, G (and sing) on the device, setup_iter computes W^-2 =
// D + uu' - vv', factors G'DG (+A'A), applies the rank-1 modifications and
// factors S into one record per problem; solve_kkt solves against it
// (socp_sqr.hip).
struct socp_sqr {
  socp_ctx* ctx = nullptr;
  SqrArgs a;
  SqrLayout L;
  size_t lds = 0;
  bool dev = false, ready = false;
  int64_t h2d_bytes = 0;
  int deg = 0;  // deg(cones) (vectors.jl:165-179), for mu = lam'lam / deg in solve_socp
  enum { Q_A, Q_G, Q_SING, Q_REC, Q_S, Q_Z, Q_DX, Q_DY, Q_DZ, Q_DS, Q_CX, Q_CY, Q_CZ, Q_CS, Q_ST, Q_OUT,
         Q_IPM, NQB };
  DevBuf buf[NQB];
};

static bool sqr_fits(const socp_dims* d, size_t* lds) {
  if (d->n < 0 || d->m < 0 || d->k < 0 || d->n > SQR_LMAX || d->m > SQR_LMAX || d->k > SQR_KMAX) return false;
  const size_t bytes = (size_t)sqr_layout(d->n, d->m, d->k, d->ncones).total * sizeof(double);
  if (lds) *lds = bytes;
  return bytes <= 160 * 1024;
}

extern "C" int socp_sqr_supported(const socp_dims* d) { return d && sqr_fits(d, nullptr) ? 1 : 0; }

extern "C" int socp_sqr_create(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                               const int32_t* cone_offs, const int32_t* cone_dim, const double* A,
                               const double* G, const uint8_t* sing, int32_t flags, socp_sqr** out) {
  if (!out) return fail(SOCP_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  socp_sqr* h = new socp_sqr();
  h->ctx = ctx;
  SqrArgs& a = h->a;
  memset(&a, 0, sizeof(a));
  auto bail = [&](int rc) {
    handle_free(h);
    return rc;
  };
  int degree = 0;
  int rc = check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree);
  if (rc) return bail(rc);
  h->deg = degree;
  if (!sqr_fits(dims, &h->lds))
    return bail(fail(SOCP_E_UNSUPPORTED, "rank-update plugin: n, m <= 1024, k <= 4096, LDS layout <= 160 KiB (socp_sqr.hip)"));
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B > 0 && (!G || (m > 0 && !A))) return bail(fail(SOCP_E_INVALID, "NULL data pointer"));
  if (hipSetDevice(ctx->device) != hipSuccess) return bail(fail(SOCP_E_HIP, "hipSetDevice"));
  h->dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  a.shared = (flags & SOCP_F_SHARED_MATRICES) ? 1 : 0;
  const size_t MB = a.shared ? 1 : (size_t)B;  // one A, G, sing for the batch
  a.B = B;
  a.n = n;
  a.m = m;
  a.k = k;
  a.nc = dims->ncones;
  h->L = sqr_layout(n, m, k, a.nc);
  if (B == 0) {
    *out = h;
    return 0;
  }
  typedef socp_sqr Q;
  const Stager st{h->buf, ctx->stream, h->dev, &h->h2d_bytes};
  if ((rc = st.own(Q::Q_A, A, MB * m * n * sizeof(double)))) return bail(rc);
  if ((rc = st.own(Q::Q_G, G, MB * k * n * sizeof(double)))) return bail(rc);
  if ((rc = st.own(Q::Q_SING, sing, MB))) return bail(rc);
  a.A = m > 0 ? (const double*)h->buf[Q::Q_A].p : nullptr;
  a.G = (const double*)h->buf[Q::Q_G].p;
  a.sing = sing ? (const uint8_t*)h->buf[Q::Q_SING].p : nullptr;
  if (h->buf[Q::Q_REC].ensure((size_t)B * (size_t)h->L.rec * sizeof(double)))
    return bail(fail(SOCP_E_NOMEM, "factor record allocation failed"));
  a.rec = (double*)h->buf[Q::Q_REC].p;
  // the setup kernels write only the factors' lower triangles
  if (hipMemsetAsync(a.rec, 0, (size_t)B * (size_t)h->L.rec * sizeof(double), ctx->stream) != hipSuccess)
    return bail(fail(SOCP_E_HIP, "hipMemsetAsync"));
  const void* kerns[2] = {sqr_setup_kernel_ptr(n, m), sqr_solve_kernel_ptr(n, m)};
  for (const void* kern : kerns)
    if (h->lds > 64 * 1024 &&
        hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess)
      return bail(fail(SOCP_E_HIP, "hipFuncSetAttribute"));
  // host sources may be pageable temporaries the caller frees on return
  if (!h->dev && hipStreamSynchronize(ctx->stream) != hipSuccess)
    return bail(fail(SOCP_E_HIP, "hipStreamSynchronize"));
  *out = h;
  return 0;
}

extern "C" int socp_sqr_destroy(socp_sqr* h) {
  handle_free(h);
  return 0;
}

static int sqr_launch(socp_sqr* h, const SqrArgs& a, bool setup, bool timed = true) {
  socp_ctx* ctx = h->ctx;
  const void* kern = setup ? sqr_setup_kernel_ptr(a.n, a.m) : sqr_solve_kernel_ptr(a.n, a.m);
  SqrArgs la = a;
  la.stamps = diag_stamps();
  void* kargs[] = {&la};
  if (timed) HIPCHK(timing_begin(ctx));
  const int nt = sqr_block_threads(a.n, a.m);
  size_t lds = h->lds;
  if (!setup && nt == 64) {  // the wave solve kernel's own layout (sqr_solve_layout)
    const SqrLayout Ls = sqr_solve_layout(a.n, a.m, a.k, a.nc);
    if (!Ls.large) lds = (size_t)Ls.total * sizeof(double);
  }
  HIPCHK(hipLaunchKernel(kern, dim3((unsigned)a.B), dim3(nt), kargs, lds, ctx->stream));
  if (timed) HIPCHK(timing_end(ctx));
  ctx->last_name = nt > 64 ? (setup ? "socp_sqr_setup_wg_kernel" : "socp_sqr_solve_wg_kernel")
                           : (setup ? "socp_sqr_setup_kernel" : "socp_sqr_solve_kernel");
  return 0;
}

extern "C" int socp_sqr_setup_iter(socp_sqr* h, const double* s, const double* z, int32_t* status) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  h->h2d_bytes = 0;
  SqrArgs a = h->a;
  const int64_t B = a.B;
  if (B == 0) {
    h->ready = true;
    return 0;
  }
  if (!s || !z || !status) return fail(SOCP_E_INVALID, "NULL data pointer");
  socp_ctx* ctx = h->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const Stager st{h->buf, ctx->stream, h->dev, &h->h2d_bytes};
  typedef socp_sqr Q;
  const size_t k = (size_t)a.k;
  TRY(st.in(Q::Q_S, s, (size_t)B * k, &a.s));
  TRY(st.in(Q::Q_Z, z, (size_t)B * k, &a.z));
  TRY(st.out(Q::Q_ST, status, (size_t)B, false, &a.status));
  TRY(sqr_launch(h, a, true));
  TRY(st.back(status, a.status, (size_t)B));
  if (!h->dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  h->ready = true;
  return 0;
}

extern "C" int socp_sqr_solve_kkt(socp_sqr* h, const double* dx, const double* dy, const double* dz,
                                  const double* ds, double* cx, double* cy, double* cz, double* cs,
                                  int32_t* status) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  if (!h->ready) return fail(SOCP_E_INVALID, "solve_kkt before setup_iter");
  h->h2d_bytes = 0;
  SqrArgs a = h->a;
  const int64_t B = a.B;
  if (B == 0) return 0;
  const int n = a.n, m = a.m, k = a.k;
  if (!dx || !dz || !ds || !cx || !cz || !cs || !status || (m > 0 && (!dy || !cy)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  socp_ctx* ctx = h->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const Stager st{h->buf, ctx->stream, h->dev, &h->h2d_bytes};
  typedef socp_sqr Q;
  TRY(st.in(Q::Q_DX, dx, (size_t)B * n, &a.dx));
  TRY(st.in(Q::Q_DY, dy, (size_t)B * m, &a.dy));
  TRY(st.in(Q::Q_DZ, dz, (size_t)B * k, &a.dz));
  TRY(st.in(Q::Q_DS, ds, (size_t)B * k, &a.ds));
  TRY(st.out(Q::Q_CX, cx, (size_t)B * n, false, &a.cx));
  TRY(st.out(Q::Q_CY, cy, (size_t)B * m, false, &a.cy));
  TRY(st.out(Q::Q_CZ, cz, (size_t)B * k, false, &a.cz));
  TRY(st.out(Q::Q_CS, cs, (size_t)B * k, false, &a.cs));
  TRY(st.out(Q::Q_ST, status, (size_t)B, false, &a.status));
  TRY(sqr_launch(h, a, false));
  TRY(st.back(cx, a.cx, (size_t)B * n));
  TRY(st.back(cy, a.cy, (size_t)B * m));
  TRY(st.back(cz, a.cz, (size_t)B * k));
  TRY(st.back(cs, a.cs, (size_t)B * k));
  TRY(st.back(status, a.status, (size_t)B));
  if (!h->dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// solve_socp(prob, SolverState(prob, SparseSolver(prob))) (solver.jl:40-153)
// for the handle's whole batch: the initial point, then up to maxit iterations
// of setup_iter + two solve_kkt with this plugin, every problem masked out of
// the launches once it stops (socp_sqr_ipm.hip).  c, b, h in; x, y, z, s,
// iters, status (and res: ||rd||, ||rp||, z's at the returned iterate, may be
// NULL) out; host or device pointers as the handle's flags say.
#ifndef SQR_FUSE_RESID
#define SQR_FUSE_RESID 1  // 0: the separate residual kernel after every setup launch (A/B builds)
#endif
#ifndef SQR_FUSE_SOLVES
#define SQR_FUSE_SOLVES 1  // the iteration's two solves and step phases in one launch (0: four launches)
#endif
extern "C" int socp_sqr_solve_socp(socp_sqr* h, const double* c, const double* b, const double* hv,
                                   const socp_params* params, double* x, double* y, double* z, double* s,
                                   int32_t* iters, int32_t* status, double* res) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  const int64_t B = h->a.B;
  if (B == 0) return 0;
  const int n = h->a.n, m = h->a.m, k = h->a.k;
  if (!c || !hv || !x || !z || !s || !iters || !status || (m > 0 && (!b || !y)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  const socp_params P = params_or_default(params);
  if (P.maxit < 0) return fail(SOCP_E_INVALID, "maxit < 0");
  TRY(check_detect_flags(P.flags));
  TRY(check_no_equilibrate(P.flags, "socp_sqr_solve_socp"));
  if (sqr_ipm_lds_bytes(n, m, k) > 160 * 1024)
    return fail(SOCP_E_UNSUPPORTED, "socp_sqr_solve_socp: the IPM kernels' vectors (7 k + n + m doubles) exceed 160 KiB");
  socp_ctx* ctx = h->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  h->h2d_bytes = 0;
  const Stager st{h->buf, ctx->stream, h->dev, &h->h2d_bytes};
  // device block: c b h | x y z s | dx dy dz ds | rx ry rz rs | res | status iters active st_setup st_solve
  const size_t nd = (size_t)B * (n + m + k) + 4 * (size_t)B * (n + m + 2 * k) + 3 * (size_t)B;
  const size_t ni = 5 * (size_t)B + 1;
  typedef socp_sqr Q;
  TRY(st.reserve(Q::Q_IPM, nd * sizeof(double) + ni * sizeof(int32_t)));
  double* d = (double*)h->buf[Q::Q_IPM].p;
  SqrIpmArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.B = B; ia.n = n; ia.m = m; ia.k = k; ia.nc = h->a.nc; ia.deg = h->deg; ia.sigma_exp = P.sigma_exp;
  ia.cones = h->a.cones;
  ia.A = h->a.A; ia.G = h->a.G; ia.shared = h->a.shared;
  double* dc = d;
  double* db = dc + (size_t)B * n;
  double* dh = db + (size_t)B * m;
  double* q = dh + (size_t)B * k;
  auto carve4 = [&](double** o0, double** o1, double** o2, double** o3) {
    *o0 = q; q += (size_t)B * n;
    *o1 = q; q += (size_t)B * m;
    *o2 = q; q += (size_t)B * k;
    *o3 = q; q += (size_t)B * k;
  };
  carve4(&ia.x, &ia.y, &ia.z, &ia.s);
  carve4(&ia.dx, &ia.dy, &ia.dz, &ia.ds);
  carve4(&ia.rx, &ia.ry, &ia.rz, &ia.rs);
  ia.res = q; q += 3 * (size_t)B;
  int32_t* ip = (int32_t*)q;
  ia.status = ip; ia.iters = ip + B; ia.active = ip + 2 * B; ia.st_setup = ip + 3 * B;
  int32_t* st_solve = ip + 4 * B;
  ia.n_active = ip + 5 * B;
  // the active count starts at B, set on the stream (no host round trip)
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ia.n_active, (int)B, 1, ctx->stream));
  const bool dev = h->dev;
  if (dev) {
    ia.c = c; ia.b = m ? b : nullptr; ia.h = hv;
  } else {
    HIPCHK(hipMemcpyAsync(dc, c, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (m) HIPCHK(hipMemcpyAsync(db, b, (size_t)B * m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dh, hv, (size_t)B * k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    h->h2d_bytes += (int64_t)((size_t)B * (n + m + k) * sizeof(double));
    ia.c = dc; ia.b = db; ia.h = dh;
  }
  ia.rec = h->a.rec; ia.rec_stride = h->L.rec; ia.r_l = h->L.r_l; ia.r_wb = h->L.r_wb; ia.r_mu = h->L.r_mu;
  ia.tol = P.tol; ia.step = P.step; ia.init_eps = P.init_eps;
  ia.detect = (P.flags & SOCP_F_DETECT_INFEASIBLE) != 0;
  ia.itol = ctx->itol;
  // the plugin's own launches on the IPM's buffers
  SqrArgs su = h->a;  // setup_iter(s, z)
  su.s = ia.s; su.z = ia.z; su.status = ia.st_setup; su.active = nullptr;
  SqrArgs sv = h->a;  // solve_kkt(dx, dy, dz, ds) -> (rx, ry, rz, rs)
  sv.dx = ia.dx; sv.dy = ia.dy; sv.dz = ia.dz; sv.ds = ia.ds;
  sv.cx = ia.rx; sv.cy = ia.ry; sv.cz = ia.rz; sv.cs = ia.rs; sv.status = st_solve; sv.active = nullptr;
  const size_t lds = sqr_ipm_lds_bytes(n, m, k);
  if (lds > 64 * 1024) {
    // above the default 64 KiB of dynamic LDS every IPM kernel has to opt in,
    // as sqr_create does for the setup / solve kernels
    for (int which = 0; which < 6; ++which)
      HIPCHK(hipFuncSetAttribute(sqr_ipm_kernel_ptr(which), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const dim3 grid((unsigned)B), blk(64);
  auto ipm = [&](int which, int it) -> int {
    void* args1[] = {&ia};
    void* args2[] = {&ia, &it};
    HIPCHK(hipLaunchKernel(sqr_ipm_kernel_ptr(which), grid, blk, which == 4 ? args2 : args1, lds, ctx->stream));
    return 0;
  };
  HIPCHK(timing_begin(ctx));
  // initial point: the KKT system with W = I (s = z = e), then the shift
  TRY(ipm(0, 0));
  TRY(sqr_launch(h, su, true, false));
  sv.init = 1;
  TRY(sqr_launch(h, sv, false, false));
  sv.init = 0;
  TRY(ipm(1, 0));
  su.active = ia.active;
  sv.active = ia.active;
  // the wavefront setup kernel computes the residuals in its pass over G and
  // takes the resid kernel's exit test and right-hand side (SqrArgs::fuse_resid)
  const bool fuse = !h->L.large && SQR_FUSE_RESID;
  if (fuse) {
    su.fuse_resid = 1;
    su.ix = ia.x; su.iy = ia.y; su.ic = ia.c; su.ib = ia.b; su.ih = ia.h;
    su.odx = ia.dx; su.ody = ia.dy; su.odz = ia.dz; su.ods = ia.ds; su.ores = ia.res;
    su.ostatus = ia.status; su.oactive = ia.active; su.n_active = ia.n_active;
    su.tol = P.tol;
    su.detect = ia.detect; su.itol = ia.itol;
    su.ux = ia.x; su.uy = ia.y; su.uz = ia.z; su.us = ia.s;
  }
  // the wave shapes run the two solves and both step phases in one launch
  const void* solves = SQR_FUSE_SOLVES ? sqr_ipm_solves_kernel_ptr(n, m) : nullptr;
  size_t solves_lds = 0;
  if (solves) {
    const SqrLayout Ls = sqr_solve_layout(n, m, k, h->a.nc);
    solves_lds = (size_t)Ls.total * sizeof(double);
    if (lds > solves_lds) solves_lds = lds;
    if (solves_lds > 160 * 1024) {
      solves = nullptr;
    } else if (solves_lds > 64 * 1024) {
      HIPCHK(hipFuncSetAttribute(solves, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solves_lds));
    }
  }
  for (int it = 0; it < P.maxit; ++it) {
    TRY(sqr_launch(h, su, true, false));   // compute_scaling + setup_iter (+ fused: the residuals)
    if (!fuse) TRY(ipm(2, it));            // residuals, exit test, affine right-hand side
    if (solves) {
      SqrArgs sl = sv;
      sl.stamps = diag_stamps();
      int itv = it;
      void* fargs[] = {&sl, &ia, &itv};
      HIPCHK(hipLaunchKernel(solves, grid, blk, fargs, solves_lds, ctx->stream));
    } else {
      TRY(sqr_launch(h, sv, false, false));  // solve_kkt (affine)
      TRY(ipm(3, it));                       // step, sigma, mu, corrector right-hand side
      TRY(sqr_launch(h, sv, false, false));  // solve_kkt (combined)
      TRY(ipm(4, it));                       // step and update
    }
    // under a stopping rule, look every 4 iterations whether any problem is
    // still iterating: the launches over an all-stopped batch are skipped
    if (P.tol > 0.0 && (it & 3) == 3 && it + 1 < P.maxit) {
      int32_t left = 0;
      HIPCHK(hipMemcpyAsync(&left, ia.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      if (left <= 0) break;
    }
  }
  if (res) TRY(ipm(5, 0));
  HIPCHK(timing_end(ctx));
  ctx->last_name = "socp_sqr_solve_socp";
  // the results leave the IPM's block: into the caller's device arrays, or back to the host
  auto give = [&](auto* user, const auto* src, size_t count) -> int {
    if (dev) HIPCHK(hipMemcpyAsync(user, src, count * sizeof(*user), hipMemcpyDeviceToDevice, ctx->stream));
    return st.back(user, src, count);
  };
  TRY(give(x, ia.x, (size_t)B * n));
  if (m) TRY(give(y, ia.y, (size_t)B * m));
  TRY(give(z, ia.z, (size_t)B * k));
  TRY(give(s, ia.s, (size_t)B * k));
  TRY(give(iters, ia.iters, (size_t)B));
  TRY(give(status, ia.status, (size_t)B));
  if (res) TRY(give(res, ia.res, 3 * (size_t)B));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  h->ready = true;  // the records hold the last iteration's factorisation
  return 0;
}

// one problem's factor of H after modify_factors! (n x n, column-major, zeros
// above the diagonal) -- the Gfact of spsolver.jl:13 as a dense matrix
extern "C" int socp_sqr_factor(socp_sqr* h, int64_t problem, double* L) {
  if (!h || !L) return fail(SOCP_E_INVALID, "NULL argument");
  if (!h->ready) return fail(SOCP_E_INVALID, "factor before setup_iter");
  if (problem < 0 || problem >= h->a.B) return fail(SOCP_E_INVALID, "problem index out of range");
  HIPCHK(hipSetDevice(h->ctx->device));
  const double* src = h->a.rec + problem * h->L.rec + h->L.r_L;
  HIPCHK(hipMemcpyAsync(L, src, (size_t)h->a.n * h->a.n * sizeof(double), hipMemcpyDefault, h->ctx->stream));
  HIPCHK(hipStreamSynchronize(h->ctx->stream));
  return 0;
}

// lambda (B x k), wb (B x k) and mu (B x ncones) of the last setup_iter: the
// SqrScaling fields l, wbs, mu (sqrscalings.jl:11-16) the driver loop reads
extern "C" int socp_sqr_scaling(socp_sqr* h, double* l, double* wbs, double* mu) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  if (!h->ready) return fail(SOCP_E_INVALID, "scaling before setup_iter");
  const int64_t B = h->a.B;
  if (B == 0) return 0;
  HIPCHK(hipSetDevice(h->ctx->device));
  const SqrLayout& L = h->L;
  const int k = h->a.k, nc = h->a.nc;
  const size_t pitch = (size_t)L.rec * sizeof(double);
  if (l)
    HIPCHK(hipMemcpy2DAsync(l, k * sizeof(double), h->a.rec + L.r_l, pitch, k * sizeof(double), B,
                            hipMemcpyDefault, h->ctx->stream));
  if (wbs)
    HIPCHK(hipMemcpy2DAsync(wbs, k * sizeof(double), h->a.rec + L.r_wb, pitch, k * sizeof(double), B,
                            hipMemcpyDefault, h->ctx->stream));
  if (mu)
    HIPCHK(hipMemcpy2DAsync(mu, nc * sizeof(double), h->a.rec + L.r_mu, pitch, nc * sizeof(double), B,
                            hipMemcpyDefault, h->ctx->stream));
  HIPCHK(hipStreamSynchronize(h->ctx->stream));
  return 0;
}

extern "C" int socp_sqr_h2d_bytes(const socp_sqr* h, int64_t* bytes) {
  if (!h || !bytes) return fail(SOCP_E_INVALID, "NULL argument");
  *bytes = h->h2d_bytes;
  return 0;
}

extern "C" int64_t socp_sqr_record_bytes(const socp_sqr* h) {
  return h ? h->L.rec * (int64_t)sizeof(double) : 0;
}
