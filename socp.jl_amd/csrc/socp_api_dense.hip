// socp_api_dense.hip — the dense KKT handles (socp_dense_*): A, G and one factor
// record per problem stay on the device; setup_iter and solve_kkt move only
// vectors.  Host code only.
#include "socp_host.hpp"

using namespace socp;
using namespace socp::host;

// The reference's solver plugin split (densesolver.jl): the solver object is
// built once per problem (A, G kept), setup_iter (:41-52) factors for the
// current (s, z), and solve_kkt (:54-90) is called twice per iteration against
// that factorisation.  A handle keeps A, G (and sing) resident and one factor
// record per problem; a setup_iter call moves s, z in and a solve_kkt call one
// right-hand side, so per-call H2D traffic is O(n + m + k) per problem.
struct socp_dense {
  socp_ctx* ctx = nullptr;
  SmallArgs a;  // problem part filled at create
  const SmallVariant* v = nullptr;
  int64_t rec_stride = 0;
  bool qp = false;         // socp_dense_create_qp gave a P: the QP plugin-entry kernels
  bool ready = false;      // setup_iter has run
  int64_t h2d_bytes = 0;   // host-to-device bytes moved by the last call
  enum { D_A, D_G, D_SING, D_P, D_ZERO, D_REC, D_S, D_Z, D_DX, D_DY, D_DZ, D_DS, D_CX, D_CY, D_CZ, D_CS,
         D_ST, D_CNT, ND };
  DevBuf buf[ND];
};

// socp_dense_create, and with Pm != NULL socp_dense_create_qp: P is kept beside A and G
static int dense_create_impl(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                             const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm, const double* A,
                             const double* G, const uint8_t* sing, int32_t flags, socp_dense** out) {
  if (!out) return fail(SOCP_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  const bool qp = Pm != nullptr;
  // (SOCP_F_DETECT_INFEASIBLE is no flag of the plugin entries: ignored, as socp_dense_create ignores it)
  if (qp) TRY(check_qp_flags(flags & ~SOCP_F_DETECT_INFEASIBLE, "socp_dense_create_qp"));
  socp_dense* h = new socp_dense();
  h->ctx = ctx;
  SmallArgs& a = h->a;
  memset(&a, 0, sizeof(a));
  int degree = 0;
  auto bail = [&](int rc) {
    handle_free(h);
    return rc;
  };
  int rc = check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree);
  if (rc) return bail(rc);
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B > 0 && (!G || (m > 0 && !A))) return bail(fail(SOCP_E_INVALID, "NULL data pointer"));
  h->qp = qp;
  if ((rc = choose_engine(*dims, flags, qp ? KIND_QP_KKT : KIND_KKT, &h->v))) return bail(rc);
  if (hipSetDevice(ctx->device) != hipSuccess) return bail(fail(SOCP_E_HIP, "hipSetDevice"));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  fill_args(a, *dims, B, degree, &kKktParams);
  a.flags = flags & (SOCP_F_DEVICE_PTRS | SOCP_F_EXPLICIT_INVERSE | SOCP_F_SHARED_MATRICES);
  if (B == 0) {
    *out = h;
    return 0;
  }
  const size_t MB = (flags & SOCP_F_SHARED_MATRICES) ? 1 : (size_t)B;  // one A, G, sing for the batch
  typedef socp_dense D;
  // the handle owns its copies (the caller's device buffers may be reused)
  const Stager st{h->buf, ctx->stream, dev, &h->h2d_bytes};
  if ((rc = st.own(D::D_A, A, MB * m * n * sizeof(double)))) return bail(rc);
  if ((rc = st.own(D::D_G, G, MB * k * n * sizeof(double)))) return bail(rc);
  if ((rc = st.own(D::D_SING, sing, MB))) return bail(rc);
  if (qp) {
    if ((rc = st.own(D::D_P, Pm, MB * n * n * sizeof(double)))) return bail(rc);
    small_set_qp_plugin(a, (const double*)h->buf[D::D_P].p);
  }
  a.A = m > 0 ? (const double*)h->buf[D::D_A].p : nullptr;
  a.G = (const double*)h->buf[D::D_G].p;
  a.sing = sing ? (const uint8_t*)h->buf[D::D_SING].p : nullptr;
  if ((rc = zero_cbh(h->buf[D::D_ZERO], ctx->stream, a))) return bail(rc);
  h->rec_stride = h->v ? small_rec_doubles(h->v->NQ, h->v->NP, h->v->MQ) : large_layout(n, m, k).r_total;
  if (h->buf[D::D_REC].ensure((size_t)B * (size_t)h->rec_stride * sizeof(double)))
    return bail(fail(SOCP_E_NOMEM, "factor record allocation failed"));
  if ((rc = st.reserve(D::D_CNT, 256))) return bail(rc);
  a.counter = (int32_t*)h->buf[D::D_CNT].p;
  a.rec = (double*)h->buf[D::D_REC].p;
  a.rec_stride = h->rec_stride;
  // host sources may be pageable temporaries the caller frees on return
  if (!dev && hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(fail(SOCP_E_HIP, "hipStreamSynchronize"));
  *out = h;
  return 0;
}

extern "C" int socp_dense_create(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                 const int32_t* cone_offs, const int32_t* cone_dim, const double* A,
                                 const double* G, const uint8_t* sing, int32_t flags, socp_dense** out) {
  return dense_create_impl(ctx, dims, cone_kind, cone_offs, cone_dim, nullptr, A, G, sing, flags, out);
}

extern "C" int socp_dense_create_qp(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                    const int32_t* cone_offs, const int32_t* cone_dim, const double* P,
                                    const double* A, const double* G, const uint8_t* sing, int32_t flags,
                                    socp_dense** out) {
  return dense_create_impl(ctx, dims, cone_kind, cone_offs, cone_dim, P, A, G, sing, flags, out);
}

extern "C" int socp_dense_destroy(socp_dense* h) {
  handle_free(h);
  return 0;
}

static int dense_launch(socp_dense* h, SmallArgs& a) {
  return h->v ? launch_small(h->ctx, a, h->v, h->qp) : launch_large(h->ctx, a, a.rec, h->qp);
}

extern "C" int socp_dense_setup_iter(socp_dense* h, const double* s, const double* z, int32_t* status) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  h->h2d_bytes = 0;
  SmallArgs a = h->a;
  const int64_t B = a.B;
  if (B == 0) {
    h->ready = true;
    return 0;
  }
  if (!s || !z || !status) return fail(SOCP_E_INVALID, "NULL data pointer");
  socp_ctx* ctx = h->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const Stager st{h->buf, ctx->stream, (a.flags & SOCP_F_DEVICE_PTRS) != 0, &h->h2d_bytes};
  typedef socp_dense D;
  const size_t k = (size_t)a.k;
  TRY(st.out(D::D_S, const_cast<double*>(s), (size_t)B * k, true, &a.s));  // read only in MODE_SETUP
  TRY(st.out(D::D_Z, const_cast<double*>(z), (size_t)B * k, true, &a.z));
  TRY(st.out(D::D_ST, status, (size_t)B, false, &a.status));
  a.mode = MODE_SETUP;
  TRY(dense_launch(h, a));
  TRY(st.back(status, a.status, (size_t)B));
  if (!st.dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  h->ready = true;
  return 0;
}

extern "C" int socp_dense_solve_kkt(socp_dense* h, const double* dx, const double* dy, const double* dz,
                                    const double* ds, double* cx, double* cy, double* cz, double* cs,
                                    int32_t* status) {
  if (!h) return fail(SOCP_E_INVALID, "handle is NULL");
  if (!h->ready) return fail(SOCP_E_INVALID, "solve_kkt before setup_iter");
  h->h2d_bytes = 0;
  SmallArgs a = h->a;
  const int64_t B = a.B;
  if (B == 0) return 0;
  const int n = a.n, m = a.m, k = a.k;
  if (!dx || !dz || !ds || !cx || !cz || !cs || !status || (m > 0 && (!dy || !cy)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  socp_ctx* ctx = h->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const Stager st{h->buf, ctx->stream, (a.flags & SOCP_F_DEVICE_PTRS) != 0, &h->h2d_bytes};
  typedef socp_dense D;
  TRY(st.in(D::D_DX, dx, (size_t)B * n, &a.dx));
  TRY(st.in(D::D_DY, dy, (size_t)B * m, &a.dy));
  TRY(st.in(D::D_DZ, dz, (size_t)B * k, &a.dz));
  TRY(st.in(D::D_DS, ds, (size_t)B * k, &a.ds));
  TRY(st.out(D::D_CX, cx, (size_t)B * n, false, &a.cx));
  TRY(st.out(D::D_CY, cy, (size_t)B * m, false, &a.cy));
  TRY(st.out(D::D_CZ, cz, (size_t)B * k, false, &a.cz));
  TRY(st.out(D::D_CS, cs, (size_t)B * k, false, &a.cs));
  TRY(st.out(D::D_ST, status, (size_t)B, false, &a.status));
  a.mode = MODE_SOLVEKKT;
  TRY(dense_launch(h, a));
  TRY(st.back(cx, a.cx, (size_t)B * n));
  TRY(st.back(cy, a.cy, (size_t)B * m));
  TRY(st.back(cz, a.cz, (size_t)B * k));
  TRY(st.back(cs, a.cs, (size_t)B * k));
  TRY(st.back(status, a.status, (size_t)B));
  if (!st.dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int socp_dense_h2d_bytes(const socp_dense* h, int64_t* bytes) {
  if (!h || !bytes) return fail(SOCP_E_INVALID, "NULL argument");
  *bytes = h->h2d_bytes;
  return 0;
}

extern "C" int64_t socp_dense_record_bytes(const socp_dense* h) {
  return h ? h->rec_stride * (int64_t)sizeof(double) : 0;
}
