// socp_api.hip — the core of libsocp's C ABI (include/socp.h): contexts, streams
// and timing, the problem checks, variant dispatch and the two solver launchers,
// the batch solves, equilibration, normalisation and the fused KKT entry.  It defines what
// socp_host.hpp declares for the other units (socp_api_*.hip); host code only.
#include <cstdio>
#include <vector>

#include "socp_equil.hpp"
#include "socp_host.hpp"
#include "socp_norm.hpp"

using namespace socp;
using namespace socp::host;

// the library's one error string: every unit writes it through fail()
static thread_local std::string g_err;
int socp::host::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int Stager::put(int slot, const void* src, size_t bytes, bool copy, hipMemcpyKind kind) const {
  if (bufs[slot].ensure(bytes)) return fail(SOCP_E_NOMEM, "device allocation failed");
  if (!copy) return 0;
  HIPCHK(hipMemcpyAsync(bufs[slot].p, src, bytes, kind, stream));
  if (kind == hipMemcpyHostToDevice && h2d) *h2d += (int64_t)bytes;
  return 0;
}

extern "C" const char* socp_last_error(void) { return g_err.c_str(); }
#ifdef SOCP_DIAG
extern "C" const char* socp_version(void) { return "socp-mi355x 0.1 (gfx950, diagnostic build: phase stamps, KKT dumps)"; }
#else
extern "C" const char* socp_version(void) { return "socp-mi355x 0.1 (gfx950)"; }
#endif

extern "C" void socp_params_default(socp_params* p) {
  p->maxit = 40;
  p->sigma_exp = 3;
  p->tol = 1e-5;
  p->step = 0.99;
  p->init_eps = 1e-10;
  p->flags = 0;
  p->reserved = 0;
}

static void ctx_free(socp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // NULL is the null stream (socp_ctx_set_stream(NULL)): synchronise it too,
  // so no kernel still reads the buffers released below
  (void)hipStreamSynchronize(c->stream);
  if (c->own && c->own != c->stream) (void)hipStreamSynchronize(c->own);
  for (auto& b : c->buf) b.release();
  for (int i = 0; i < socp_ctx::NTIME; ++i) {
    if (c->tev0[i]) (void)hipEventDestroy(c->tev0[i]);
    if (c->tev1[i]) (void)hipEventDestroy(c->tev1[i]);
  }
  if (c->evh) (void)hipEventDestroy(c->evh);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

extern "C" int socp_ctx_create(int device, socp_ctx** out) {
  if (!out) return fail(SOCP_E_INVALID, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(SOCP_E_INVALID, "bad device index");
  HIPCHK(hipSetDevice(device));
  socp_ctx* c = new socp_ctx();
  c->device = device;
  // every partially created resource is released on an error path
  auto bail = [&](hipError_t e, const char* what) {
    ctx_free(c);
    return fail(SOCP_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hipDeviceProp_t prop;
  hipError_t e;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail(e, "hipGetDeviceProperties");
  c->num_cu = prop.multiProcessorCount;
  if ((e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking)) != hipSuccess)
    return bail(e, "hipStreamCreateWithFlags");
  c->stream = c->own;
  for (int i = 0; i < socp_ctx::NTIME; ++i) {
    if ((e = hipEventCreate(&c->tev0[i])) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreate(&c->tev1[i])) != hipSuccess) return bail(e, "hipEventCreate");
  }
  if ((e = hipEventCreateWithFlags(&c->evh, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
  *out = c;
  return 0;
}

extern "C" int socp_ctx_destroy(socp_ctx* c) {
  ctx_free(c);
  return 0;
}

extern "C" int socp_ctx_set_infeasibility_tol(socp_ctx* c, double tol) {
  if (!c) return fail(SOCP_E_INVALID, "ctx is NULL");
  if (!(tol > 0.0)) return fail(SOCP_E_INVALID, "infeasibility tolerance must be positive");  // NaN too
  c->itol = tol;
  return 0;
}

extern "C" int socp_ctx_set_equilibration_passes(socp_ctx* c, int passes) {
  if (!c) return fail(SOCP_E_INVALID, "ctx is NULL");
  if (passes < 1 || passes > 64) return fail(SOCP_E_INVALID, "equilibration passes must be 1..64");
  c->equil_passes = passes;
  return 0;
}

// SOCP_F_EQUILIBRATE or SOCP_F_NORMALISE on an entry that does not scale: refused rather than ignored
int host::check_no_equilibrate(int32_t flags, const char* who) {
  if (flags & SOCP_F_NORMALISE)
    return fail(SOCP_E_UNSUPPORTED, std::string(who) + ": SOCP_F_NORMALISE is honoured by socp_batch_solve, "
                                                       "socp_batch_solve_ex and socp_batch_solve_qp only");
  if (flags & SOCP_F_EQUILIBRATE)
    return fail(SOCP_E_UNSUPPORTED, std::string(who) + ": SOCP_F_EQUILIBRATE is honoured by socp_batch_solve, "
                                                       "socp_batch_solve_ex and socp_batch_solve_qp only");
  return 0;
}

// the flags no QP kernel is compiled for, refused by the QP entry `who` (include/socp.h)
int host::check_qp_flags(int32_t flags, const char* who) {
  if (flags & SOCP_F_EXPLICIT_INVERSE)
    return fail(SOCP_E_UNSUPPORTED, std::string(who) + " with SOCP_F_EXPLICIT_INVERSE: no QP kernel is compiled in the "
                                                       "explicit-inverse operation order");
  if (flags & SOCP_F_DETECT_INFEASIBLE)
    return fail(SOCP_E_UNSUPPORTED, std::string(who) + " with SOCP_F_DETECT_INFEASIBLE: the unboundedness rule would "
                                                       "also need Px = 0, which the detecting kernels do not test");
  return 0;
}

// SOCP_F_DETECT_INFEASIBLE with SOCP_F_EXPLICIT_INVERSE: refused (include/socp.h)
int host::check_detect_flags(int32_t flags) {
  if ((flags & SOCP_F_DETECT_INFEASIBLE) && (flags & SOCP_F_EXPLICIT_INVERSE))
    return fail(SOCP_E_UNSUPPORTED,
                "SOCP_F_DETECT_INFEASIBLE with SOCP_F_EXPLICIT_INVERSE: the iteration at which the rule fires is "
                "not stable in the explicit-inverse operation order");
  return 0;
}

static int ctx_switch_stream(socp_ctx* c, hipStream_t s) {
  if (s == c->stream) return 0;
  // work already queued on the old stream stays ordered before what follows
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->evh, c->stream));
  HIPCHK(hipStreamWaitEvent(s, c->evh, 0));
  c->stream = s;
  return 0;
}

// `stream` is taken literally: NULL is HIP's null (default) stream, which is
// torch's default current stream.
extern "C" int socp_ctx_set_stream(socp_ctx* c, void* stream) {
  if (!c) return fail(SOCP_E_INVALID, "ctx is NULL");
  return ctx_switch_stream(c, (hipStream_t)stream);
}

extern "C" int socp_ctx_reset_stream(socp_ctx* c) {
  if (!c) return fail(SOCP_E_INVALID, "ctx is NULL");
  return ctx_switch_stream(c, c->own);
}

extern "C" int socp_ctx_sync(socp_ctx* c) {
  if (!c) return fail(SOCP_E_INVALID, "ctx is NULL");
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" void* socp_ctx_stream(socp_ctx* c) { return c ? (void*)c->stream : nullptr; }

hipError_t host::timing_begin(socp_ctx* c) {
  return hipEventRecord(c->tev0[c->tlaunches % socp_ctx::NTIME], c->stream);
}
hipError_t host::timing_end(socp_ctx* c) {
  const hipError_t e = hipEventRecord(c->tev1[c->tlaunches % socp_ctx::NTIME], c->stream);
  if (e == hipSuccess) ++c->tlaunches;
  return e;
}

extern "C" int socp_last_kernel_ms(socp_ctx* c, float* ms) {
  if (!c || !ms) return fail(SOCP_E_INVALID, "NULL argument");
  if (c->tlaunches == 0) return fail(SOCP_E_INVALID, "no timed launch on this context");
  const int i = (int)((c->tlaunches - 1) % socp_ctx::NTIME);
  HIPCHK(hipEventSynchronize(c->tev1[i]));
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->tev0[i], c->tev1[i]));
  *ms = c->last_ms;
  return 0;
}

extern "C" int socp_kernel_times(socp_ctx* c, float* ms, int n) {
  if (!c || !ms || n < 0) return fail(SOCP_E_INVALID, "NULL argument or n < 0");
  int64_t cnt = c->tlaunches < n ? c->tlaunches : n;
  if (cnt > socp_ctx::NTIME) cnt = socp_ctx::NTIME;
  if (cnt == 0) return 0;
  for (int64_t j = 0; j < cnt; ++j) {
    const int i = (int)((c->tlaunches - cnt + j) % socp_ctx::NTIME);
    // each pair is waited on: the pairs may lie on different streams when the
    // context's stream was switched inside the window (socp_ctx_set_stream)
    HIPCHK(hipEventSynchronize(c->tev1[i]));
    HIPCHK(hipEventElapsedTime(&ms[j], c->tev0[i], c->tev1[i]));
  }
  c->last_ms = ms[cnt - 1];
  return (int)cnt;
}
extern "C" const char* socp_last_kernel_name(socp_ctx* c) { return c ? c->last_name : ""; }

// ---------------------------------------------------------------- checks
int host::check_problem(const socp_dims* d, const int32_t* kind, const int32_t* offs, const int32_t* dim,
                        ConeTable* tab, int* degree) {
  if (!d) return fail(SOCP_E_INVALID, "dims is NULL");
  if (d->batch < 0 || d->n <= 0 || d->m < 0 || d->k <= 0 || d->ncones <= 0)
    return fail(SOCP_E_INVALID, "bad dims (need batch>=0, n>0, m>=0, k>0, ncones>0)");
  if (d->batch > kMaxBatch)
    return fail(SOCP_E_INVALID, "batch above 2^31-1 (problem indices are int32 on the device)");
  if (d->ncones > MAXC) return fail(SOCP_E_UNSUPPORTED, "too many cones");
  if (!kind || !offs || !dim) return fail(SOCP_E_INVALID, "cone arrays are NULL");
  int next = 0, deg = 0;
  bool seen_soc = false;
  tab->nc = d->ncones;
  for (int c = 0; c < d->ncones; ++c) {
    if (kind[c] != SOCP_CONE_POC && kind[c] != SOCP_CONE_SOC)
      return fail(SOCP_E_INVALID, "cone kind must be POC(0) or SOC(1)");
    if (offs[c] != next || dim[c] <= 0)
      return fail(SOCP_E_INVALID, "cones must be contiguous from 0 with dim>0 (scalings.jl:102)");
    if (kind[c] == SOCP_CONE_POC && seen_soc)
      return fail(SOCP_E_INVALID, "cones must list POC before SOC (scalings.jl:102)");
    if (kind[c] == SOCP_CONE_SOC) seen_soc = true;
    tab->kind[c] = kind[c];
    tab->offs[c] = offs[c];
    tab->dim[c] = dim[c];
    next += dim[c];
    deg += (kind[c] == SOCP_CONE_POC) ? dim[c] : 1;
  }
  if (next != d->k) return fail(SOCP_E_INVALID, "cone dims must sum to k");
  *degree = deg;
  return 0;
}

static const SmallVariant* pick_variant(int n, int m, int k) {
  int cnt = 0;
  const SmallVariant* v = small_variants(&cnt);
  const SmallVariant* best = nullptr;
  long best_cost = 0;
  for (int i = 0; i < cnt; ++i) {
    if (16 * v[i].NQ < n || 4 * v[i].NP < k || 16 * v[i].MQ < (m > 0 ? m : 1)) continue;
    if (k > KMAX) continue;
    long cost = (long)v[i].NQ * v[i].NQ * v[i].NP * 64 + (long)v[i].MQ * 16;
    if (!best || cost < best_cost) {
      best = &v[i];
      best_cost = cost;
    }
  }
  return best;
}

// The blocked kernel (socp_large.hip): n, m <= 2048.  The problem's vectors live in the 160 KiB LDS of a CU when
// they fit; otherwise (e.g. k = 1000 at n = 512) in the workgroup's slot of the
// HBM workspace (*gv: the GV kernels), with only the problem index in LDS.
static bool large_fits(int n, int m, int k, int nc, size_t* lds_bytes, bool* gv = nullptr) {
  // Every LDS / vector offset of the kernel (LargeLayout::o_*, total, LV(int))
  // is a 32-bit int and X = W^-1 G (KP x NPAD) is addressed from int row
  // offsets: bound k before the layout is computed in int, so that neither
  // wraps (the layout's size is computed here in int64).
  if (n < 0 || m < 0 || k < 0 || k > LARGE_KMAX) return false;
  {
    const int64_t KP = ((int64_t)k + 15) / 16 * 16, NP = ((int64_t)n + 63) / 64 * 64,
                  MP = ((int64_t)(m > 0 ? m : 1) + 63) / 64 * 64, RW = NP > MP ? NP : MP;
    const int64_t lds_total = 16 * KP + 2 * RW + 1024 + 64 + 8 * RW + 16 * RW + 12 * MAXC + 6 * RW + 5 * RW + 64 + 512;
    if (lds_total > INT32_MAX / 2 || KP * RW > INT32_MAX) return false;
  }
  const LargeLayout L = large_layout(n, m, k);
  // n, m: up to 64 LARGE_NB_MAX_CHOL with Cholesky factors of H and S (wide
  // panels in windows, socp_large.hip panel_chol_wide), in both operation
  // orders (SOCP_F_EXPLICIT_INVERSE forms Li and S^-1 from those factors)
  if (L.NPAD > 64 * LARGE_NB_MAX_CHOL || L.MPAD > 64 * LARGE_NB_MAX_CHOL || nc > MAXC) return false;
  size_t lds = (size_t)L.total * sizeof(double);
  const bool g = lds + 64 > 160 * 1024;
  if (g) lds = 64 * sizeof(double);
  if (lds_bytes) *lds_bytes = lds;
  if (gv) *gv = g;
  return true;
}

const char* const host::kUnsupported =
    "dims outside both kernels (register-resident: n, m <= 64, k <= 128, <= 8 cones; "
    "blocked: n, m <= 2048, <= 64 cones, k <= 2^21)";

// Which engine runs a call of these dims that wants kernel `kind`: the register kernel's cheapest variant
// that holds them (*v), or the blocked kernel (*v = NULL) -- with SOCP_F_FORCE_LARGE, with more than NCS
// cones, and where the variant has no kernel of the kind.  false: the dims fit neither (no error text is set).
static bool engine_fits(const socp_dims& d, int32_t flags, SmallKind kind, const SmallVariant** v) {
  *v = ((flags & SOCP_F_FORCE_LARGE) || d.ncones > NCS) ? nullptr : pick_variant(d.n, d.m, d.k);
  if (*v && !(*v)->k[kind].fn) *v = nullptr;
  return *v || large_fits(d.n, d.m, d.k, d.ncones, nullptr);
}
int host::choose_engine(const socp_dims& d, int32_t flags, SmallKind kind, const SmallVariant** v) {
  return engine_fits(d, flags, kind, v) ? 0 : fail(SOCP_E_UNSUPPORTED, kUnsupported);
}

extern "C" int socp_supported(const socp_dims* d) {
  const SmallVariant* v = nullptr;
  return d && engine_fits(*d, 0, KIND_SOLVE, &v) ? 1 : 0;
}

// ---------------------------------------------------------------- launch
static unsigned long long* g_stamps = nullptr;  // per-phase cycle table (SOCP_DIAG builds)

// 1, 2 or 4 when every cone is 16, 32 or 64 long (each cone is then whole
// 16-lane rows of one 64-element slot), else 0
static int cone_rows_uniform(const ConeTable& t, int nc) {
  const int d = t.dim[0];
  if (d != 16 && d != 32 && d != 64) return 0;
  for (int c = 1; c < nc; ++c)
    if (t.dim[c] != d) return 0;
  return d / 16;
}

// The A/B switches of the environment, read at every launch.  What NAME=0 does (the results
// are the same bits either way):
// SOCP_SLOT_SPECIALISE: the solver kernels take the slots as the cone table lays them out
// and run the mixed cone code (the A/B of the slot plan)
// SOCP_FUSE_U: the SYRK's cone rows U are formed by compute_U() in factor() on every table,
// as before the residuals' G x pass learnt to form them
// SOCP_INIT_OVERLAP: the initial point's G'G is formed by form_H's row loop on every kernel,
// not under G's load in load_problem
// SOCP_EXACT_FIT: a launch that fills its variant exactly runs the pair's generic pure-slot
// kernel, not the one compiled for its geometry (small_select)
static bool env_enabled(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0' && e[1] == '\0');
}

extern "C" int socp_debug_slot_plan(const socp_dims* d, const int32_t* kind, const int32_t* offs,
                                    const int32_t* dim, int32_t* rot, int32_t* kind0, int32_t* kind1) {
  ConeTable tab;
  int deg = 0;
  if (!rot || !kind0 || !kind1) return fail(SOCP_E_INVALID, "output pointers are NULL");
  TRY(check_problem(d, kind, offs, dim, &tab, &deg));  // the tables a solve takes, no others
  int32_t r = 0, kk = 0;
  small_slot_plan(tab, tab.nc, d->k, cone_rows_uniform(tab, tab.nc), env_enabled("SOCP_SLOT_SPECIALISE"), r, kk);
  *rot = r;
  *kind0 = kk & 15;
  *kind1 = kk >> 4;
  return 0;
}

// Which kernel of variant v a launch runs (*out), and what the choice sets in its arguments:
// al_rows, fuse_u, slot_rot, slot_kinds and init_overlap.  args: mode, flags, dims and cone
// table set; qp: the call carries a P.  Host logic only.
int host::small_select(const SmallVariant* v, SmallArgs& args, bool qp, SmallKernel* out) {
  args.al_rows = cone_rows_uniform(args.cones, args.nc);
  // (cones of 32 or 64 rows on a variant of whole 8-row-step chunks: a G x chunk lies in one cone)
  args.fuse_u = 0;
  if (args.al_rows >= 2 && v->NP % 8 == 0 && env_enabled("SOCP_FUSE_U")) {
    args.fuse_u = 0x100;
    for (int c = 0; c < args.nc && c < NCS; ++c)
      if (args.cones.kind[c] == SOC_K) args.fuse_u |= 1 << c;
  }
  const bool solver = args.mode == MODE_SOLVE;
  // SOCP_F_EXPLICIT_INVERSE: the explicit-inverse variants (m <= 16 shapes; larger m form Li anyway)
  const bool xi = (args.flags & SOCP_F_EXPLICIT_INVERSE) != 0 && v->k[KIND_XI].fn;
  // SOCP_F_DETECT_INFEASIBLE: the solver instantiation with the rule (never with xi: check_detect_flags)
  const bool di = solver && !xi && (args.flags & SOCP_F_DETECT_INFEASIBLE) != 0;
  int kind = qp   ? (solver ? KIND_QP : KIND_QP_KKT)  // (the plugin modes: the QP plugin-entry kernel)
             : di ? KIND_DI
             : xi ? (solver ? KIND_XI : KIND_XI_KKT)
                  : (solver ? KIND_SOLVE : KIND_KKT);
  // the slot plan: the plain solver only -- the kernel compiled for the table's pair of pure slots (the plugin
  // entries keep their records' layout; the xi and di solvers keep their one kernel; the QP solver is mixed only)
  const bool plain = kind == KIND_SOLVE;
  args.slot_rot = args.slot_kinds = 0;
  if (plain) {
    int32_t rot = 0, kinds = 0;
    small_slot_plan(args.cones, args.nc, args.k, args.al_rows, env_enabled("SOCP_SLOT_SPECIALISE"), rot, kinds);
    const int pair = slot_pair_of(kinds & 15, kinds >> 4);
    if (pair != SLOT_PAIR_NONE && v->k[KIND_SLOT_SP + pair - 1].fn) {
      kind = KIND_SLOT_SP + pair - 1;
      args.slot_rot = rot;
      args.slot_kinds = kinds;
      // the same solver compiled for exactly this launch's dims, cone table, al_rows, slot_rot and fuse_u,
      // where there is one (small_exact_fit: SOCP_FUSE_U=0 or SOCP_SLOT_SPECIALISE=0 so leave none)
      if (v->k[KIND_EXACT_SP + pair - 1].fn && env_enabled("SOCP_EXACT_FIT") &&
          small_exact_fit(args, v->NQ, v->NP, v->MQ, pair))
        kind = KIND_EXACT_SP + pair - 1;
    }
  }
  if (!v->k[kind].fn) return fail(SOCP_E_UNSUPPORTED, "no compiled kernel for these flags");
  // the load forms the initial point's G'G: the plain solver kernels compiled with the pipelined
  // load (mixed or pure-slot), when an initial factorisation follows the load (no warm start)
  args.init_overlap = plain && init_overlap_kernel(v->NQ, v->NP, v->MQ, 0) && !(args.flags & SOCP_F_WARM_START) &&
                      env_enabled("SOCP_INIT_OVERLAP");
  *out = v->k[kind];
  return 0;
}

extern "C" int socp_debug_exact_fit(const socp_dims* d, const int32_t* kind, const int32_t* offs, const int32_t* dim,
                                    int32_t flags, int32_t* exact) {
  SmallArgs a{};
  int deg = 0;
  if (!exact) return fail(SOCP_E_INVALID, "output pointer is NULL");
  TRY(check_problem(d, kind, offs, dim, &a.cones, &deg));
  *exact = 0;
  const SmallVariant* v = nullptr;
  if (!engine_fits(*d, flags, KIND_SOLVE, &v) || !v) return 0;  // the blocked kernel's, or no kernel's
  // what socp_batch_solve_ex gives launch_small of the choice's inputs
  fill_args(a, *d, d->batch, deg, nullptr);
  a.mode = MODE_SOLVE;
  a.flags = flags & ~(SOCP_F_EQUILIBRATE | SOCP_F_NORMALISE);
  SmallKernel kern;
  TRY(small_select(v, a, false, &kern));
  for (int pair = SLOT_PAIR_SP; pair <= SLOT_PAIR_PP; ++pair)
    if (kern.fn == v->k[KIND_EXACT_SP + pair - 1].fn) *exact = 1;
  return 0;
}

// a persistent kernel's launch: its problem counter zeroed, the launch inside the next timing pair, its name kept
static int launch_counted(socp_ctx* ctx, const SmallKernel& sel, int64_t grid, int threads, size_t lds,
                          int32_t* counter, void* args) {
  HIPCHK(hipMemsetAsync(counter, 0, sizeof(int32_t), ctx->stream));
  void* kargs[] = {args};
  HIPCHK(timing_begin(ctx));
  HIPCHK(hipLaunchKernel(sel.fn, dim3((unsigned)grid), dim3(threads), kargs, lds, ctx->stream));
  HIPCHK(timing_end(ctx));
  ctx->last_name = sel.name;
  return 0;
}

int host::launch_small(socp_ctx* ctx, SmallArgs& args, const SmallVariant* v, bool qp) {
  size_t lds = small_lds_bytes(v->NQ, v->NP, v->MQ);
  if (lds > 160 * 1024) return fail(SOCP_E_UNSUPPORTED, "LDS footprint too large");
  SmallKernel sel;
  TRY(small_select(v, args, qp, &sel));
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(sel.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sel.fn, 64, lds));
  if (per_cu < 1) per_cu = 1;
  int64_t blocks = (int64_t)ctx->num_cu * per_cu;
  if (blocks > args.B) blocks = args.B;
  if (blocks < 1) blocks = 1;
  args.stamps = g_stamps;
  return launch_counted(ctx, sel, blocks, 64, lds, args.counter, &args);
}

int host::launch_large(socp_ctx* ctx, const SmallArgs& a, double* rec, bool qp) {
  size_t lds = 0;
  bool gv = false;
  const bool xi = (a.flags & SOCP_F_EXPLICIT_INVERSE) != 0;
  if (!large_fits(a.n, a.m, a.k, a.nc, &lds, &gv)) return fail(SOCP_E_UNSUPPORTED, kUnsupported);
  const bool di = a.mode == MODE_SOLVE && !xi && (a.flags & SOCP_F_DETECT_INFEASIBLE) != 0;
  const LargeKernel sel = large_kernel(xi, gv, di, qp);
  if (!sel.fn) return fail(SOCP_E_UNSUPPORTED, "no compiled kernel for these flags");
  HIPCHK(hipFuncSetAttribute(sel.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sel.fn, 512, lds));
  if (per_cu < 1) return fail(SOCP_E_UNSUPPORTED, "blocked kernel does not fit on a CU");
  int64_t grid = (int64_t)ctx->num_cu * per_cu;
  if (grid > a.B) grid = a.B;
  if (grid < 1) grid = 1;
  const LargeLayout L = large_layout(a.n, a.m, a.k);
  LargeArgs la;
  la.a = a;
  la.a.stamps = g_stamps;
  la.wstride = L.w_total;
  const int rc = ctx->buf[socp_ctx::B_LWS].ensure((size_t)grid * (size_t)L.w_total * sizeof(double));
  if (rc) return fail(rc, "workspace allocation failed");
  la.ws = (double*)ctx->buf[socp_ctx::B_LWS].p;
  la.rec = rec;
  return launch_counted(ctx, sel, grid, 512, lds, a.counter, &la);
}

socp_params host::params_or_default(const socp_params* params) {
  socp_params P;
  socp_params_default(&P);
  return params ? *params : P;
}

socp_params host::fill_args(SmallArgs& a, const socp_dims& d, int64_t B, int degree, const socp_params* params) {
  const socp_params P = params_or_default(params);
  a.B = B;
  a.n = d.n;
  a.m = d.m;
  a.k = d.k;
  a.nc = d.ncones;
  a.deg = degree;
  a.maxit = P.maxit;
  a.sigma_exp = P.sigma_exp;
  a.tol = P.tol;
  a.step = P.step;
  a.init_eps = P.init_eps;
  return P;
}

int host::zero_cbh(DevBuf& buf, hipStream_t stream, SmallArgs& a) {
  const size_t bytes = (size_t)a.B * (a.n + a.m + a.k) * sizeof(double);
  if (buf.ensure(bytes)) return fail(SOCP_E_NOMEM, "device allocation failed");
  HIPCHK(hipMemsetAsync(buf.p, 0, bytes, stream));
  a.c = (const double*)buf.p;
  a.b = a.c + (size_t)a.B * a.n;
  a.h = a.b + (size_t)a.B * a.m;
  return 0;
}

// ------------------------------------------------------- problem dumps
// SOCP_DUMP_DIR=<dir> (env): every batch solve writes the first
// SOCP_DUMP_COUNT (default 1) problems of the batch as text, one file per
// quantity, as the reference's commented-out dumps do (solver.jl:48-67: A, G,
// c, b, h, cones; :75-82: the init right-hand side initv = [-c; b; h]).
// A QP solve (socp_batch_solve_qp) also writes its P.
// Matrices are written one row per line.  Diagnostic only: it synchronises.
static void dump_mat(const char* dir, int64_t p, const char* name, const double* v, int rows, int cols) {
  char fn[1024];
  snprintf(fn, sizeof(fn), "%s/problem%lld_%s.txt", dir, (long long)p, name);
  FILE* f = fopen(fn, "w");
  if (!f) return;
  for (int i = 0; i < rows; ++i) {
    for (int j = 0; j < cols; ++j) fprintf(f, j ? " %.17g" : "%.17g", v[(size_t)j * rows + i]);
    fputc('\n', f);
  }
  fclose(f);
}
static int dump_problems(socp_ctx* ctx, const SmallArgs& a, const double* Pq = nullptr) {
  const char* dir = getenv("SOCP_DUMP_DIR");
  if (!dir || !*dir) return 0;
  const char* cnt = getenv("SOCP_DUMP_COUNT");
  int64_t np = cnt ? atoll(cnt) : 1;
  if (np > a.B) np = a.B;
  const int n = a.n, m = a.m, k = a.k;
  std::vector<double> buf((size_t)k * n + (size_t)m * n + n + m + k + n + m + k);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int64_t p = 0; p < np; ++p) {
    double* G = buf.data();
    double* A = G + (size_t)k * n;
    double* c = A + (size_t)m * n;
    double* b = c + n;
    double* h = b + m;
    double* iv = h + k;
    const int64_t pm = (a.flags & SOCP_F_SHARED_MATRICES) ? 0 : p;  // the batch's one A and G
    HIPCHK(hipMemcpy(G, a.G + pm * (int64_t)k * n, sizeof(double) * k * n, hipMemcpyDefault));
    if (m) HIPCHK(hipMemcpy(A, a.A + pm * (int64_t)m * n, sizeof(double) * m * n, hipMemcpyDefault));
    HIPCHK(hipMemcpy(c, a.c + p * n, sizeof(double) * n, hipMemcpyDefault));
    if (m) HIPCHK(hipMemcpy(b, a.b + p * m, sizeof(double) * m, hipMemcpyDefault));
    HIPCHK(hipMemcpy(h, a.h + p * k, sizeof(double) * k, hipMemcpyDefault));
    for (int j = 0; j < n; ++j) iv[j] = -c[j];
    for (int i = 0; i < m; ++i) iv[n + i] = b[i];
    for (int i = 0; i < k; ++i) iv[n + m + i] = h[i];
    dump_mat(dir, p, "A", A, m, n);
    dump_mat(dir, p, "G", G, k, n);
    dump_mat(dir, p, "c", c, n, 1);
    dump_mat(dir, p, "b", b, m, 1);
    dump_mat(dir, p, "h", h, k, 1);
    dump_mat(dir, p, "initv", iv, n + m + k, 1);
    if (Pq) {
      std::vector<double> pb((size_t)n * n);
      HIPCHK(hipMemcpy(pb.data(), Pq + pm * (int64_t)n * n, sizeof(double) * n * n, hipMemcpyDefault));
      dump_mat(dir, p, "P", pb.data(), n, n);
    }
    char fn[1024];
    snprintf(fn, sizeof(fn), "%s/problem%lld_cones.txt", dir, (long long)p);
    if (FILE* f = fopen(fn, "w")) {
      for (int q = 0; q < a.nc; ++q)
        fprintf(f, "%s(%d,%d)\n", a.cones.kind[q] == POC_K ? "POC" : "SOC", a.cones.offs[q], a.cones.dim[q]);
      fclose(f);
    }
  }
  return 0;
}

// ------------------------------------------------------- equilibration
// socp_equil.hip on device pointers.  equil_matrices: the rule's passes on MB
// matrix sets; the exponents go to the context's B_EX buffer (MB x (n+m+k)
// int32, *ex), the factors and the scaled matrices where a pointer is given
// (a scaled matrix may be its own input).
static int equil_matrices(socp_ctx* ctx, const ConeTable& cones, int n, int m, int k, int nc, size_t MB,
                          const double* Pd, const double* Ad, const double* Gd, double* D, double* E, double* F,
                          double* Ps, double* As, double* Gs, const int32_t** ex) {
  const size_t S = (size_t)n + m + k;
  if (ctx->buf[socp_ctx::B_EX].ensure(MB * S * sizeof(int32_t))) return fail(SOCP_E_NOMEM, "device allocation failed");
  EquilArgs e;
  memset(&e, 0, sizeof(e));
  e.A = m > 0 ? Ad : nullptr;
  e.G = Gd;
  e.P = Pd;
  e.As = m > 0 ? As : nullptr;
  e.Gs = Gs;
  e.Ps = Pd ? Ps : nullptr;
  e.D = D;
  e.E = m > 0 ? E : nullptr;
  e.F = F;
  e.ex = (int32_t*)ctx->buf[socp_ctx::B_EX].p;
  e.n = n;
  e.m = m;
  e.k = k;
  e.nc = nc;
  e.passes = ctx->equil_passes;
  e.cones = cones;
  HIPCHK(equil_launch(e, (int64_t)MB, ctx->stream));
  *ex = e.ex;
  return 0;
}

// dst = ldexp(src, sign * exponent) on up to four batch-major vectors; `which`
// picks each vector's exponents: 0 ed (length n), 1 ee (m), 2 ef (k).  NULL
// vectors are skipped.
struct EquilVec {
  double* dst;
  const double* src;
  int which;
  int sign;
};
static int equil_vectors(socp_ctx* ctx, int n, int m, int k, int64_t B, bool shared, const int32_t* ex,
                         const EquilVec* v, int cnt) {
  const int len[3] = {n, m, k}, at[3] = {0, n, n + m};
  EquilVecArgs va;
  memset(&va, 0, sizeof(va));
  va.B = B;
  va.exstride = shared ? 0 : (int64_t)n + m + k;
  for (int i = 0; i < cnt; ++i) {
    if (!v[i].dst || !v[i].src || len[v[i].which] == 0) continue;
    EquilVecSeg& s = va.seg[va.nseg++];
    s.dst = v[i].dst;
    s.src = v[i].src;
    s.ex = ex + at[v[i].which];
    s.len = len[v[i].which];
    s.sign = v[i].sign;
  }
  HIPCHK(equil_vec_launch(va, ctx->stream));
  return 0;
}

extern "C" int socp_batch_equilibrate(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                      const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm,
                                      const double* c, const double* A, const double* b, const double* G,
                                      const double* h, int32_t flags, double* D, double* E, double* F, double* Ps,
                                      double* cs, double* As, double* bs, double* Gs, double* hs) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  ConeTable cones;
  memset(&cones, 0, sizeof(cones));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &cones, &degree));
  if (flags & ~(SOCP_F_DEVICE_PTRS | SOCP_F_SHARED_MATRICES))
    return fail(SOCP_E_INVALID, "socp_batch_equilibrate: flags other than SOCP_F_DEVICE_PTRS | SOCP_F_SHARED_MATRICES");
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (!socp_supported(dims)) return fail(SOCP_E_UNSUPPORTED, kUnsupported);
  if (B == 0) return 0;
  if (!G || (m > 0 && !A)) return fail(SOCP_E_INVALID, "NULL data pointer");
  if ((cs && !c) || (bs && !b) || (hs && !h) || (Ps && !Pm))
    return fail(SOCP_E_INVALID, "a scaled output without its input");
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  const bool shared = (flags & SOCP_F_SHARED_MATRICES) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const size_t MB = shared ? 1 : (size_t)B;
  typedef socp_ctx X;
  // host pointers: inputs staged as a solve stages them and scaled in place; D, E, F through B_EC, B_EB, B_EH
  const double *Pd = nullptr, *cd = nullptr, *Ad = nullptr, *bd = nullptr, *Gd = nullptr, *hd = nullptr;
  TRY(st.in(X::B_P, Pm, MB * n * n, &Pd));
  TRY(st.in(X::B_C, cs ? c : nullptr, (size_t)B * n, &cd));
  TRY(st.in(X::B_A, m > 0 ? A : nullptr, MB * m * n, &Ad));
  TRY(st.in(X::B_B, bs ? b : nullptr, (size_t)B * m, &bd));
  TRY(st.in(X::B_G, G, MB * k * n, &Gd));
  TRY(st.in(X::B_H, hs ? h : nullptr, (size_t)B * k, &hd));
  double *Dd = nullptr, *Ed = nullptr, *Fd = nullptr;
  TRY(st.out(X::B_EC, D, MB * n, false, &Dd));
  TRY(st.out(X::B_EB, E, MB * m, false, &Ed));
  TRY(st.out(X::B_EH, F, MB * k, false, &Fd));
  double* Psd = !Ps ? nullptr : dev ? Ps : const_cast<double*>(Pd);
  double* Asd = !As ? nullptr : dev ? As : const_cast<double*>(Ad);
  double* Gsd = !Gs ? nullptr : dev ? Gs : const_cast<double*>(Gd);
  double* csd = !cs ? nullptr : dev ? cs : const_cast<double*>(cd);
  double* bsd = !bs ? nullptr : dev ? bs : const_cast<double*>(bd);
  double* hsd = !hs ? nullptr : dev ? hs : const_cast<double*>(hd);
  const int32_t* ex = nullptr;
  TRY(equil_matrices(ctx, cones, n, m, k, dims->ncones, MB, Pd, Ad, Gd, Dd, Ed, Fd, Psd, Asd, Gsd, &ex));
  const EquilVec fw[3] = {{csd, cd, 0, 1}, {bsd, bd, 1, 1}, {hsd, hd, 2, 1}};
  TRY(equil_vectors(ctx, n, m, k, B, shared, ex, fw, 3));
  TRY(st.back(D, Dd, MB * n));
  TRY(st.back(E, Ed, MB * m));
  TRY(st.back(F, Fd, MB * k));
  TRY(st.back(Ps, Psd, MB * n * n));
  TRY(st.back(cs, csd, (size_t)B * n));
  TRY(st.back(As, Asd, MB * m * n));
  TRY(st.back(bs, bsd, (size_t)B * m));
  TRY(st.back(Gs, Gsd, MB * k * n));
  TRY(st.back(hs, hsd, (size_t)B * k));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ------------------------------------------------------- normalisation
// socp_norm.hip on device pointers.  norm_exponents: the rule's exponents of B
// problems in the context's B_NX buffer (B x 2 int32, *expo); batchwide: one
// pair for the whole batch (a shared P), through the norms in B_NN.
static int norm_exponents(socp_ctx* ctx, int64_t B, int n, int m, int k, const double* cd, const double* bd,
                          const double* hd, bool batchwide, const int32_t** expo) {
  typedef socp_ctx X;
  if (ctx->buf[X::B_NX].ensure((size_t)B * 2 * sizeof(int32_t))) return fail(SOCP_E_NOMEM, "device allocation failed");
  if (batchwide && ctx->buf[X::B_NN].ensure((size_t)B * 2 * sizeof(unsigned long long)))
    return fail(SOCP_E_NOMEM, "device allocation failed");
  NormArgs na;
  memset(&na, 0, sizeof(na));
  na.c = cd;
  na.b = m > 0 ? bd : nullptr;
  na.h = hd;
  na.expo = (int32_t*)ctx->buf[X::B_NX].p;
  na.nrm = batchwide ? (unsigned long long*)ctx->buf[X::B_NN].p : nullptr;
  na.B = B;
  na.n = n;
  na.m = m;
  na.k = k;
  HIPCHK(norm_launch(na, ctx->stream));
  if (batchwide) HIPCHK(norm_batch_launch(na.nrm, na.expo, B, ctx->stream));
  *expo = na.expo;
  return 0;
}

// dst = ldexp(src, +-(sc * ec + sb * eb)) on up to eight arrays of `rows` rows of `len`
// (row r takes problem r's exponents); NULL and empty arrays are skipped
struct NormVec {
  double* dst;
  const double* src;
  int64_t len, rows;
  int sc, sb;
};
static int norm_vectors(socp_ctx* ctx, const int32_t* expo, const NormVec* v, int cnt, bool forward) {
  NormScaleArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.expo = expo;
  for (int i = 0; i < cnt; ++i) {
    if (!v[i].dst || !v[i].src || v[i].len == 0 || v[i].rows == 0) continue;
    NormSeg& s = sa.seg[sa.nseg++];
    s.dst = v[i].dst;
    s.src = v[i].src;
    s.len = v[i].len;
    s.rows = v[i].rows;
    s.sc = v[i].sc;
    s.sb = v[i].sb;
  }
  HIPCHK(forward ? norm_forward_launch(sa, ctx->stream) : norm_backward_launch(sa, ctx->stream));
  return 0;
}

extern "C" int socp_batch_normalise(socp_ctx* ctx, const socp_dims* dims, const double* Pm, const double* c,
                                    const double* b, const double* h, int32_t flags, int32_t* expo, double* Ps,
                                    double* cs, double* bs, double* hs) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  if (!dims) return fail(SOCP_E_INVALID, "dims is NULL");
  if (dims->batch < 0 || dims->n <= 0 || dims->m < 0 || dims->k <= 0)
    return fail(SOCP_E_INVALID, "bad dims (need batch>=0, n>0, m>=0, k>0)");
  if (dims->batch > kMaxBatch)
    return fail(SOCP_E_INVALID, "batch above 2^31-1 (problem indices are int32 on the device)");
  if (flags & ~(SOCP_F_DEVICE_PTRS | SOCP_F_SHARED_MATRICES))
    return fail(SOCP_E_INVALID, "socp_batch_normalise: flags other than SOCP_F_DEVICE_PTRS | SOCP_F_SHARED_MATRICES");
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B == 0) return 0;
  if (!c || !h || (m > 0 && !b)) return fail(SOCP_E_INVALID, "NULL data pointer");
  if (Ps && !Pm) return fail(SOCP_E_INVALID, "a scaled output without its input");
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  const bool shared = (flags & SOCP_F_SHARED_MATRICES) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const size_t MB = shared ? 1 : (size_t)B;
  typedef socp_ctx X;
  // host pointers: inputs staged as a solve stages them and scaled in place
  const double *Pd = nullptr, *cd = nullptr, *bd = nullptr, *hd = nullptr;
  TRY(st.in(X::B_P, Ps ? Pm : nullptr, MB * n * n, &Pd));
  TRY(st.in(X::B_C, c, (size_t)B * n, &cd));
  TRY(st.in(X::B_B, m > 0 ? b : nullptr, (size_t)B * m, &bd));
  TRY(st.in(X::B_H, h, (size_t)B * k, &hd));
  double* Psd = !Ps ? nullptr : dev ? Ps : const_cast<double*>(Pd);
  double* csd = !cs ? nullptr : dev ? cs : const_cast<double*>(cd);
  double* bsd = !bs ? nullptr : dev ? bs : const_cast<double*>(bd);
  double* hsd = !hs ? nullptr : dev ? hs : const_cast<double*>(hd);
  const int32_t* ex = nullptr;
  TRY(norm_exponents(ctx, B, n, m, k, cd, bd, hd, shared && Pm, &ex));
  const NormVec fw[4] = {{csd, cd, n, B, 1, 0}, {bsd, bd, m, B, 0, 1}, {hsd, hd, k, B, 0, 1},
                         {Psd, Pd, (int64_t)n * n, (int64_t)MB, 1, -1}};
  TRY(norm_vectors(ctx, ex, fw, 4, true));
  if (expo) {
    if (dev)
      HIPCHK(hipMemcpyAsync(expo, ex, (size_t)B * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    else
      TRY(st.back(expo, ex, (size_t)B * 2));
  }
  TRY(st.back(Ps, Psd, MB * n * n));
  TRY(st.back(cs, csd, (size_t)B * n));
  TRY(st.back(bs, bsd, (size_t)B * m));
  TRY(st.back(hs, hsd, (size_t)B * k));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// socp_batch_solve_ex, and with Pm != NULL socp_batch_solve_qp: the QP solver
// kernels with the objective x'Px/2 + c'x
static int batch_solve_impl(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                            const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm,
                            const double* c, const double* A, const double* b,
                            const double* G, const double* h, const uint8_t* sing,
                            const socp_params* params, double* x, double* y, double* z,
                            double* s, int32_t* iters, int32_t* status, double* res) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  SmallArgs a;
  memset(&a, 0, sizeof(a));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree));
  const int64_t B = dims->batch;
  const socp_params P = fill_args(a, *dims, B, degree, params);
  const int n = dims->n, m = dims->m, k = dims->k;
  TRY(check_detect_flags(P.flags));
  const bool qp = Pm != nullptr;
  if (qp) TRY(check_qp_flags(P.flags, "socp_batch_solve_qp"));
  const bool eq = (P.flags & SOCP_F_EQUILIBRATE) != 0;
  if (eq && (P.flags & SOCP_F_WARM_START))
    return fail(SOCP_E_UNSUPPORTED,
                "SOCP_F_EQUILIBRATE with SOCP_F_WARM_START: the incoming iterate would have to be scaled as well");
  if (eq && (P.flags & SOCP_F_DETECT_INFEASIBLE))
    return fail(SOCP_E_UNSUPPORTED,
                "SOCP_F_EQUILIBRATE with SOCP_F_DETECT_INFEASIBLE: the meaning of the infeasibility tolerance would "
                "move with the scaling");
  const bool nrm = (P.flags & SOCP_F_NORMALISE) != 0;
  if (nrm && (P.flags & SOCP_F_DETECT_INFEASIBLE))
    return fail(SOCP_E_UNSUPPORTED,
                "SOCP_F_NORMALISE with SOCP_F_DETECT_INFEASIBLE: the meaning of the infeasibility tolerance would "
                "move with the scaling of c, b and h");
  if (B == 0) return 0;
  if (!c || !G || !h || !x || !z || !s || !iters || !status || (m > 0 && (!A || !b || !y)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  const SmallVariant* v = nullptr;
  TRY(choose_engine(*dims, P.flags, qp ? KIND_QP : KIND_SOLVE, &v));
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (P.flags & SOCP_F_DEVICE_PTRS) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const bool warm = (P.flags & SOCP_F_WARM_START) != 0;
  // SOCP_F_SHARED_MATRICES: one A, one G and one sing byte for the whole batch
  const size_t MB = (P.flags & SOCP_F_SHARED_MATRICES) ? 1 : (size_t)B;
  a.flags = P.flags & ~(SOCP_F_EQUILIBRATE | SOCP_F_NORMALISE);  // (the kernels run what they run without the flags)
  a.mode = MODE_SOLVE;
  if (P.flags & SOCP_F_DETECT_INFEASIBLE) small_set_itol(a, ctx->itol);
  typedef socp_ctx X;
  TRY(st.in(X::B_C, c, (size_t)B * n, &a.c));
  TRY(st.in(X::B_A, A, MB * m * n, &a.A));
  TRY(st.in(X::B_B, b, (size_t)B * m, &a.b));
  TRY(st.in(X::B_G, G, MB * k * n, &a.G));
  TRY(st.in(X::B_H, h, (size_t)B * k, &a.h));
  TRY(st.in(X::B_SING, sing, MB, &a.sing));
  const double* Pd = nullptr;
  if (qp) {
    TRY(st.in(X::B_P, Pm, MB * n * n, &Pd));
    small_set_qp(a, Pd);
  }
  TRY(st.out(X::B_X, x, (size_t)B * n, warm, &a.x));
  TRY(st.out(X::B_Y, y, (size_t)B * m, warm, &a.y));
  TRY(st.out(X::B_Z, z, (size_t)B * k, warm, &a.z));
  TRY(st.out(X::B_S, s, (size_t)B * k, warm, &a.s));
  TRY(st.out(X::B_IT, iters, (size_t)B, false, &a.iters));
  TRY(st.out(X::B_ST, status, (size_t)B, false, &a.status));
  TRY(st.out(X::B_RES, res, (size_t)B * 3, false, &a.res));
  TRY(st.reserve(X::B_CNT, 256));
  a.counter = (int32_t*)ctx->buf[X::B_CNT].p;
  TRY(dump_problems(ctx, a, Pd));  // (the caller's data: before any scaling)
  const int32_t* ex = nullptr;
  if (eq) {
    // SOCP_F_EQUILIBRATE: the solver reads scaled copies -- context buffers beside the caller's
    // device data, or the staged copy of host data scaled in place
    double* sc[6] = {const_cast<double*>(a.c), const_cast<double*>(a.A), const_cast<double*>(a.b),
                     const_cast<double*>(a.G), const_cast<double*>(a.h), const_cast<double*>(Pd)};
    if (dev) {
      const int slot[6] = {X::B_EC, X::B_EA, X::B_EB, X::B_EG, X::B_EH, X::B_EP};
      const size_t cnt[6] = {(size_t)B * n, MB * m * n, (size_t)B * m, MB * k * n, (size_t)B * k,
                             qp ? MB * n * n : 0};
      for (int i = 0; i < 6; ++i) {
        if (cnt[i] == 0) continue;
        TRY(st.reserve(slot[i], cnt[i] * sizeof(double)));
        sc[i] = (double*)ctx->buf[slot[i]].p;
      }
    }
    TRY(equil_matrices(ctx, a.cones, n, m, k, a.nc, MB, Pd, a.A, a.G, nullptr, nullptr, nullptr, sc[5], sc[1], sc[3],
                       &ex));
    const EquilVec fw[3] = {{sc[0], a.c, 0, 1}, {sc[2], a.b, 1, 1}, {sc[4], a.h, 2, 1}};
    TRY(equil_vectors(ctx, n, m, k, B, MB == 1 && (P.flags & SOCP_F_SHARED_MATRICES), ex, fw, 3));
    a.c = sc[0];
    a.A = sc[1];
    a.b = sc[2];
    a.G = sc[3];
    a.h = sc[4];
    if (qp) small_set_qp(a, Pd = sc[5]);
  }
  const int32_t* expo = nullptr;
  if (nrm) {
    // SOCP_F_NORMALISE: c, b, h and P scaled where they are copies already (staged host data, or
    // equilibration's), else into context buffers beside the caller's device data; a warm start's
    // iterate in place
    double* sc[4] = {const_cast<double*>(a.c), const_cast<double*>(a.b), const_cast<double*>(a.h),
                     const_cast<double*>(Pd)};
    if (dev && !eq) {
      const int slot[4] = {X::B_NC, X::B_NB, X::B_NH, X::B_NP};
      const size_t cnt[4] = {(size_t)B * n, (size_t)B * m, (size_t)B * k, qp ? MB * n * n : 0};
      for (int i = 0; i < 4; ++i) {
        if (cnt[i] == 0) continue;
        TRY(st.reserve(slot[i], cnt[i] * sizeof(double)));
        sc[i] = (double*)ctx->buf[slot[i]].p;
      }
    }
    TRY(norm_exponents(ctx, B, n, m, k, a.c, a.b, a.h, qp && MB == 1 && (P.flags & SOCP_F_SHARED_MATRICES), &expo));
    const NormVec fw[8] = {{sc[0], a.c, n, B, 1, 0},
                           {sc[1], a.b, m, B, 0, 1},
                           {sc[2], a.h, k, B, 0, 1},
                           {sc[3], Pd, (int64_t)n * n, (int64_t)MB, 1, -1},
                           {warm ? a.x : nullptr, a.x, n, B, 0, 1},
                           {warm ? a.y : nullptr, a.y, m, B, 1, 0},
                           {warm ? a.z : nullptr, a.z, k, B, 1, 0},
                           {warm ? a.s : nullptr, a.s, k, B, 0, 1}};
    TRY(norm_vectors(ctx, expo, fw, 8, true));
    a.c = sc[0];
    a.b = sc[1];
    a.h = sc[2];
    if (qp) small_set_qp(a, sc[3]);
  }
  const int launched = v ? launch_small(ctx, a, v, qp) : launch_large(ctx, a, nullptr, qp);
  if (nrm) {
    // x = 2^-eb x^, y = 2^-ec y^, z = 2^-ec z^, s = 2^-eb s^, whatever the status -- and after a launch that
    // failed, so that a warm start's iterate in the caller's device buffers does not stay scaled
    const NormVec bw[4] = {{a.x, a.x, n, B, 0, 1}, {a.y, a.y, m, B, 1, 0}, {a.z, a.z, k, B, 1, 0}, {a.s, a.s, k, B, 0, 1}};
    const int unscaled = norm_vectors(ctx, expo, bw, 4, false);
    if (!launched) TRY(unscaled);
  }
  TRY(launched);
  if (eq) {  // x = D x^, y = E y^, z = F z^, s = F^-1 s^
    const EquilVec bw[4] = {{a.x, a.x, 0, 1}, {a.y, a.y, 1, 1}, {a.z, a.z, 2, 1}, {a.s, a.s, 2, -1}};
    TRY(equil_vectors(ctx, n, m, k, B, (P.flags & SOCP_F_SHARED_MATRICES) != 0, ex, bw, 4));
  }
  TRY(st.back(x, a.x, (size_t)B * n));
  TRY(st.back(y, a.y, (size_t)B * m));
  TRY(st.back(z, a.z, (size_t)B * k));
  TRY(st.back(s, a.s, (size_t)B * k));
  TRY(st.back(iters, a.iters, (size_t)B));
  TRY(st.back(status, a.status, (size_t)B));
  TRY(st.back(res, a.res, (size_t)B * 3));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int socp_batch_solve_ex(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                   const int32_t* cone_offs, const int32_t* cone_dim,
                                   const double* c, const double* A, const double* b,
                                   const double* G, const double* h, const uint8_t* sing,
                                   const socp_params* params, double* x, double* y, double* z,
                                   double* s, int32_t* iters, int32_t* status, double* res) {
  return batch_solve_impl(ctx, dims, cone_kind, cone_offs, cone_dim, nullptr, c, A, b, G, h, sing, params, x, y, z,
                          s, iters, status, res);
}

extern "C" int socp_batch_solve_qp(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                   const int32_t* cone_offs, const int32_t* cone_dim, const double* P,
                                   const double* c, const double* A, const double* b,
                                   const double* G, const double* h, const uint8_t* sing,
                                   const socp_params* params, double* x, double* y, double* z,
                                   double* s, int32_t* iters, int32_t* status, double* res) {
  return batch_solve_impl(ctx, dims, cone_kind, cone_offs, cone_dim, P, c, A, b, G, h, sing, params, x, y, z, s,
                          iters, status, res);
}

extern "C" int socp_batch_solve(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                const int32_t* cone_offs, const int32_t* cone_dim, const double* c,
                                const double* A, const double* b, const double* G, const double* h,
                                const uint8_t* sing, const socp_params* params, double* x,
                                double* y, double* z, double* s, int32_t* iters, int32_t* status) {
  return socp_batch_solve_ex(ctx, dims, cone_kind, cone_offs, cone_dim, c, A, b, G, h, sing, params,
                             x, y, z, s, iters, status, nullptr);
}

static double* g_kkt_debug = nullptr;  // device buffer for socp_debug_kkt (testing hook)
unsigned long long* host::diag_stamps() { return g_stamps; }
double* host::diag_kkt_dump() { return g_kkt_debug; }
extern "C" int socp_debug_set_stamps(unsigned long long* dev_buf) {
#ifdef SOCP_DIAG
  g_stamps = dev_buf;
  return 0;
#else
  (void)dev_buf;
  return fail(SOCP_E_UNSUPPORTED, "phase stamps exist only in the diagnostic build (libsocp_diag.so)");
#endif
}

extern "C" int socp_debug_set_kkt_dump(double* dev_buf) {
#ifdef SOCP_DIAG
  g_kkt_debug = dev_buf;
  return 0;
#else
  (void)dev_buf;
  return fail(SOCP_E_UNSUPPORTED, "KKT dumps exist only in the diagnostic build (libsocp_diag.so)");
#endif
}

// socp_batch_kkt_solve, and with Pm != NULL socp_batch_kkt_solve_qp: the QP
// plugin-entry kernels, whose first block row is P cx + A'cy + G'cz = dx
static int batch_kkt_impl(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                          const int32_t* cone_offs, const int32_t* cone_dim, const double* Pm,
                          const double* A, const double* G, const uint8_t* sing,
                          const double* s, const double* z, const double* dx,
                          const double* dy, const double* dz, const double* ds,
                          double* cx, double* cy, double* cz, double* cs,
                          int32_t* kkt_status, int32_t flags) {
  if (!ctx) return fail(SOCP_E_INVALID, "ctx is NULL");
  const bool qp = Pm != nullptr;
  // (SOCP_F_DETECT_INFEASIBLE is no flag of the plugin entries: ignored, as socp_batch_kkt_solve ignores it)
  if (qp) TRY(check_qp_flags(flags & ~SOCP_F_DETECT_INFEASIBLE, "socp_batch_kkt_solve_qp"));
  SmallArgs a;
  memset(&a, 0, sizeof(a));
  int degree = 0;
  TRY(check_problem(dims, cone_kind, cone_offs, cone_dim, &a.cones, &degree));
  const int64_t B = dims->batch;
  const int n = dims->n, m = dims->m, k = dims->k;
  if (B == 0) return 0;
  if (!G || !s || !z || !dx || !dz || !ds || !cx || !cz || !cs || !kkt_status ||
      (m > 0 && (!A || !dy || !cy)))
    return fail(SOCP_E_INVALID, "NULL data pointer");
  const SmallVariant* v = nullptr;
  TRY(choose_engine(*dims, flags, qp ? KIND_QP_KKT : KIND_KKT, &v));
  HIPCHK(hipSetDevice(ctx->device));
  const bool dev = (flags & SOCP_F_DEVICE_PTRS) != 0;
  const Stager st{ctx->buf, ctx->stream, dev, nullptr};
  const size_t MB = (flags & SOCP_F_SHARED_MATRICES) ? 1 : (size_t)B;
  fill_args(a, *dims, B, degree, &kKktParams);
  a.mode = MODE_KKT;
  a.flags = flags & (SOCP_F_EXPLICIT_INVERSE | SOCP_F_SHARED_MATRICES);
  a.dbg = g_kkt_debug;
  typedef socp_ctx X;
  TRY(zero_cbh(ctx->buf[X::B_C], ctx->stream, a));
  TRY(st.in(X::B_A, A, MB * m * n, &a.A));
  TRY(st.in(X::B_G, G, MB * k * n, &a.G));
  TRY(st.in(X::B_SING, sing, MB, &a.sing));
  if (qp) {
    const double* Pd = nullptr;
    TRY(st.in(X::B_P, Pm, MB * n * n, &Pd));
    small_set_qp_plugin(a, Pd);
  }
  TRY(st.out(X::B_S, const_cast<double*>(s), (size_t)B * k, true, &a.s));
  TRY(st.out(X::B_Z, const_cast<double*>(z), (size_t)B * k, true, &a.z));
  TRY(st.in(X::B_DX, dx, (size_t)B * n, &a.dx));
  TRY(st.in(X::B_DY, dy, (size_t)B * m, &a.dy));
  TRY(st.in(X::B_DZ, dz, (size_t)B * k, &a.dz));
  TRY(st.in(X::B_DS, ds, (size_t)B * k, &a.ds));
  TRY(st.out(X::B_CX, cx, (size_t)B * n, false, &a.cx));
  TRY(st.out(X::B_CY, cy, (size_t)B * m, false, &a.cy));
  TRY(st.out(X::B_CZ, cz, (size_t)B * k, false, &a.cz));
  TRY(st.out(X::B_CS, cs, (size_t)B * k, false, &a.cs));
  TRY(st.out(X::B_ST, kkt_status, (size_t)B, false, &a.status));
  TRY(st.reserve(X::B_CNT, 256));
  a.counter = (int32_t*)ctx->buf[X::B_CNT].p;
  TRY(v ? launch_small(ctx, a, v, qp) : launch_large(ctx, a, nullptr, qp));
  TRY(st.back(cx, a.cx, (size_t)B * n));
  TRY(st.back(cy, a.cy, (size_t)B * m));
  TRY(st.back(cz, a.cz, (size_t)B * k));
  TRY(st.back(cs, a.cs, (size_t)B * k));
  TRY(st.back(kkt_status, a.status, (size_t)B));
  if (!dev) HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int socp_batch_kkt_solve(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                    const int32_t* cone_offs, const int32_t* cone_dim,
                                    const double* A, const double* G, const uint8_t* sing,
                                    const double* s, const double* z, const double* dx,
                                    const double* dy, const double* dz, const double* ds,
                                    double* cx, double* cy, double* cz, double* cs,
                                    int32_t* kkt_status, int32_t flags) {
  return batch_kkt_impl(ctx, dims, cone_kind, cone_offs, cone_dim, nullptr, A, G, sing, s, z, dx, dy, dz, ds, cx, cy,
                        cz, cs, kkt_status, flags);
}

extern "C" int socp_batch_kkt_solve_qp(socp_ctx* ctx, const socp_dims* dims, const int32_t* cone_kind,
                                       const int32_t* cone_offs, const int32_t* cone_dim, const double* P,
                                       const double* A, const double* G, const uint8_t* sing,
                                       const double* s, const double* z, const double* dx,
                                       const double* dy, const double* dz, const double* ds,
                                       double* cx, double* cy, double* cz, double* cs,
                                       int32_t* kkt_status, int32_t flags) {
  return batch_kkt_impl(ctx, dims, cone_kind, cone_offs, cone_dim, P, A, G, sing, s, z, dx, dy, dz, ds, cx, cy, cz,
                        cs, kkt_status, flags);
}
