// socp_host.hpp — what the C ABI units (socp_api*.hip) share: the error
// string, device buffers, the context, staging of host pointers, the problem
// checks and the two solver launchers.  Everything declared here is defined
// once, in socp_api.hip (the generator unit's launchers in socp_api_gen.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/socp.h"
#include "socp_kernels.hpp"

namespace socp::host {

// sets the calling thread's socp_last_error() text (one thread_local string for
// the whole library, behind this function) and returns `code`
int fail(int code, const std::string& msg);

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return ::socp::host::fail(SOCP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define TRY(x)          \
  do {                  \
    int rc_ = (x);      \
    if (rc_) return rc_; \
  } while (0)

// the persistent kernels pull problem indices from an int32 counter and the
// per-problem launches use one workgroup per problem (grid.x)
constexpr int64_t kMaxBatch = 0x7fffffff;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    size_t want = bytes < 256 ? 256 : bytes;
    if (hipMalloc(&p, want) != hipSuccess) return SOCP_E_NOMEM;
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace socp::host

struct socp_ctx {
  int device = 0;
  hipStream_t own = nullptr;     // created by socp_ctx_create
  hipStream_t stream = nullptr;  // where work goes: `own`, or the caller's (socp_ctx_set_stream)
  // timing pairs around the solver launches, a ring of NTIME so that a run of
  // launches can be timed without a host synchronisation between them
  // (socp_last_kernel_ms, socp_kernel_times)
  static constexpr int NTIME = 64;
  hipEvent_t tev0[NTIME] = {}, tev1[NTIME] = {};
  int64_t tlaunches = 0;
  hipEvent_t evh = nullptr;                 // stream hand-off (ctx_switch_stream), never a timing event
  int num_cu = 0;
  float last_ms = 0.f;
  const char* last_name = "";
  double itol = 1e-7;  // SOCP_F_DETECT_INFEASIBLE's tolerance (socp_ctx_set_infeasibility_tol)
  int equil_passes = 8;  // SOCP_F_EQUILIBRATE's passes (socp_ctx_set_equilibration_passes)
  // B_EX: the equilibration exponents; B_E*: the scaled copies of device-pointer inputs, and with
  // host pointers the staging of socp_batch_equilibrate's D, E, F
  // B_NX: SOCP_F_NORMALISE's exponents, B_NN: the norms of its shared-P batch stage; B_N*: the scaled
  // copies of device-pointer inputs that equilibration has not copied already
  // B_VST: the fused KKT solve's status inside socp_batch_centre / socp_batch_vjp; B_VOUT: the staging of
  // socp_batch_vjp's vector outputs; B_VSUM: socp_batch_vjp_sum's per-slab partial sums
  enum { B_C, B_A, B_B, B_G, B_H, B_SING, B_X, B_Y, B_Z, B_S, B_IT, B_ST, B_RES, B_DX, B_DY,
         B_DZ, B_DS, B_CX, B_CY, B_CZ, B_CS, B_CNT, B_LWS, B_ERR, B_P, B_EX, B_EC, B_EA, B_EB,
         B_EG, B_EH, B_EP, B_VST, B_VOUT, B_VSUM, B_NX, B_NN,
         B_NC, B_NB, B_NH, B_NP, NB };
  socp::host::DevBuf buf[NB];
};

namespace socp::host {

// the timing pair of the next launch
hipError_t timing_begin(socp_ctx* c);
hipError_t timing_end(socp_ctx* c);

// Staging between a caller's arrays and a context's or handle's device buffers
// `bufs`, on `stream`.  With `dev` (SOCP_F_DEVICE_PTRS) the caller's pointers
// are device pointers and pass through; so do NULL and zero counts.  Host
// sources are copied asynchronously and their bytes added to *h2d (may be NULL).
struct Stager {
  DevBuf* bufs;
  hipStream_t stream;
  bool dev;
  int64_t* h2d;
  // bufs[slot] grown to `bytes` and, with `copy`, `src` copied into it
  int put(int slot, const void* src, size_t bytes, bool copy, hipMemcpyKind kind = hipMemcpyHostToDevice) const;
  int reserve(int slot, size_t bytes) const { return put(slot, nullptr, bytes, false); }
  // an output (copy_in: read as well, e.g. a warm start); `back` returns it
  template <class T>
  int out(int slot, T* user, size_t count, bool copy_in, T** o) const {
    *o = user;
    if (!user || count == 0 || dev) return 0;
    TRY(put(slot, user, count * sizeof(T), copy_in));
    *o = (T*)bufs[slot].p;
    return 0;
  }
  template <class T>
  int in(int slot, const T* src, size_t count, const T** o) const { return out(slot, src, count, true, o); }
  template <class T>
  int back(T* user, const T* devp, size_t count) const {
    if (dev || !user || count == 0) return 0;
    HIPCHK(hipMemcpyAsync(user, devp, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    return 0;
  }
  // a copy the handle owns in bufs[slot] (the caller's device buffers may be
  // reused): device to device with `dev`, else from the host
  int own(int slot, const void* src, size_t bytes) const {
    if (!src || bytes == 0) return 0;
    return put(slot, src, bytes, true, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  }
};

// a dense or rank-update handle: its context's stream drained, its buffers released
template <class H>
void handle_free(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  for (auto& b : h->buf) b.release();
  delete h;
}

// ---------------------------------------------------------------- checks
int check_problem(const socp_dims* d, const int32_t* kind, const int32_t* offs, const int32_t* dim, ConeTable* tab,
                  int* degree);
int check_detect_flags(int32_t flags);
// SOCP_F_EQUILIBRATE or SOCP_F_NORMALISE on an entry that does not scale
int check_no_equilibrate(int32_t flags, const char* who);
int check_qp_flags(int32_t flags, const char* who);
extern const char* const kUnsupported;
// the engine of a call that wants kernel `kind`: *v the register kernel's variant, or NULL for the blocked kernel
int choose_engine(const socp_dims& d, int32_t flags, SmallKind kind, const SmallVariant** v);

// ---------------------------------------------------------------- launch
// *params, or socp_params_default's values when it is NULL
socp_params params_or_default(const socp_params* params);
// a's dims (B problems of d's shape) and degree, and the solver parameters
// maxit ... init_eps of params_or_default(params), which is returned
socp_params fill_args(SmallArgs& a, const socp_dims& d, int64_t B, int degree, const socp_params* params);
// the plugin entries' parameters: one iteration, no stopping rule
constexpr socp_params kKktParams = {1, 3, 0.0, 0.0, 0.0, 0, 0};
// a.c | a.b | a.h as one zeroed block in `buf`: the KKT entries do not use them but the loader reads them
int zero_cbh(DevBuf& buf, hipStream_t stream, SmallArgs& a);
// the kernel of variant v that a launch of args runs (no HIP call: socp_debug_exact_fit asks it too)
int small_select(const SmallVariant* v, SmallArgs& args, bool qp, SmallKernel* out);
// qp: the QP solver (socp_batch_solve_qp; args carries P, small_set_qp)
int launch_small(socp_ctx* ctx, SmallArgs& args, const SmallVariant* v, bool qp = false);
int launch_large(socp_ctx* ctx, const SmallArgs& a, double* rec = nullptr, bool qp = false);
// the diagnostic build's device buffers (NULL otherwise): the per-phase cycle
// table (socp_debug_set_stamps) and the KKT dump (socp_debug_set_kkt_dump)
unsigned long long* diag_stamps();
double* diag_kkt_dump();

// ------------------------------------------------- socp_api_gen.hip's kernels
// plain launches on `stream`; the caller checks hipGetLastError()
void pack_csc_launch(hipStream_t stream, int64_t batch, int32_t rows, int32_t cols, const int64_t* nz_offs,
                     const int64_t* colptr, const int64_t* rowval, const double* nzval, int64_t base, double* dense,
                     int32_t* err);
void pair_launch(hipStream_t stream, int64_t B, const int32_t* status, const int32_t* iters, int32_t* pairs);
void outcome_launch(hipStream_t stream, int64_t B, const int32_t* status, const int32_t* iters, const double* res,
                    socp_outcome* rec);

}  // namespace socp::host
