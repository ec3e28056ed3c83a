/*
 * socp.h — C ABI of libsocp, the MI355X-native batched dense SOCP solver.
 *
 * This is the drop-in boundary for the dense path of BenChung/Socp.jl.
 * The reference has no C ABI of its own: its plugin interface is Julia multiple
 * dispatch (abstract type KKTSolver{T}, Socp.jl:77-78) and the per-iteration
 * calls compute_scaling / setup_iter / solve_kkt made by solve_socp
 * (solver.jl:105-151).  Every entry point below names the reference interface
 * it replaces; INTEGRATION.md shows the `ccall` binding a Julia maintainer adds.
 *
 * Problem (reference Socp.jl:20-38, README.md:4):
 *     minimize c'x   s.t.  A x = b,   G x + s = h,   s in K
 * K is a product of cones listed POC-first then SOC, contiguous over 0..k-1
 * (scalings.jl:102).  All arithmetic is IEEE fp64.
 *
 * Layout (shared by host and device pointers):
 *   - one cone description for the whole batch (every problem has the same
 *     dims and cone structure, as the reference's Problem{C,n,m,k} type does);
 *   - per problem, matrices are dense COLUMN-MAJOR (Julia order):
 *       A: m x n  -> A[p*m*n + j*m + i] = A_p(i,j)
 *       G: k x n  -> G[p*k*n + j*k + i] = G_p(i,j)
 *     vectors are stacked batch-major: c[p*n + j], b[p*m + i], h[p*k + i], ...
 *
 * Errors: every function returns 0 on success and a negative SOCP_E* code on
 * an API error; socp_last_error() gives a message (thread-local).  Numerical
 * failures are NOT API errors: they are reported per problem in status[]
 * (the reference instead throws PosDefException / DomainError and aborts the
 * solve: densesolver.jl:47,51; Julia sqrt of a negative argument).
 */
#ifndef SOCP_H
#define SOCP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes (API errors) ---- */
#define SOCP_OK 0
#define SOCP_E_INVALID (-1)     /* bad argument / shape (reference: AssertionError, Socp.jl:43-47) */
#define SOCP_E_UNSUPPORTED (-2) /* dims not covered by any compiled kernel                          */
#define SOCP_E_HIP (-3)         /* HIP runtime error                                                 */
#define SOCP_E_NOMEM (-4)       /* device allocation failed                                          */

/* ---- per-problem status (numerical outcome) ---- */
#define SOCP_CONVERGED 0      /* exit test ||rd||+||rp||+z's < tol met (solver.jl:122)               */
#define SOCP_MAXIT 1          /* iteration cap reached (solver.jl:105)                               */
#define SOCP_CHOL_H_FAILED 2  /* H = G'W^-2G (+A'A) not positive definite (densesolver.jl:47)        */
#define SOCP_CHOL_S_FAILED 3  /* S = A H^-1 A' not positive definite (densesolver.jl:51)            */
#define SOCP_DOMAIN_ERROR 4   /* sqrt of a negative number: Julia throws DomainError (scalings.jl:46,47,57,68,91; mats.jl:71) */
#define SOCP_PRIMAL_INFEASIBLE 5 /* SOCP_F_DETECT_INFEASIBLE: (y, z) certifies that no x, s in K satisfy Ax = b, Gx + s = h */
#define SOCP_DUAL_INFEASIBLE 6   /* SOCP_F_DETECT_INFEASIBLE: (x, s) is a ray along which c'x is unbounded below            */

/* ---- cone kinds (reference Socp.jl:8-16) ---- */
#define SOCP_CONE_POC 0 /* nonnegative orthant, POC{D}(offs) */
#define SOCP_CONE_SOC 1 /* second-order cone,   SOC{D}(offs) */

typedef struct socp_dims {
  int64_t batch; /* number of independent problems B                    */
  int32_t n;     /* variables        (Problem.n, Socp.jl:36)             */
  int32_t m;     /* equality rows    (Problem.m)                         */
  int32_t k;     /* cone rows        (Problem.k)                         */
  int32_t ncones;
} socp_dims;

/* Solver constants.  Defaults (socp_params_default) equal the reference's
 * hard-coded values: maxit 40 (solver.jl:105), tol 1e-5 absolute (:122),
 * step 0.99 (:146), sigma exponent 3 (:133), init shift threshold 1e-10 (:91,97). */
typedef struct socp_params {
  int32_t maxit;
  int32_t sigma_exp;
  double tol;      /* tol = 0 gives the fixed-iteration ("fixed-K") mode        */
  double step;
  double init_eps;
  int32_t flags;   /* SOCP_F_* bit set */
  int32_t reserved;
} socp_params;

#define SOCP_F_DEVICE_PTRS 1 /* all data pointers are device (HBM) pointers */
#define SOCP_F_WARM_START 2  /* x,y,z,s hold the starting iterate: skip the init solve (solver.jl:68-104) */
#define SOCP_F_FORCE_LARGE 4 /* run the blocked kernel even where the register-resident one applies (testing, tuning) */
/* Form Li = H^-1 explicitly, as densesolver.jl:47-48 does (ldiv!(Li,
 * cholesky!(H), I): H = L L', then Li = L^-T L^-1 from the factor; S^-1 the
 * same way), and use it in every solve (:73,83) -- the reference's operation
 * order.  By
 * default the kernels factor H = L L' (cholesky!, :47) and replace every
 * product with Li by two triangular solves (A Li enters as Z = L^-1 A',
 * S = Z'Z): the same linear algebra in exact arithmetic, far more accurate
 * near the end of a solve -- where the explicit inverse decides convergence
 * (a pure LP: chol(H) fails on every problem with it, converges without; see
 * DESIGN.md §9).  Honoured by socp_batch_solve[_ex], socp_batch_kkt_solve,
 * socp_dense_create (for all calls of the handle) and socp_ingest_submit. */
#define SOCP_F_EXPLICIT_INVERSE 8
/* Infeasibility / unboundedness detection (the reference has none: solver.jl:
 * 105-151 runs such a problem to maxit or into a PosDefException).  Bits 16 to
 * 128 belong to flags of the CPU oracle.  With this flag the rule below is
 * evaluated where the exit test is (solver.jl:122): at the start of iteration
 * `it` < maxit, after compute_scaling's domain check and the exit test, before
 * the factorisation; warm-started solves included.  tau is the context's
 * infeasibility tolerance (socp_ctx_set_infeasibility_tol, default 1e-7).
 *   1. hz = h'z + b'y.  If hz < 0 and ||A'y + G'z||_2 < tau (-hz):
 *      status SOCP_PRIMAL_INFEASIBLE; y and z are returned multiplied by
 *      1/(-hz), so that b'y + h'z = -1; x and s as they stand.
 *   2. Otherwise cx = c'x.  If cx < 0 and max(||Ax||_2, ||Gx + s||_2) < tau (-cx):
 *      status SOCP_DUAL_INFEASIBLE; x and s are returned multiplied by
 *      1/(-cx), so that c'x = -1; y and z as they stand.
 * In both cases iters = it and res[] holds the exit-test quantities at the
 * iterate before that multiplication.  With m = 0 the b and A terms vanish.
 * Every comparison is false on NaN.  The iterates are interior to the cones,
 * so the returned (y, z) or (x, s) is a certificate that can be checked from
 * the outputs alone (z in K*, or s in K).  Without the flag nothing changes:
 * the solver kernels that run are the ones that ran before.
 * Honoured by socp_batch_solve[_ex], socp_ingest_submit[_csc] and
 * socp_sqr_solve_socp through params->flags.  Together with
 * SOCP_F_EXPLICIT_INVERSE the call returns SOCP_E_UNSUPPORTED: in that
 * operation order the iteration at which the rule fires moves under a one-ulp
 * change of G.  The register kernel's m > 16 shapes, which
 * form the inverse by nature, stay supported. */
#define SOCP_F_DETECT_INFEASIBLE 256
/* Parametric batches: one A and one G shared by every problem of the batch
 * (model-predictive control; the reference's own timed workload solves one
 * optimal-control problem 100 times with the same matrices, runtests.jl:241-243).
 * With this flag
 *   A    points to ONE m x n matrix and G to ONE k x n matrix, column-major
 *        as above (A[j*m + i], G[j*k + i]);
 *   sing points to ONE byte, or is NULL for the device probe;
 * and every problem of the batch uses those.  c, b, h, the iterates and all
 * outputs stay per problem.  Contract: a call with the flag returns, for every
 * output array, the bits of the same call without the flag on A, G and sing
 * replicated B times -- on every kernel and in every combination with the
 * other flags.  Without the flag nothing changes.  The register kernel then
 * loads G (and A) once per wavefront instead of once per problem; the other
 * kernels change only their addressing.
 * Honoured through params->flags by socp_batch_solve[_ex]; through `flags` by
 * socp_batch_kkt_solve, socp_dense_create and socp_sqr_create (for all calls
 * of the handle, socp_sqr_solve_socp included: the handle copies one A and one
 * G at create, and socp_*_h2d_bytes reports that smaller count; the factor
 * records stay per problem) and by socp_ingest_create (the matrices are then
 * given by socp_ingest_set_matrices, not per submit). */
#define SOCP_F_SHARED_MATRICES 512
/* Equilibration: the solver stops on an absolute test and factors H without
 * pivoting, so both depend on the units of the caller's rows and columns.
 * With this flag the problem is first scaled by socp_batch_equilibrate's rule
 * (below) -- diagonal D, E, F whose entries are powers of two, so scaling and
 * unscaling are exact in fp64 -- then solved, then unscaled.
 * Contract: every output (x, y, z, s, iters, status, res, the kernel name) is
 * bitwise what this pipeline gives:
 *   1. socp_batch_equilibrate on (P, c, A, b, G, h);
 *   2. the same solve entry without the flag on the scaled data;
 *   3. x = D x^, y = E y^, z = F z^, s = F^-1 s^ (ldexp: exact).
 * It follows that tol, init_eps, the sing == NULL probe and res[] refer to the
 * SCALED problem: status == 0 still implies res[0] + res[1] + res[2] < tol, in
 * the scaled units (res[0] is ||D rd||, res[1] is ||E rp|| of the returned
 * iterate; z's is invariant, and so are G x + s = h up to F, cone membership
 * and the objective).  A given `sing` is used as given.  The caller's inputs
 * are never written: the scaled copies live in buffers of the context (with
 * host pointers, the staged device copy is scaled in place).  The
 * SOCP_DUMP_DIR dump writes the caller's data.
 * Honoured through params->flags by socp_batch_solve, socp_batch_solve_ex and
 * socp_batch_solve_qp.  SOCP_F_FORCE_LARGE, SOCP_F_EXPLICIT_INVERSE and
 * SOCP_F_SHARED_MATRICES pass through (shared: one scaling for the batch, and
 * the replicated-bits contract above holds).  With SOCP_F_WARM_START (the
 * incoming iterate would need scaling) or SOCP_F_DETECT_INFEASIBLE (tau's
 * meaning would move with the units) the call returns SOCP_E_UNSUPPORTED;
 * so do socp_ingest_submit[_csc] and socp_sqr_solve_socp for the bit.
 * Without the flag nothing changes. */
#define SOCP_F_EQUILIBRATE 1024
/* Normalisation: the exit test ||rd|| + ||rp|| + z's < tol is absolute, so it
 * depends on the units of c, b and h, which equilibration leaves alone.  With
 * this flag c and (b, h) are first scaled by socp_batch_normalise's rule
 * (below) -- two powers of two per problem, so scaling and unscaling are exact
 * in fp64 -- then the problem is solved, then the iterates are unscaled.  The
 * rule, per problem p:
 *   nc = max_j |c_j|;
 *   nb = max(max_i |b_i|, max_i |h_i|); the b term is absent when m = 0;
 *   e(v) = -ilogb(v) for v finite and > 0, subnormals included, clamped to
 *          [-256, 256];
 *   e(v) = 0 for every other v: zero, Inf, and NaN anywhere in the vector;
 *   ec = e(nc), eb = e(nb).  Afterwards the largest entry of c^, and of
 *   (b^, h^), lies in [1, 2).
 * The scaled problem:
 *   c^ = ldexp(c, ec);
 *   b^ = ldexp(b, eb), h^ = ldexp(h, eb);
 *   P^ = ldexp(P, ec - eb);
 *   A and G as given.
 * The iterates, both ways:
 *   forward: x^ = ldexp(x, eb), s^ = ldexp(s, eb), y^ = ldexp(y, ec),
 *            z^ = ldexp(z, ec);
 *   unscaling uses the negated exponents.
 * The factors are per problem, with SOCP_F_SHARED_MATRICES too, since c, b and
 * h stay per problem there.  One exception: with SOCP_F_SHARED_MATRICES and a
 * P, nc and nb are the maxima over the whole batch, so that one P^ serves
 * every problem (a maximum is exact in any order).
 * Contract: every output (x, y, z, s, iters, status, res, the kernel name) is
 * bitwise what this pipeline gives:
 *   1. socp_batch_normalise on (P, c, b, h);
 *   2. the same solve entry without the flag on the scaled data; with
 *      SOCP_F_WARM_START the incoming iterate is scaled forward as above;
 *   3. the unscaling of x, y, z, s.
 * It follows that tol, init_eps and res[] refer to the NORMALISED problem:
 * status == 0 implies 2^ec ||rd|| + 2^eb ||rp|| + 2^(ec+eb) z's < tol in the
 * caller's units -- a test relative to the sizes of c and of (b, h).  The
 * iterates are unscaled whatever the status.  The caller's inputs are never
 * written: the scaled copies live in buffers of the context (with host
 * pointers, the staged device copy is scaled in place); with device pointers
 * the in/out iterate of a warm start is scaled in place and unscaled in place,
 * also when the solver's launch returns an error.
 * The SOCP_DUMP_DIR dump writes the caller's data.
 * Honoured through params->flags by socp_batch_solve, socp_batch_solve_ex and
 * socp_batch_solve_qp.  SOCP_F_DEVICE_PTRS, SOCP_F_WARM_START,
 * SOCP_F_FORCE_LARGE, SOCP_F_EXPLICIT_INVERSE and SOCP_F_SHARED_MATRICES pass
 * through.  With SOCP_F_EQUILIBRATE the order is equilibrate, normalise,
 * solve, un-normalise, unscale; every step is exact, so both pipeline
 * contracts hold together.  With SOCP_F_DETECT_INFEASIBLE the call returns
 * SOCP_E_UNSUPPORTED (the rule's ratios change by 2^eb and 2^ec, so tau's
 * meaning would move, as it does under equilibration); so do
 * socp_ingest_submit[_csc] and socp_sqr_solve_socp for the bit.
 * Without the flag nothing changes. */
#define SOCP_F_NORMALISE 2048

typedef struct socp_ctx socp_ctx;

/* Library / context.  One context per host thread, each owning a HIP stream
 * (the reference indexes CHOLMOD state by Threads.threadid(), cholutils.jl:73). */
const char* socp_last_error(void);
const char* socp_version(void);
void socp_params_default(socp_params* p);
int socp_ctx_create(int device, socp_ctx** out);
int socp_ctx_destroy(socp_ctx* ctx);
int socp_ctx_sync(socp_ctx* ctx);
/* hipStream_t of the context (as void*) so callers can order their own work. */
void* socp_ctx_stream(socp_ctx* ctx);
/* Make the context issue its work on the caller's hipStream_t (as void*), e.g.
 * torch.cuda.current_stream().cuda_stream, so the solve is ordered after the
 * caller's producers of its inputs and before their consumers.  NULL is HIP's
 * null (default) stream -- torch's default current stream.  socp_ctx_reset_stream
 * returns to the context's own stream.  Work already queued on the previous
 * stream stays ordered before later work (an event wait is inserted). */
int socp_ctx_set_stream(socp_ctx* ctx, void* stream);
int socp_ctx_reset_stream(socp_ctx* ctx);
/* tau of SOCP_F_DETECT_INFEASIBLE for every later solve on the context.  The
 * default is 1e-7 (CVXOPT's feastol).  A non-positive or NaN value returns
 * SOCP_E_INVALID and leaves the tolerance as it was. */
int socp_ctx_set_infeasibility_tol(socp_ctx* ctx, double tol);
/* Passes of the equilibration rule (socp_batch_equilibrate, SOCP_F_EQUILIBRATE)
 * for every later call on the context.  The default is 8: data spread over
 * 2^+-20 per row and column reaches the rule's fixed point in 6 passes and not
 * in 4.  A value < 1 or > 64 returns SOCP_E_INVALID and leaves the count as it was. */
int socp_ctx_set_equilibration_passes(socp_ctx* ctx, int passes);

/* 1 if a compiled kernel accepts the dims: the register-resident kernel (one
 * wavefront per problem, <= 8 cones, m <= 64; k <= 128 for n <= 48, k <= 96
 * for 48 < n <= 64: the compiled variant table, socp.jl_amd/csrc/gen_inst.py)
 * or the blocked kernel (n, m <= 2048, <= 64 cones, k <= 2^21 -- its
 * LDS / vector offsets are 32-bit; one 512-thread workgroup per problem), which
 * also takes every register-kernel shape.  The
 * blocked kernel keeps the problem's vectors in the 160 KiB LDS of a CU when
 * they fit (C4, n=512 m=64 k=640, uses 126 KiB) and in its HBM workspace slot
 * otherwise (e.g. k = 1000 at n = 512).  Other shapes return
 * SOCP_E_UNSUPPORTED from the solve entries.  Every entry rejects batch >
 * 2^31-1 (device problem indices are int32). */
int socp_supported(const socp_dims* dims);

/* Batched solve: replaces solve_socp(prob, SolverState(prob, DenseSolver(prob)))
 * (solver.jl:40-153 with the DenseSolver plugin, densesolver.jl:1-90), run once
 * per problem of the batch.
 *   cone_kind/offs/dim : ncones entries (POC first, then SOC), host pointers.
 *   c,A,b,G,h          : problem data (layout above).
 *   sing               : per-problem flag; 1 if cholesky(G'G) fails (Socp.jl:49-56).
 *                        NULL -> computed on device by the same positive-definiteness
 *                        test the kernel uses for H.
 *   x,y,z,s            : out (in as well with SOCP_F_WARM_START): final iterate
 *                        (the reference returns State(x,y,z,s), solver.jl:152).
 *   iters, status      : out, per problem (int32); iters = completed Newton steps.
 * With SOCP_F_DEVICE_PTRS the call is stream-ordered and returns without
 * synchronising; otherwise it copies, solves and synchronises.
 * Diagnostics: with SOCP_DUMP_DIR=<dir> in the environment, the first
 * SOCP_DUMP_COUNT (default 1) problems of every batch are written to
 * <dir>/problem<p>_{A,G,c,b,h,initv,cones}.txt, as the reference's commented
 * dumps do (solver.jl:48-67,75-82). */
int socp_batch_solve(socp_ctx* ctx, const socp_dims* dims,
                     const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                     const double* c, const double* A, const double* b,
                     const double* G, const double* h, const uint8_t* sing,
                     const socp_params* params,
                     double* x, double* y, double* z, double* s,
                     int32_t* iters, int32_t* status);

/* Same, plus per-problem final residual norms: res[3*p+0]=||rd||, [1]=||rp||, [2]=z's
 * (the quantities of the exit test, solver.jl:109-122), evaluated at the returned iterate. */
int socp_batch_solve_ex(socp_ctx* ctx, const socp_dims* dims,
                        const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                        const double* c, const double* A, const double* b,
                        const double* G, const double* h, const uint8_t* sing,
                        const socp_params* params,
                        double* x, double* y, double* z, double* s,
                        int32_t* iters, int32_t* status, double* res);

/* Quadratic objectives: minimise x'Px/2 + c'x subject to the same constraints.
 * Arguments as for socp_batch_solve_ex (res may be NULL), plus
 *   P : per problem n x n, column-major: P[p*n*n + j*n + i] = P_p(i,j).  It is
 *       read in full and must be symmetric positive semidefinite.  Neither is
 *       checked on the device: an unsymmetric P gives unspecified results, and
 *       a P that makes H indefinite gives SOCP_CHOL_H_FAILED for that problem
 *       only.  With SOCP_F_SHARED_MATRICES P is ONE n x n matrix, like A and G,
 *       and the results are the bits of the replicated call.
 * The method is that of socp_batch_solve_ex with two changes: the dual
 * residual is rd = Px + A'y + G'z + c wherever it appears (the exit test, the
 * right-hand sides, res[0]), and the reduced KKT matrix is
 * H = P + G'W^-2 G (+A'A when sing); the initial point solves the W = I
 * system with H0 = P + G'G (+A'A).  `sing` keeps its meaning (cholesky(G'G)
 * fails), and the sing == NULL probe factors G'G alone.  The reference already
 * takes one common step length for the primal and the dual (solver.jl:146-150),
 * as a QP requires.
 * P == NULL runs exactly what socp_batch_solve_ex runs (the same kernel, the
 * same bits).  Flags honoured: SOCP_F_DEVICE_PTRS (stream-ordered),
 * SOCP_F_WARM_START, SOCP_F_FORCE_LARGE, SOCP_F_SHARED_MATRICES.  With a P,
 * SOCP_F_EXPLICIT_INVERSE and SOCP_F_DETECT_INFEASIBLE return
 * SOCP_E_UNSUPPORTED (no QP kernel is compiled in the explicit-inverse order;
 * the unboundedness rule would need Px = 0 as well); socp_last_error says so.
 * The dims gate is socp_supported's.  The SOCP_DUMP_DIR dump also writes
 * problem<p>_P.txt. */
int socp_batch_solve_qp(socp_ctx* ctx, const socp_dims* dims,
                        const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                        const double* P, const double* c, const double* A, const double* b,
                        const double* G, const double* h, const uint8_t* sing,
                        const socp_params* params,
                        double* x, double* y, double* z, double* s,
                        int32_t* iters, int32_t* status, double* res);

/* Ruiz equilibration with power-of-two factors, on the device (the reference
 * has none).  Per matrix set, integer exponents ed[n], ee[m], ef[k] start at 0;
 * D = 2^ed, E = 2^ee, F = 2^ef.  Each of the context's passes
 * (socp_ctx_set_equilibration_passes, default 8):
 *   - scaled magnitudes ldexp(|A_ij|, ee_i + ed_j), ldexp(|G_ij|, ef_i + ed_j)
 *     and, with a P, ldexp(|P_ij|, ed_i + ed_j);
 *   - cn_j: the max over column j of all of them; ra_i, rg_i: the max over row
 *     i of A's and of G's; every row of an SOC cone gets the max of the cone's
 *     rg (one factor per cone: F s in K <=> s in K); POC rows stay individual;
 *   - a norm v that is finite and > 0 (subnormals included) gives
 *     t = -floor((ilogb(v) + 1) / 2), every other norm (zero rows and columns,
 *     Inf, NaN) t = 0;  ed += t(cn), ee += t(ra), ef += t(rg), each clamped to
 *     [-256, 256], all three from the same pass's norms.
 * At the fixed point every norm lies in [1/2, 2).  Outputs:
 *   D (MB x n), E (MB x m), F (MB x k) doubles, MB = 1 with
 *   SOCP_F_SHARED_MATRICES and batch otherwise;
 *   Ps = D P D, As = E A D, Gs = F G D (the layout of the inputs);
 *   cs = D c, bs = E b, hs = F h (per problem; the one factor set when shared).
 * Every scaled value is ldexp(value, sum of the exponents): exact, up to one
 * rounding where a result is subnormal.
 * P, and A when m = 0, may be NULL.  Any output pointer may be NULL and is then
 * skipped; c, b, h may be NULL together with their outputs.  The inputs are
 * not written.  flags: SOCP_F_DEVICE_PTRS (stream-ordered, no synchronisation)
 * | SOCP_F_SHARED_MATRICES.  The dims gate is socp_supported's. */
int socp_batch_equilibrate(socp_ctx* ctx, const socp_dims* dims,
                           const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                           const double* P, const double* c, const double* A, const double* b,
                           const double* G, const double* h, int32_t flags,
                           double* D, double* E, double* F,
                           double* Ps, double* cs, double* As, double* bs, double* Gs, double* hs);

/* SOCP_F_NORMALISE's rule (above) on the device: the two exponents of every
 * problem and the scaled data.  Outputs:
 *   expo : 2 * batch int32, expo[2p] = ec and expo[2p+1] = eb of problem p --
 *          always 2 * batch entries, all equal in the shared-P case;
 *   Ps = ldexp(P, ec - eb) (the layout of P: ONE matrix with
 *        SOCP_F_SHARED_MATRICES, which then takes the batch-wide pair);
 *   cs = ldexp(c, ec), bs = ldexp(b, eb), hs = ldexp(h, eb), per problem.
 * Every scaled value is exact, up to one rounding where a result is subnormal.
 * P may be NULL, and b when m = 0.  Any output pointer may be NULL and is then
 * skipped.  The inputs are not written.  flags: SOCP_F_DEVICE_PTRS
 * (stream-ordered, no synchronisation) | SOCP_F_SHARED_MATRICES.  Only batch,
 * n, m and k of dims are read (batch > 2^31-1 is rejected as everywhere). */
int socp_batch_normalise(socp_ctx* ctx, const socp_dims* dims,
                         const double* P, const double* c, const double* b, const double* h,
                         int32_t flags, int32_t* expo,
                         double* Ps, double* cs, double* bs, double* hs);

/* Single-problem plugin entries.  They replace the two KKTSolver methods of
 * DenseSolver so the reference's own KKT golden (runtests.jl:95-128) runs
 * through the HIP path:
 *   setup_iter(ss::DenseSolver, pr, state, scaling)   densesolver.jl:41-52
 *   solve_kkt (ss::DenseSolver, pr, state, scaling, dx,dy,dz,ds, cx,cy,cz,cs)   densesolver.jl:54-90
 * Here both happen in one device call on a batch: given the iterate (s,z) the
 * NT scaling is computed (scalings.jl:101-110), the KKT matrix factored, and the
 * system solved for the right-hand side (dx,dy,dz,ds) -> (cx,cy,cz,cs).
 * kkt_status[p]: 0 ok, SOCP_CHOL_H_FAILED, SOCP_CHOL_S_FAILED, SOCP_DOMAIN_ERROR. */
int socp_batch_kkt_solve(socp_ctx* ctx, const socp_dims* dims,
                         const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                         const double* A, const double* G, const uint8_t* sing,
                         const double* s, const double* z,
                         const double* dx, const double* dy, const double* dz, const double* ds,
                         double* cx, double* cy, double* cz, double* cs,
                         int32_t* kkt_status, int32_t flags);  /* flags: SOCP_F_DEVICE_PTRS | SOCP_F_FORCE_LARGE | SOCP_F_SHARED_MATRICES */

/* socp_batch_kkt_solve for a quadratic objective (socp_batch_solve_qp's P: per
 * problem n x n column-major, ONE matrix with SOCP_F_SHARED_MATRICES; symmetric
 * positive semidefinite, unchecked).  The first row of the block system
 * becomes
 *     P cx + A'cy + G'cz = dx
 * and the other three stay (A cx = dy, G cx + cs = dz, lam o (W cz + W^-T cs)
 * = ds): the reduced matrix is H = P + G'W^-2 G (+A'A when sing) and nothing
 * else of solve_kkt changes.  A P that leaves H indefinite gives that problem
 * alone SOCP_CHOL_H_FAILED and a NaN solution (what socp_dense_solve_kkt
 * returns after a failed setup_iter).  The sing == NULL probe factors G'G
 * without P, as the solver's does.
 * P == NULL runs exactly what socp_batch_kkt_solve runs (the same kernel, the
 * same bits).  flags: SOCP_F_DEVICE_PTRS | SOCP_F_FORCE_LARGE |
 * SOCP_F_SHARED_MATRICES; with a P, SOCP_F_EXPLICIT_INVERSE returns
 * SOCP_E_UNSUPPORTED (no QP kernel is compiled in that order, as for the
 * solver) and socp_last_error names this entry. */
int socp_batch_kkt_solve_qp(socp_ctx* ctx, const socp_dims* dims,
                            const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                            const double* P, const double* A, const double* G, const uint8_t* sing,
                            const double* s, const double* z,
                            const double* dx, const double* dy, const double* dz, const double* ds,
                            double* cx, double* cy, double* cz, double* cs,
                            int32_t* kkt_status, int32_t flags);

/* Differentiable solves (the reference has none).  The gradient
 * of a solve is the adjoint of the block system above -- exactly so at a point
 * of the central path (s o z = mu e), which a solver's returned iterate is not:
 * Mehrotra steps of length 0.99 leave it off-centre by its own size.  So there
 * are two entries: one centres an iterate, one forms the adjoint at a point.
 *
 * socp_batch_centre: `steps` (0..16) pure Newton centring passes on (x, y, z, s),
 * in place.  Each pass, per problem:
 *   1. mu = s'z / deg, deg = POC rows + SOC cones;
 *   2. lam = compute_scaling's l at (s, z) (scalings.jl:22-99; IEEE sqrt and /);
 *   3. dx = -(Px + c + A'y + G'z), dy = -(Ax - b), dz = -(Gx + s - h),
 *      ds = mu e - lam o lam   (no Mehrotra term; the residuals stay in);
 *   4. one socp_batch_kkt_solve_qp at (s, z) on that right-hand side (P == NULL:
 *      socp_batch_kkt_solve's kernels), chosen and launched as a caller's own;
 *   5. t = 1, halved while z + t cz or s + t cs is not interior (POC entries
 *      > 0, SOC v0 > sqrt(sum_{i>=1} v_i^2)), given up below 2^-30;
 *   6. (x, y, z, s) += t (cx, cy, cz, cs).
 * The last pass refines its step once before 5: the residual of the three
 * linear rows at (cx, cy, cz, cs), with ds = 0, goes through the same entry
 * again and the result is added.  The kernels' solve leaves those rows a
 * residual of its own accuracy times the step (1e-12 .. 1e-9 on ill-conditioned
 * late iterates); with the refinement the returned point satisfies
 * Px + c + A'y + G'z = 0, Ax = b, Gx + s = h to the rounding of their terms.
 * So `steps` passes cost steps + 1 KKT solves.
 * status[p]: 0; the KKT solve's status; or SOCP_DOMAIN_ERROR where no t is
 * found.  Such a problem stops at its last good iterate and the others go on.
 * res (4 per problem, may be NULL): ||rd||_2, ||rp||_2, z's and the off-centre
 * measure ||lam o lam - mu e||_2 / mu at the returned point.  steps = 0 returns
 * the iterate's bits and its res.  P may be NULL; sing as in socp_batch_solve.
 * For a `sing` problem dy = -rp != 0, where the sing formula is not the block
 * system's solve (socp_batch_kkt_solve above: its cx leaves A cx - dy of dy's
 * size); as in the solver that is harmless once rp is small, and it is left so.
 * flags: SOCP_F_DEVICE_PTRS (stream-ordered, no synchronisation) |
 * SOCP_F_FORCE_LARGE | SOCP_F_SHARED_MATRICES (one P, A, G and sing byte; the
 * outputs are the bits of the replicated call).  SOCP_F_EXPLICIT_INVERSE
 * returns SOCP_E_UNSUPPORTED, every other bit SOCP_E_INVALID. */
int socp_batch_centre(socp_ctx* ctx, const socp_dims* dims,
                      const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                      const double* P, const double* c, const double* A, const double* b,
                      const double* G, const double* h, const uint8_t* sing,
                      int32_t steps, int32_t flags,
                      double* x, double* y, double* z, double* s,
                      int32_t* status, double* res);

/* The adjoint at a given point (x, y, z, s); no centring.  gx, gy, gz, gs are
 * the upstream gradients dL/d(x, y, z, s), each may be NULL meaning zero.
 * Definition:
 *   Solve the block system of socp_batch_kkt_solve_qp at (s, z) with the
 *   right-hand side (dx, dy, dz, ds) = (gx - G'gs, gy, gz, 0).  Call the
 *   solution (ux, uy, uz, .) and set w = uz + gs.  Then
 *     dc = -ux        db = uy         dh = w
 *     dP = -(ux x' + x ux')/2
 *     dA = -(y ux' + uy x')
 *     dG = -(z ux' + w x')
 * (the gs term uses row 3 of the system, ds = dh - dG x - G dx, so no scaling
 * matrix is needed outside the KKT kernel).  Outputs, each may be NULL and is
 * then skipped: dc[B n], db[B m], dh[B k]; dP[B n^2], dA[B m n], dG[B k n],
 * column-major as the inputs; the adjoint variables ux[B n], uy[B m], uz[B k].
 * skip (int32 per problem, may be NULL): a problem with skip[p] != 0, or whose
 * KKT solve fails, gets zeros in every output -- never NaN, so that a sum over
 * the batch stays finite -- and status[p] = skip[p], or else the KKT status.
 * For a `sing` problem a nonzero gy is not supported: the sing formula is not
 * the block system's solve when dy != 0.
 * flags: SOCP_F_DEVICE_PTRS | SOCP_F_FORCE_LARGE; SOCP_F_SHARED_MATRICES (one
 * P, A, G, sing) only while dP, dA and dG are NULL -- with one of them it
 * returns SOCP_E_UNSUPPORTED (those are sums over the batch, which
 * socp_batch_vjp_sum below forms);
 * SOCP_F_EXPLICIT_INVERSE returns SOCP_E_UNSUPPORTED, every other bit
 * SOCP_E_INVALID. */
int socp_batch_vjp(socp_ctx* ctx, const socp_dims* dims,
                   const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                   const double* P, const double* A, const double* G, const uint8_t* sing,
                   const double* x, const double* y, const double* z, const double* s,
                   const double* gx, const double* gy, const double* gz, const double* gs,
                   const int32_t* skip, int32_t flags,
                   double* dc, double* db, double* dh, double* dP, double* dA, double* dG,
                   double* ux, double* uy, double* uz, int32_t* status);

/* The adjoint of a shared-matrix batch with the gradients of its ONE P, A and
 * G.  P, A, G are ONE matrix each and sing ONE byte or NULL, and
 * SOCP_F_SHARED_MATRICES must be set (without it: SOCP_E_INVALID).  dc, db, dh,
 * ux, uy, uz and status are per problem and bitwise those of socp_batch_vjp
 * with SOCP_F_SHARED_MATRICES on the same inputs (the same kernels, launched
 * the same way).  dP[n^2], dA[m n], dG[k n], column-major, are the sums of the
 * per-problem outer products over the problems that count, on(p) meaning
 * status[p] == 0, with w_p = fl(uz_p + gs_p) (the bits of dh_p):
 *     dG = -sum_{on(p)} (z_p ux_p' + w_p x_p')
 *     dA = -sum_{on(p)} (y_p ux_p' + uy_p x_p')
 *     dP = -(M + M')/2,   M = sum_{on(p)} ux_p x_p'
 * A problem with skip[p] != 0 or a failed KKT solve contributes nothing (its
 * terms are selected away, not multiplied by zero: the sums stay finite).  dP
 * is symmetric in bits.  Each of dP, dA, dG may be NULL and is then skipped;
 * dA is skipped when m = 0; with all three NULL the call is socp_batch_vjp's.
 * The sums are deterministic: the same bits from run to run, with host or
 * device pointers, and whichever other outputs are asked for.  The batch is
 * cut into slabs of consecutive problems by a rule that depends on (batch, n,
 * m, k) alone (socp_debug_vjp_sum_plan); one launch writes each
 * slab's partial sums, a second adds them in ascending slab order.  No atomics.
 * flags: SOCP_F_SHARED_MATRICES, with SOCP_F_DEVICE_PTRS (stream-ordered, no
 * synchronisation) and SOCP_F_FORCE_LARGE allowed; SOCP_F_EXPLICIT_INVERSE
 * returns SOCP_E_UNSUPPORTED, every other bit SOCP_E_INVALID. */
int socp_batch_vjp_sum(socp_ctx* ctx, const socp_dims* dims,
                       const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                       const double* P, const double* A, const double* G, const uint8_t* sing,
                       const double* x, const double* y, const double* z, const double* s,
                       const double* gx, const double* gy, const double* gz, const double* gs,
                       const int32_t* skip, int32_t flags,
                       double* dc, double* db, double* dh, /* per problem, as socp_batch_vjp */
                       double* dP, double* dA, double* dG, /* ONE n x n, m x n, k x n */
                       double* ux, double* uy, double* uz, int32_t* status);

/* The same two methods split the way the reference's KKTSolver plugin is
 * (densesolver.jl): a handle stands for a batch of DenseSolver objects.
 *   socp_dense_create      replaces DenseSolver(...) construction
 *                          (densesolver.jl:9-39): A and G (and sing, or NULL
 *                          for the cholesky(G'G) test at every setup) are
 *                          copied into the handle once;
 *   socp_dense_setup_iter  replaces setup_iter(ss, pr, state, scaling)
 *                          (densesolver.jl:41-52): NT scaling of (s, z), H and
 *                          its factorisation, kept on the device as one factor
 *                          record per problem.  By default the record holds
 *                          the Cholesky factor of H (register kernel, m <= 16:
 *                          16x16 tiles, L_PP^-1 on the diagonal; blocked
 *                          kernel: L in place, L_PP^-1 in the diagonal
 *                          blocks), Z = L^-1 A' and S^-1 for S = Z'Z =
 *                          A H^-1 A' (blocked kernel: the Cholesky factor of
 *                          S, applied by two triangular solves, here and in
 *                          socp_batch_kkt_solve); H^-1 itself is never formed.  Where m > 16
 *                          on the register kernel, or with
 *                          SOCP_F_EXPLICIT_INVERSE, it holds Li = H^-1, A Li
 *                          (or Li A') and S^-1, as densesolver.jl:48-51 do;
 *                          status[p]: 0, SOCP_CHOL_H_FAILED,
 *                          SOCP_CHOL_S_FAILED or SOCP_DOMAIN_ERROR (where the
 *                          reference throws PosDefException / DomainError);
 *   socp_dense_solve_kkt   replaces solve_kkt(ss, ...) (densesolver.jl:54-90)
 *                          against the last setup_iter; call it any number of
 *                          times (the solver calls it twice per iteration,
 *                          solver.jl:125-145).  status[p] = 0, or setup_iter's
 *                          status with NaN outputs for a problem whose setup
 *                          failed.
 * flags (at create, for all calls of the handle): SOCP_F_DEVICE_PTRS (every
 * pointer, A and G included, is a device pointer; the calls are then
 * stream-ordered on the context's stream and return without synchronising) |
 * SOCP_F_FORCE_LARGE | SOCP_F_SHARED_MATRICES.  With host pointers each setup_iter moves 2k doubles
 * per problem host-to-device and each solve_kkt n+m+2k; A and G move once, at
 * create (socp_dense_h2d_bytes reports the last call's count).  The results are
 * bitwise those of socp_batch_kkt_solve on the same inputs.  Device memory:
 * socp_dense_record_bytes() per problem plus A, G.
 *   socp_dense_create_qp   the same handle for a quadratic objective: P (as in
 *                          socp_batch_kkt_solve_qp) is copied into the handle
 *                          beside A and G and counted by socp_dense_h2d_bytes at
 *                          create; setup_iter factors H = P + G'W^-2 G (+A'A)
 *                          (where the record holds Li it is the inverse of that
 *                          H), solve_kkt reads the record alone.  Results are
 *                          bitwise those of socp_batch_kkt_solve_qp.  P == NULL
 *                          is socp_dense_create; with a P,
 *                          SOCP_F_EXPLICIT_INVERSE returns SOCP_E_UNSUPPORTED
 *                          and socp_last_error names this entry. */
typedef struct socp_dense socp_dense;
int socp_dense_create(socp_ctx* ctx, const socp_dims* dims,
                      const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                      const double* A, const double* G, const uint8_t* sing, int32_t flags,
                      socp_dense** out);
int socp_dense_create_qp(socp_ctx* ctx, const socp_dims* dims,
                         const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                         const double* P, const double* A, const double* G, const uint8_t* sing,
                         int32_t flags, socp_dense** out);
int socp_dense_setup_iter(socp_dense* h, const double* s, const double* z, int32_t* status);
int socp_dense_solve_kkt(socp_dense* h, const double* dx, const double* dy, const double* dz,
                         const double* ds, double* cx, double* cy, double* cz, double* cs,
                         int32_t* status);
int socp_dense_h2d_bytes(const socp_dense* h, int64_t* bytes);
int64_t socp_dense_record_bytes(const socp_dense* h);
int socp_dense_destroy(socp_dense* h);

/* The rank-update plugin: SparseSolver with SqrScaling (spsolver.jl:1-130,
 * sqrscalings.jl:8-214), the solver the reference's own tests and MOI run.
 *   socp_sqr_create      replaces SparseSolver(pr) (spsolver.jl:24-57): A, G
 *                        and sing (the Problem's type parameter; NULL = no
 *                        problem is sing) copied into the handle once;
 *   socp_sqr_setup_iter  replaces compute_scaling(cones, ::SqrScaling, s, z)
 *                        (sqrscalings.jl:177-185) + setup_iter(::SparseSolver)
 *                        (spsolver.jl:60-84): W^-2 = D + uu' - vv' per SOC cone,
 *                        L L' = G'DG (+A'A when sing), one rank-1 update with
 *                        G'u and one downdate with G'v per SOC cone
 *                        (modify_factors!, sqrscalings.jl:160-194), and the
 *                        factor of S = (L^-1 A')'(L^-1 A'); status[p] as for
 *                        socp_dense_setup_iter (a downdate that loses positive
 *                        definiteness is SOCP_CHOL_H_FAILED);
 *   socp_sqr_solve_kkt   replaces solve_kkt(::SparseSolver) (spsolver.jl:86-130)
 *                        by triangular solves against the record;
 *   socp_sqr_factor      problem p's factor L of H after the modifications
 *                        (n x n, column-major, zeros above the diagonal): the
 *                        Gfact CHOLMOD factor of spsolver.jl:13 as a dense matrix;
 *   socp_sqr_scaling     the SqrScaling fields l, wbs, mu (B x k, B x k,
 *                        B x ncones) of the last setup_iter.
 * CHOLMOD's fill-reducing permutation and supernodal LDL' are replaced by a
 * dense factor: results agree with the reference to rounding, not bitwise.
 * Shapes: n, m <= 1024, k <= 4096, <= 64 cones, the problem's vectors
 * within 160 KiB of LDS (socp_sqr_supported): one wavefront per problem for
 * n, m <= 64, one 256-thread workgroup above -- its factors packed in LDS,
 * or in the per-problem record when they and a right-hand-side chunk exceed
 * the LDS (n, m beyond about 160).  Flags and
 * host/device pointer semantics as socp_dense_*. */
typedef struct socp_sqr socp_sqr;
int socp_sqr_supported(const socp_dims* dims);
int socp_sqr_create(socp_ctx* ctx, const socp_dims* dims,
                    const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                    const double* A, const double* G, const uint8_t* sing, int32_t flags,
                    socp_sqr** out);
int socp_sqr_setup_iter(socp_sqr* h, const double* s, const double* z, int32_t* status);
int socp_sqr_solve_kkt(socp_sqr* h, const double* dx, const double* dy, const double* dz,
                       const double* ds, double* cx, double* cy, double* cz, double* cs,
                       int32_t* status);
int socp_sqr_factor(socp_sqr* h, int64_t problem, double* L);
int socp_sqr_scaling(socp_sqr* h, double* l, double* wbs, double* mu);
/* solve_socp(prob, SolverState(prob, SparseSolver(prob))) (solver.jl:40-153)
 * for the handle's whole batch -- the reference's own tested configuration
 * (runtests.jl:143-144, 188-189, 204-244) -- with this plugin's setup_iter /
 * solve_kkt: initial point (the KKT system with W = I and the cone shift,
 * solver.jl:68-104), then up to params->maxit iterations with the reference's
 * exit test, per-problem status and masking (problems that stop are skipped by
 * every later launch).  c (B x n), b (B x m), h (B x k) in; x, y, z, s, iters,
 * status, res (B x 3: ||rd||, ||rp||, z's at the returned iterate; may be
 * NULL) out.  params NULL: socp_params_default.  Host or device pointers as
 * the handle's flags.  Afterwards the records hold the last factorisation.
 * With tol > 0 the call synchronises its stream every 4 iterations to stop
 * launching once every problem has stopped (converged or failed); such a call
 * cannot be captured into a HIP graph.  With tol <= 0 (fixed iteration count)
 * it issues only stream-ordered work until the final copies.
 * params->flags: SOCP_F_DETECT_INFEASIBLE (statuses 5 and 6 stop a problem
 * like every other status; its res[] is the exit test's, from before the
 * certificate was scaled).
 * The initial point factors G'G (+ A'A where sing) with W = I: `sing` must be
 * the flag Problem() computes (Socp.jl:49-56, cholesky(G'G) fails).  Where the
 * given flag disagrees and that factorisation fails, the problem stops with
 * status SOCP_CHOL_H_FAILED at iteration 0 -- the reference's sparse `\`
 * (solver.jl:84) would solve the full KKT system instead. */
int socp_sqr_solve_socp(socp_sqr* h, const double* c, const double* b, const double* hvec,
                        const socp_params* params, double* x, double* y, double* z, double* s,
                        int32_t* iters, int32_t* status, double* res);
int socp_sqr_h2d_bytes(const socp_sqr* h, int64_t* bytes);
int64_t socp_sqr_record_bytes(const socp_sqr* h);
int socp_sqr_destroy(socp_sqr* h);

/* Device-side deterministic generator of feasible synthetic problems
 * (SURVEY.md §8(d)): counter-based SplitMix64 keyed on the GLOBAL problem
 * index first_problem + p, so shards of a multi-GPU run reproduce the same
 * problems.  Output pointers are device pointers with the layout above. */
int socp_generate(socp_ctx* ctx, const socp_dims* dims,
                  const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                  uint64_t seed, int64_t first_problem,
                  double* c, double* A, double* b, double* G, double* h);

/* Ingest: pack a batch of sparse matrices in Julia's
 * SparseMatrixCSC form -- the storage of Problem.A and Problem.G
 * (Socp.jl:25,29) -- into the dense column-major batch layout above, on the
 * device.  Every matrix is rows x cols.  Problem p's nonzeros are
 * nz_offs[p] .. nz_offs[p+1]-1 of rowval/nzval; its column pointer is
 * colptr[p*(cols+1) .. p*(cols+1)+cols] (relative to nz_offs[p]).  Indices are
 * int64 with index_base 1 (Julia, zero-copy) or 0.  All pointers are device
 * pointers; dense[p*rows*cols + j*rows + i] is written for every element
 * (zeros included).  Duplicate (i,j) entries are summed, as sparse() does.
 * Returns SOCP_E_INVALID (after synchronising) if any row index or column
 * pointer is out of range; nothing else is validated. */
int socp_pack_csc(socp_ctx* ctx, int64_t batch, int32_t rows, int32_t cols,
                  const int64_t* nz_offs, const int64_t* colptr, const int64_t* rowval,
                  const double* nzval, int32_t index_base, double* dense);

/* Pipelined ingest of host-resident batches: the
 * reference builds each Problem on the host (Socp.jl:20-60); here a stream of
 * host batches flows through two slots of pinned (hipHostMalloc) staging so
 * batch i+1's host-to-device copy -- and, in the CSC form, its packing --
 * runs on a copy stream while batch i solves on the context's stream, and
 * batch i's results drain to pinned memory on a third stream.
 *   socp_ingest_create(ctx, dims, cones..., flags, &ing): dims.batch is the
 *       largest batch one submit may carry (pinned + device space for two
 *       such batches is allocated here); flags: SOCP_F_FORCE_LARGE |
 *       SOCP_F_SHARED_MATRICES.
 *   socp_ingest_submit(ing, B, c, A, b, G, h, sing, params, &ticket): host
 *       arrays in the batch layout above, copied into the slot's pinned
 *       block (no copy for arrays already written at the pointers
 *       socp_ingest_next_inputs returns), then everything is asynchronous.
 *       Of params->flags, SOCP_F_EXPLICIT_INVERSE and
 *       SOCP_F_DETECT_INFEASIBLE are honoured (together: SOCP_E_UNSUPPORTED,
 *       before the slot is claimed); there is no warm start.
 *   socp_ingest_submit_csc(...): A and G as the SparseMatrixCSC arrays of
 *       socp_pack_csc (host pointers; nz_offs[B] - nz_offs[0] nonzeros each),
 *       packed on the device on the copy stream.
 *   socp_ingest_wait(ing, ticket, x, y, z, s, iters, status, res): blocks
 *       until that batch's results are on the host and copies them out (res
 *       may be NULL).  A CSC batch with bad indices returns SOCP_E_INVALID here.
 * At most two tickets are outstanding: a third submit before the oldest is
 * waited for returns SOCP_E_INVALID.  Results are bitwise those of
 * socp_batch_solve_ex on the same inputs.
 * With SOCP_F_SHARED_MATRICES in socp_ingest_create's flags the slots hold no
 * A, G or sing staging (the pinned and device blocks shrink accordingly):
 *   socp_ingest_set_matrices(ing, A, G, sing): the one m x n A, k x n G and
 *       sing byte (NULL: the device probe) of every later batch.  Host
 *       pointers; the copy is synchronous.  Allowed only with no ticket
 *       outstanding (SOCP_E_INVALID otherwise); may be called again between
 *       batches.  SOCP_E_INVALID on an ingest created without the flag.
 *   socp_ingest_submit then requires A, G and sing to be NULL and
 *       set_matrices to have been called (SOCP_E_INVALID otherwise);
 *       socp_ingest_next_inputs hands back NULL for A, G and sing;
 *       socp_ingest_submit_csc returns SOCP_E_INVALID.
 * Quadratic objectives (socp_batch_solve_qp's P; dense only, no CSC form):
 *   socp_ingest_submit_qp(ing, B, P, c, A, b, G, h, sing, params, &ticket):
 *       socp_ingest_submit with the batch's B matrices P; results are bitwise
 *       those of socp_batch_solve_qp on the same inputs.  The slots' pinned
 *       and device room for P is allocated by the first call that brings a P
 *       (this one or socp_ingest_next_P); that call may synchronise the
 *       device once.  P == NULL is socp_ingest_submit, and so is any later
 *       plain submit: the linear solve, bit for bit.  With a P,
 *       SOCP_F_EXPLICIT_INVERSE or SOCP_F_DETECT_INFEASIBLE in params->flags
 *       returns SOCP_E_UNSUPPORTED before the slot is claimed, as the
 *       synchronous entry refuses them.
 *   socp_ingest_next_P(ing, &P): the next slot's pinned P block (max_batch
 *       matrices), to be written in place like socp_ingest_next_inputs'
 *       arrays; allocates as above.  SOCP_E_INVALID on a shared ingest.
 *   socp_ingest_set_matrices_qp(ing, P, A, G, sing): socp_ingest_set_matrices
 *       with the one n x n P of a SOCP_F_SHARED_MATRICES ingest (P == NULL:
 *       none).  socp_ingest_submit_qp on such an ingest requires its own P to
 *       be NULL and a set_matrices_qp that gave one (SOCP_E_INVALID
 *       otherwise) and solves with it; socp_ingest_submit stays the linear
 *       solve; plain socp_ingest_set_matrices clears the P. */
typedef struct socp_ingest socp_ingest;
int socp_ingest_create(socp_ctx* ctx, const socp_dims* dims,
                       const int32_t* cone_kind, const int32_t* cone_offs, const int32_t* cone_dim,
                       int32_t flags, socp_ingest** out);
int socp_ingest_set_matrices(socp_ingest* ing, const double* A, const double* G, const uint8_t* sing);
int socp_ingest_next_inputs(socp_ingest* ing, double** c, double** A, double** b, double** G,
                            double** h, uint8_t** sing);
int socp_ingest_submit(socp_ingest* ing, int64_t batch, const double* c, const double* A,
                       const double* b, const double* G, const double* h, const uint8_t* sing,
                       const socp_params* params, int64_t* ticket);
int socp_ingest_submit_qp(socp_ingest* ing, int64_t batch, const double* P, const double* c,
                          const double* A, const double* b, const double* G, const double* h,
                          const uint8_t* sing, const socp_params* params, int64_t* ticket);
int socp_ingest_set_matrices_qp(socp_ingest* ing, const double* P, const double* A, const double* G,
                                const uint8_t* sing);
int socp_ingest_next_P(socp_ingest* ing, double** P);
int socp_ingest_submit_csc(socp_ingest* ing, int64_t batch, const double* c, const double* b,
                           const double* h, const uint8_t* sing,
                           const int64_t* A_nz_offs, const int64_t* A_colptr, const int64_t* A_rowval,
                           const double* A_nzval,
                           const int64_t* G_nz_offs, const int64_t* G_colptr, const int64_t* G_rowval,
                           const double* G_nzval, int32_t index_base, const socp_params* params,
                           int64_t* ticket);
int socp_ingest_wait(socp_ingest* ing, int64_t ticket, double* x, double* y, double* z, double* s,
                     int32_t* iters, int32_t* status, double* res);
int socp_ingest_destroy(socp_ingest* ing);

/* Multi-GPU outcome gather: problems shard across ranks
 * (one process per GPU) with no data-path exchange; the only collective is the
 * all-gather of each problem's (status, iters) over RCCL (xGMI between the
 * GPUs of a node).  This replaces nothing in the reference (which solves one
 * problem per call, solver.jl:40); it is the exchange step of the batched
 * multi-GPU drop-in.  RCCL (librccl.so.1) is opened on first use, so the rest
 * of the library has no RCCL dependency.
 *   rank 0: socp_comm_unique_id(id), then hands the 128 bytes to every rank
 *           (MPI broadcast, a file, torch.distributed ...);
 *   every rank: socp_comm_init(ctx, nranks, rank, id, &comm);
 *   socp_allgather_status(comm, B, status, iters, out): device pointers;
 *           out[(r*B + p)*2 + 0] = status, [.. + 1] = iters of rank r's
 *           problem p; equal B on every rank; stream-ordered on the
 *           context's stream (socp_ctx_sync to wait). */
#define SOCP_COMM_ID_BYTES 128
typedef struct socp_comm socp_comm;
int socp_comm_unique_id(unsigned char* id);
int socp_comm_init(socp_ctx* ctx, int nranks, int rank, const unsigned char* id, socp_comm** out);
int socp_comm_destroy(socp_comm* comm);
int socp_allgather_status(socp_comm* comm, int64_t batch, const int32_t* status, const int32_t* iters,
                          int32_t* out);
/* The SURVEY.md §8(e) record: per problem 32 bytes -- status, iters and the
 * exit-test quantities ||rd||, ||rp||, z's at the returned iterate
 * (solver.jl:109-122; res[] of socp_batch_solve_ex, NaN where res is NULL).
 * out[r*B + p] is rank r's problem p; device pointers; stream-ordered.  A comm
 * must be destroyed before the context it was created on. */
typedef struct socp_outcome {
  int32_t status;
  int32_t iters;
  double res_dual;   /* ||A'y + G'z + c|| */
  double res_primal; /* ||Ax - b||        */
  double gap;        /* z's               */
} socp_outcome;
int socp_allgather_outcomes(socp_comm* comm, int64_t batch, const int32_t* status, const int32_t* iters,
                            const double* res, socp_outcome* out);

/* Timing of the last solve's main kernel, measured with HIP events on the
 * context's stream (milliseconds), and its name.  socp_last_kernel_ms waits
 * for that launch. */
int socp_last_kernel_ms(socp_ctx* ctx, float* ms);
const char* socp_last_kernel_name(socp_ctx* ctx);
/* The main-kernel times of the context's last min(n, 64) timed launches,
 * oldest first, into ms[]; returns how many were written (< 0: error).  Each
 * launch records its own event pair, so a run of launches is timed without a
 * host synchronisation between them (bench.py's timed steps); the call waits
 * for the newest one. */
int socp_kernel_times(socp_ctx* ctx, float* ms, int n);

/* Testing hook (not part of the reference surface; diagnostic build
 * libsocp_diag.so only): when set to a device buffer of
 * batch*(2n^2+2k+nm+m^2) doubles, socp_batch_kkt_solve on the register kernel
 * dumps per problem the KKT matrix H = G'W^-2G (+A'A) (densesolver.jl:43-46),
 * its inverse Li (:48), lambda and wbar (scalings.jl:1-20), Li A' and S --
 * on the explicit-inverse path only (m > 16, or SOCP_F_EXPLICIT_INVERSE): the
 * default Cholesky path never forms Li and dumps nothing.  NULL disables. */
int socp_debug_set_kkt_dump(double* dev_buf);

/* Diagnostic hook: device buffer of 13 uint64 counters; in the phase-stamp build
 * (libsocp_stamps.so, -DSOCP_STAMPS) every solve adds per-phase shader-clock
 * cycles (load, scaling, residuals, U, SYRK, sweep(H), Schur, solve, step, init,
 * store, other) and the executed iterations.  The product build ignores it. */
int socp_debug_set_stamps(unsigned long long* dev_buf);

/* Testing hook (host only, no device work): the slot plan a plain solve of
 * this cone table takes on the register-resident kernel when k > 64 (the
 * table is checked as a solve checks it).  The cone vector operations hold a
 * k-vector as two 64-lane slots; slot s, lane l holds element
 * (64 s + l - rot) mod k, rot 0 or 64.  kind0 / kind1: 0 mixed, 1 all SOC,
 * 2 all POC -- both slots are pure, and the solver kernel compiled for that
 * pair runs, or both are reported mixed and rot is 0.  The environment variable
 * SOCP_SLOT_SPECIALISE=0 (read at every launch and by this call) forces rot = 0
 * and the mixed kernel; the results are the same bits. */
int socp_debug_slot_plan(const socp_dims* dims, const int32_t* kind, const int32_t* offs,
                         const int32_t* dim, int32_t* rot, int32_t* kind0, int32_t* kind1);

/* Testing hook (host only, no device work): does socp_batch_solve with these
 * dims, this cone table (checked as a solve checks it) and these socp_params
 * flags run an exact-fit kernel -- the pure-slot plain solver compiled for one
 * launch geometry, dims, cone layout and slot plan as constants?  *exact = 1
 * only when the plain solver runs (neither SOCP_F_EXPLICIT_INVERSE nor
 * SOCP_F_DETECT_INFEASIBLE; warm starts and shared matrices do not matter),
 * the slot plan chose a pure pair, n, m and k fill the compiled variant
 * exactly, the cone table is the one the kernel holds, the SYRK's cone rows
 * are fused (`sing` may be given or left to the device).  The one geometry compiled
 * is n = 64, m = 16, k = 96 with POC(0, 32), SOC(32, 32), SOC(64, 32).
 * SOCP_EXACT_FIT=0, SOCP_FUSE_U=0 or SOCP_SLOT_SPECIALISE=0 in the environment
 * (read at every launch and by this call) give 0: the generic kernel runs, and
 * the results are the same bits. */
int socp_debug_exact_fit(const socp_dims* dims, const int32_t* kind, const int32_t* offs,
                         const int32_t* dim, int32_t flags, int32_t* exact);

/* Testing hook (host only, no device work): how socp_batch_vjp_sum cuts a batch
 * of dims->batch >= 1 problems of this n, m, k (ncones is not read): *slabs runs
 * of *slab_problems consecutive problems, the last one ragged.  slab_problems
 * is 512, doubled while there is more than one slab and the partial sums,
 * slabs * (k n + m n + n^2) doubles, would pass 64 MiB. */
int socp_debug_vjp_sum_plan(const socp_dims* dims, int64_t* slabs, int64_t* slab_problems);

#ifdef __cplusplus
}
#endif
#endif /* SOCP_H */
