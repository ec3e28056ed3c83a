// socp_small.hpp — the register-resident batched dense SOCP IPM kernel (gfx950).
//
// One 64-lane wavefront owns one problem for its whole solve (persistent
// one-wave blocks pull problem indices from an atomic work counter).  The
// problem's G (k x n, the dominant data: 48 KiB at n=64,k=96) is loaded from
// HBM once per solve and stays in AGPRs for every iteration, laid out as the
// B-operand fragment of v_mfma_f64_16x16x4_f64:
//     lane (g = lane>>4, cl = lane&15) holds G[4p+g][16q+cl] in G[p][q].
// Per iteration (reference solver.jl:105-151):
//   - NT scaling (scalings.jl:22-110) with per-cone segmented DPP scans;
//   - residuals (solver.jl:110-122) from register G;
//   - H = X'X with X = W^-1 G generated in registers and contracted by f64
//     MFMA: the reference's iWiW GEMM, G'*iWiW and *G (scalings.jl:108,
//     densesolver.jl:42-43) done structurally; +A'A if sing (:44-46);
//   - H = L L' by an in-register blocked Cholesky factorisation on 16x16
//     tiles (factor_tile), failing where cholesky! would.  m <= 16: Z = L^-1 A'
//     and S = Z'Z, Li never formed (triangular solves).  Otherwise the explicit
//     inverse Li = L^-T L^-1 (densesolver.jl:47-48), ALi' = Li A' and
//     S = A Li A' on MFMA, S^-1 the same way (:49-51);
//   - two KKT solves (densesolver.jl:54-90) and the step/update.
// LDS (<40 KiB per wave at n=64) holds only vectors, A and broadcast scratch,
// so four one-wave blocks (one per SIMD) share a CU.
//
// Code-size discipline: the driver is a micro-phase loop in which the cone
// vector op, the factorisation, the KKT solve body and the residuals each
// have exactly one inlined instance (no calls: a call would force the live
// H/Li tiles out of registers), keeping the instruction stream cache-resident.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace socp {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int MAXC = 64;   // cone table size in the kernel arguments
constexpr int NCS = 8;     // cones supported by the register-resident kernel
constexpr int KMAX = 128;  // k supported by the register-resident kernel
constexpr int POC_K = 0, SOC_K = 1;

struct ConeTable {
  int32_t nc;
  int32_t kind[MAXC];
  int32_t offs[MAXC];
  int32_t dim[MAXC];
};

// MODE_SETUP / MODE_SOLVEKKT: the two plugin calls of densesolver.jl
// (setup_iter :41-52 keeps scaling + H^-1 + S^-1 in a per-problem device
// record; solve_kkt :54-90 solves one right-hand side against it)
enum { MODE_SOLVE = 0, MODE_KKT = 1, MODE_SETUP = 2, MODE_SOLVEKKT = 3 };
enum { ST_CONVERGED = 0, ST_MAXIT = 1, ST_CHOL_H = 2, ST_CHOL_S = 3, ST_DOMAIN = 4, ST_PRIMAL_INF = 5, ST_DUAL_INF = 6 };
enum { F_WARM = 2, F_DETECT = 256, F_SHARED = 512 };

// SOCP_F_DETECT_INFEASIBLE (include/socp.h): the verdict from the five sums
// hz = h'z + b'y, |A'y + G'z|^2, cx = c'x, |Ax|^2, |Gx + s|^2 of the iterate.
// 0, or ST_PRIMAL_INF / ST_DUAL_INF with the factor (1/(-hz), 1/(-cx)) the
// certificate is returned multiplied by.  Every comparison is false on NaN.
__host__ __device__ inline int infeas_verdict(double hz, double aty2, double cx, double ax2, double gxs2,
                                              double tau, double& scale) {
  if (hz < 0.0 && sqrt(aty2) < tau * -hz) {
    scale = 1.0 / -hz;
    return ST_PRIMAL_INF;
  }
  if (cx < 0.0) {
    const double t = tau * -cx;
    if (sqrt(ax2) < t && sqrt(gxs2) < t) {
      scale = 1.0 / -cx;
      return ST_DUAL_INF;
    }
  }
  return 0;
}

struct SmallArgs {
  int64_t B;
  int32_t n, m, k, nc;
  int32_t maxit, sigma_exp;
  double tol, step, init_eps;
  int32_t flags, mode, deg;
  int32_t al_rows;  // 1, 2 or 4 when every cone is 16, 32 or 64 long (so 16-lane-row aligned): register-only cone reductions; 0 otherwise
  const double *c, *A, *b, *G, *h;
  const uint8_t* sing;
  double *x, *y, *z, *s;
  int32_t *iters, *status;
  double* res;
  const double *dx, *dy, *dz, *ds;  // (MODE_SOLVE with F_DETECT: dx carries the tolerance, small_itol)
  double *cx, *cy, *cz, *cs;
  int32_t* counter;
  double* dbg;                 // optional (KKT mode): per problem H[n*n], Li[n*n], lam[k], wb[k]
  unsigned long long* stamps;  // SOCP_DIAG builds: per-phase cycle totals
  ConeTable cones;
  double* rec;                 // MODE_SETUP / MODE_SOLVEKKT: per-problem factor records
  int64_t rec_stride;          // doubles per record
  // solver kernels compiled for pure slots (k > 64, small_slot_plan): the
  // slots' rotation, 0 or 64, and the pair of kinds the host picked the kernel by
  int32_t slot_rot, slot_kinds;
  // nonzero: the residuals' G x pass forms the SYRK's cone rows U (gemv_G_chunk<.., FU>):
  // bit 8, and bit c for every SOC cone c.  The host sets it only with al_rows >= 2,
  // cones of 32 or 64 rows (env SOCP_FUSE_U=0 clears it)
  int32_t fuse_u;
  // nonzero: load_problem forms the initial point's G'G in the H tiles while G's
  // loads are in flight, and the first factorisation takes it (FAC_IDENT_H).
  // The host sets it for the plain solver kernels compiled with the pipelined
  // load (init_overlap_kernel), never on a warm start (no initial
  // factorisation); env SOCP_INIT_OVERLAP=0 clears it
  int32_t init_overlap;
};

// Slot kinds.  The cone vector ops hold a k-vector as two 64-lane slots; slot
// s, lane l holds element (64 s + l - rot) mod k (only the lanes 64 s + l < k).
// A slot whose elements are all SOC (all POC) runs only that cone kind's
// algebra and reductions.  The pair of kinds is a template parameter of the
// kernel: the mixed kernel carries nothing of the pure ones.
enum { SLOT_MIXED = 0, SLOT_SOC = 1, SLOT_POC = 2 };
// pure-slot solver kernels: socp_small_kernel<.., KM = pair << 4>
enum { SLOT_PAIR_NONE = 0, SLOT_PAIR_SP = 1, SLOT_PAIR_PS = 2, SLOT_PAIR_SS = 3, SLOT_PAIR_PP = 4 };
constexpr int slot_pair_kind(int pair, int s) {
  if (pair == SLOT_PAIR_NONE) return SLOT_MIXED;
  const bool soc = pair == SLOT_PAIR_SS || (pair == SLOT_PAIR_SP && s == 0) || (pair == SLOT_PAIR_PS && s == 1);
  return soc ? SLOT_SOC : SLOT_POC;
}
constexpr int slot_pair_of(int k0, int k1) {
  return k0 == SLOT_SOC ? (k1 == SLOT_POC ? SLOT_PAIR_SP : (k1 == SLOT_SOC ? SLOT_PAIR_SS : SLOT_PAIR_NONE))
                        : (k0 == SLOT_POC ? (k1 == SLOT_SOC ? SLOT_PAIR_PS : (k1 == SLOT_POC ? SLOT_PAIR_PP : SLOT_PAIR_NONE))
                                          : SLOT_PAIR_NONE);
}

// kind of slot s under rotation rot (k > 64)
inline int small_slot_kind(const ConeTable& t, int nc, int k, int rot, int s) {
  bool soc = false, poc = false;
  for (int p = 64 * s; p < 64 * s + 64 && p < k; ++p) {
    const int i = (p - rot + k) % k;
    for (int c = 0; c < nc; ++c)
      if (i >= t.offs[c] && i < t.offs[c] + t.dim[c]) (t.kind[c] == SOC_K ? soc : poc) = true;
  }
  return soc && poc ? (int)SLOT_MIXED : (soc ? (int)SLOT_SOC : (int)SLOT_POC);
}
// The launch's slot plan.  Both slots pure as the table stands: rot = 0.
// Otherwise, when elements 0 .. k-65 are POC and the last 64 are SOC, rot = 64
// puts the SOC elements in slot 0 and the POC elements in slot 1 -- taken only
// when every cone is whole 16-lane rows (al_rows != 0), which the rotation by
// whole rows keeps so, so that every reduction keeps its order.  Otherwise
// rot = 0 and mixed slots.  Slot bases stay wave-uniform: slot s starts at
// element (rot ? (s ? 0 : k - 64) : 64 s).
inline void small_slot_plan(const ConeTable& t, int nc, int k, int al_rows, bool enable, int32_t& rot,
                            int32_t& kinds) {
  rot = 0;
  kinds = 0;
  if (!enable || k <= 64 || k > KMAX) return;
  for (int r = 0; r <= 64; r += 64) {
    if (r && !al_rows) break;
    const int k0 = small_slot_kind(t, nc, k, r, 0), k1 = small_slot_kind(t, nc, k, r, 1);
    // (two SOC slots are left to the mixed kernel: that pair's kernel did not repeat the mixed kernel's bits)
    if (k0 != SLOT_MIXED && k1 != SLOT_MIXED && !(k0 == SLOT_SOC && k1 == SLOT_SOC) &&
        (r == 0 || (k0 == SLOT_SOC && k1 == SLOT_POC))) {
      rot = r;
      kinds = k0 | (k1 << 4);
      return;
    }
  }
}

// Exact-fit solver kernels: socp_small_kernel<.., KM = (pair << 4) | KM_EXACT>,
// the pure-slot plain solver compiled for ONE launch geometry.  The launch fills
// its variant exactly (n = 16 NQ, k = 4 NP, m = 16 MQ), so the dims are
// constants and every bounds predicate folds; al_rows, slot_rot and fuse_u are
// constants too, and with them the cone table: k / (16 al_rows) cones of
// 16 al_rows rows each, laid end to end, cone c SOC exactly when bit c of
// fuse_u is set.  The phase loop is the generic kernel's, the G'G probe and the
// KKT entry phase included (leaving them out gained nothing measurable,
// DESIGN.md 5l).  One line per compiled kernel;
// gen_inst.py's EXACT names the same (variant, pair) entries, and the host
// takes the kernel only where small_exact_fit() says the launch is this one.
struct ExactFit {
  int NQ, NP, MQ, pair;
  int al_rows, slot_rot, fuse_u;
};
constexpr int KM_EXACT = 128;
constexpr ExactFit kExactFit[] = {
    {4, 24, 1, SLOT_PAIR_SP, 2, 64, 0x100 | 2 | 4},  // n=64 m=16 k=96, POC32+SOC32+SOC32 (bench.py's C2)
};
constexpr int kExactFitCount = (int)(sizeof(kExactFit) / sizeof(kExactFit[0]));
constexpr int exact_fit_index(int NQ, int NP, int MQ, int pair) {
  for (int i = 0; i < kExactFitCount; ++i)
    if (kExactFit[i].NQ == NQ && kExactFit[i].NP == NP && kExactFit[i].MQ == MQ && kExactFit[i].pair == pair) return i;
  return -1;
}
// Is this launch the one the exact-fit kernel of (variant, pair) was compiled
// for?  All of it is read from what launch_small has set in `a`.
inline bool small_exact_fit(const SmallArgs& a, int NQ, int NP, int MQ, int pair) {
  const int i = exact_fit_index(NQ, NP, MQ, pair);
  if (i < 0) return false;
  const ExactFit& e = kExactFit[i];
  if (a.n != 16 * NQ || a.k != 4 * NP || a.m != 16 * MQ) return false;
  if (a.al_rows != e.al_rows || a.slot_rot != e.slot_rot || a.fuse_u != e.fuse_u) return false;
  const int d = 16 * e.al_rows;
  if (a.nc * d != a.k) return false;
  for (int c = 0; c < a.nc; ++c)
    if (a.cones.offs[c] != c * d || a.cones.dim[c] != d) return false;
  return true;
}

// socp_small_kernel's fourth template argument KM, decoded in this one place (the kernel's own template
// arguments read it, and inst_table.hip's static_asserts hold it to gen_inst.py's KINDS).  bit 0 plugin: the
// plugin-entry kernel (MODE_KKT / MODE_SETUP / MODE_SOLVEKKT) instead of the solver; bit 1 xi: the explicit-inverse
// variant; bit 2 di: the solver with SOCP_F_DETECT_INFEASIBLE; bit 3 qp: the QP solver (socp_batch_solve_qp; mixed
// slots only), with bit 0 the QP plugin entries; bits 4..6 pair: the plain solver for a pair of pure slots
// (SLOT_PAIR_*); bit 7 exact (KM_EXACT, with a pair): that solver at one exact launch geometry (ExactFit)
struct SmallKM {
  bool plugin, xi, di, qp;
  int pair;
  bool exact;
};
constexpr SmallKM small_km(int KM) {
  return {(KM & 1) != 0, (KM & 2) != 0, (KM & 4) != 0, (KM & 8) != 0, (KM >> 4) & 7, (KM & KM_EXACT) != 0};
}

// MODE_SOLVE reads no right-hand side: with F_DETECT the slot of dx carries
// the bits of the infeasibility tolerance, so that the layout of the kernel
// arguments -- and with it the code of every kernel that does not detect --
// stays as it was.
inline void small_set_itol(SmallArgs& a, double tol) {
  uint64_t u;
  static_assert(sizeof(u) == sizeof(tol) && sizeof(u) == sizeof(a.dx), "64-bit slot");
  __builtin_memcpy(&u, &tol, sizeof(u));
  a.dx = reinterpret_cast<const double*>(static_cast<uintptr_t>(u));
}
__device__ __forceinline__ double small_itol(const SmallArgs& a) {
  return __longlong_as_double(static_cast<long long>(reinterpret_cast<uintptr_t>(a.dx)));
}

// The QP solver kernels (socp_batch_solve_qp; KM bit 3, the blocked kernel's
// QP instantiations): MODE_SOLVE reads no dy either, and that slot carries P --
// B matrices n x n column-major, or one with F_SHARED.  Only those kernels read
// it; the argument layout of the others stays as it was.
inline void small_set_qp(SmallArgs& a, const double* P) { a.dy = P; }
__device__ __forceinline__ const double* small_qp(const SmallArgs& a) { return a.dy; }
// The QP plugin entries (socp_batch_kkt_solve_qp, socp_dense_create_qp; KM = 9,
// the blocked QP kernels in MODE_KKT / MODE_SETUP / MODE_SOLVEKKT) read dy as a
// right-hand side: there P rides in the slot of x, which only MODE_SOLVE reads
// or writes.
inline void small_set_qp_plugin(SmallArgs& a, const double* P) { a.x = const_cast<double*>(P); }
__device__ __forceinline__ const double* small_qp_plugin(const SmallArgs& a) { return a.x; }

// ------------------------------------------------------------ LDS layout
// Fixed region (independent of the template shape):
#ifdef SOCP_DIAG
#define SOCP_NSTAMP_SLOTS 24
#else
#define SOCP_NSTAMP_SLOTS 0
#endif
enum : int {
  O_COFF = 0,                // cone offs[NCS]
  O_CDIM = O_COFF + NCS,     // cone dim[NCS]
  O_CKIND = O_CDIM + NCS,    // cone kind[NCS]
  O_CC = O_CKIND + NCS,        // per-cone constants of the current scaling [NCC][NCS]
  O_PART = O_CC + 20 * NCS,    // segment partials [NVMAX = 6][NCS][2 slots] (zero where unused)
  O_TOTC = O_PART + 6 * NCS * 2,  // per-cone results [4][NCS]
  O_STAMPS = O_TOTC + 4 * NCS,  // diagnostic build only: per-phase cycle totals of this wave [24]
  O_FIXED = O_STAMPS + SOCP_NSTAMP_SLOTS  // then (Shape): rcode[KP], 17 k-vectors KS apart, ...
};
constexpr int NKV = 17;
// per-cone constants (SOC cones), recomputed by every scaling:
//   MU = mu, IMU = 1/mu, WB0 = wbar_0, I1 = 1/(1+wbar_0), W2 = |wbar_1|^2,
//   L0 = lambda_0, AA = lambda_0^2 - |lambda_1|^2 (iprod!'s `a`, vectors.jl:105),
//   IAA = 1/AA, IL0 = 1/lambda_0, IL0AA = 1/(lambda_0 AA),
//   SA = 1/sqrt(AA) (scmax's `a`, mats.jl:66), SAL = 1/(SA lambda_0 + 1),
//   WL = wbar_1'lambda_1; AS, AZ, BS, BZ: the tail rows of wbar and lambda as
//   wbar_i = AS s_i - AZ z_i, lambda_i = BS s_i + BZ z_i (scalings.jl:57-97);
// per solve: DLT = wbar_1'k0_1 of the current KKT solve's k0 (solve_head ->
// solve_tail), KK = the cone's kt2'kt3 (head of kt2 o kt3, solve_tail -> affine_post)
enum : int { CC_MU, CC_IMU, CC_WB0, CC_I1, CC_W2, CC_L0, CC_AA, CC_IAA, CC_IL0, CC_IL0AA, CC_SA,
             CC_SAL, CC_WL, CC_AS, CC_AZ, CC_BS, CC_BZ, CC_DLT, CC_KK };
__host__ __device__ constexpr int cc(int q, int c) { return O_CC + q * NCS + c; }
// k-vector ids (IL: 1/lambda_i of the POC elements).  KV_RZ .. KV_T2 are
// dead while a factorisation runs (the previous solve's results are consumed,
// the next solve's temporaries not yet written): the Cholesky shapes' tile
// transpose buffer lives there (Shape::O_TB).
enum : int { KV_H, KV_Z, KV_S, KV_DZ, KV_DS, KV_LAM, KV_WB, KV_CA, KV_CB, KV_IL, KV_RZ, KV_RS, KV_K0,
             KV_K1, KV_K2, KV_T1, KV_T2 };
constexpr int NKV_DEAD = KV_T2 - KV_RZ + 1;

// the A block's leading dimension (Shape::LDA)
__host__ __device__ constexpr int small_lda(int NQ, int NP) {
  return (NQ * NP > 24 && NQ > 1) ? 16 * NQ + 2 : 16 * NQ + 1;  // (16 NQ + 2) / 2 is odd
}

// The LDS layout of one shape, in doubles from the wave's base: the one source
// of Shape's offsets, small_lds_bytes and small_rec_doubles.
struct SmallLayout {
  int NPAD, KP, MPAD, LDA, KS;
  bool AL_LDS, TB_ALIAS, UBT;
  int O_RC, O_KV, O_A, O_NV, O_MV, UAL, O_U, O_TB, O_UBT, TOTAL;
};
__host__ __device__ constexpr SmallLayout small_layout(int NQ, int NP, int MQ) {
  SmallLayout L{};
  // LDA (row stride of A and of Z' / A Li in LDS): NPAD + 1 on the two-wave
  // shapes (their LDS is tight); on the others NPAD + 2 = 2 x odd, where the
  // A x / Z't reads of a half-wave (lanes cl, g in {0, 1}: cl LDA + g doubles)
  // hit 32 distinct bank pairs, instead of two lanes per pair at NPAD + 1
  L.NPAD = 16 * NQ;
  L.KP = 4 * NP;
  L.MPAD = 16 * MQ;
  L.LDA = small_lda(NQ, NP);
  // k-vector stride KP: lanes read slot 1 / padding elements i >= KP
  // unconditionally and mask the values by their type code (3 = pad), so those
  // reads may alias the next vector (the last one reads into the A block); every
  // write is guarded by i < k or the code, and rows [k, KP) stay zero.
  L.KS = L.KP;
  L.O_RC = O_FIXED;            // rcode[KP]: cone*4 + type (0 POC, 1 SOC head, 2 SOC tail, 3 pad)
  L.O_KV = L.O_RC + L.KP;      // 17 k-vectors, KS apart
  L.O_A = L.O_KV + NKV * L.KS;
  L.O_NV = L.O_A + L.MPAD * L.LDA;  // n-vectors: c x rd rx n0 tn
  L.O_MV = L.O_NV + 6 * L.NPAD;     // m-vectors: b y rp ry m0 tm
  // U[NCS][NPAD] (the SYRK's cone rows) and, for m <= 16, A Li (MPAD x LDA,
  // from the Schur step to the solves): their lifetimes do not overlap.
  // Z' / A Li is written by factor() after form_H and last read by the
  // combined solve; U is written either by compute_U() in factor() or, on
  // fused launches (SmallArgs::fuse_u), by the G x pass of the next
  // iteration's residuals -- after that last read -- and read by form_H only.
  // Nothing between the residuals and form_H touches the region (the exit
  // tests and infeas_check read k-, n- and m-vectors only), on the Cholesky,
  // the explicit-inverse and the detecting solvers alike.
  L.AL_LDS = MQ == 1;
  L.UAL = (L.AL_LDS && L.MPAD * L.LDA > NCS * L.NPAD) ? L.MPAD * L.LDA : NCS * L.NPAD;
  L.O_U = L.O_MV + 6 * L.MPAD;
  // tile transpose [16][17]: only factor() uses it; on the Cholesky shapes
  // (AL_LDS) in the k-vectors dead during a factorisation when they hold it
  L.TB_ALIAS = L.AL_LDS && NKV_DEAD * L.KS >= 16 * 17;
  L.O_TB = L.TB_ALIAS ? L.O_KV + KV_RZ * L.KS : L.O_U + L.UAL;
  // the SYRK's U-row table (int32 per k-row) where the LDS allows (not the
  // two-wave shapes, whose LDS is tight)
  L.UBT = NQ * NP > 24 && NQ > 1;
  L.O_UBT = L.O_U + L.UAL + (L.TB_ALIAS ? 0 : 16 * 17);
  L.TOTAL = L.O_UBT + (L.UBT ? (L.KP + 1) / 2 : 0);
  return L;
}

template <int NQ, int NP, int MQ>
struct Shape {
  static constexpr SmallLayout L = small_layout(NQ, NP, MQ);
  static constexpr int NPAD = L.NPAD, KP = L.KP, MPAD = L.MPAD, LDA = L.LDA, KS = L.KS;
  static constexpr int O_RC = L.O_RC, O_KV = L.O_KV, O_A = L.O_A, O_NV = L.O_NV, O_MV = L.O_MV;
  static constexpr bool AL_LDS = L.AL_LDS, TB_ALIAS = L.TB_ALIAS, UBT = L.UBT;
  static constexpr int UAL = L.UAL, O_U = L.O_U, O_AL = L.O_U, O_TB = L.O_TB, O_UBT = L.O_UBT, TOTAL = L.TOTAL;
  static constexpr int nv(int id) { return O_NV + id * NPAD; }
  static constexpr int mv(int id) { return O_MV + id * MPAD; }
};
enum : int { NV_C, NV_X, NV_RD, NV_RX, NV_N0, NV_TN };
enum : int { MV_B, MV_Y, MV_RP, MV_RY, MV_M0, MV_TM };

// doubles of one factor record of the register kernel: the H^-1 and S^-1
// tiles in lane order, LAM WB CA CBV IL, the per-cone constants, the sing flag,
// and on the AL_LDS shapes the A Li block kept in LDS
constexpr int64_t small_rec_doubles(int NQ, int NP, int MQ) {
  const SmallLayout L = small_layout(NQ, NP, MQ);
  const int64_t NT = NQ * (NQ + 1) / 2, MT = MQ * (MQ + 1) / 2;
  const int64_t al = L.AL_LDS ? (int64_t)L.MPAD * L.LDA : 0;
  return (NT + MT) * 256 + 5 * (int64_t)L.KP + 20 * NCS + al + 8;
}

#ifndef SOCP_DEV_LDS_PAD
#define SOCP_DEV_LDS_PAD 0  // probe builds only: extra LDS bytes per wave to cap the waves per CU
#endif
inline size_t small_lds_bytes(int NQ, int NP, int MQ) {
  return (size_t)small_layout(NQ, NP, MQ).TOTAL * sizeof(double) + SOCP_DEV_LDS_PAD;
}

// Diagnostic phase timing (separate build, -DSOCP_DIAG): per-phase s_memtime
// deltas accumulated per problem and added to a global table by lane 0.
#ifdef SOCP_DIAG
#define NSTAMP 12
#define NSUBSTAMP 11  // sub-phases (0-3 the H factorisation, 4-10 solve / cone-op parts), slots NSTAMP+1 ..
// Totals live in LDS (lane 0 read-modify-writes them), so the stamps cost no
// registers beyond the last timestamp; they are flushed once per wave.
#define STAMP_DECL uint64_t st_last = 0;
#define STAMP_START_S(obj) do { __builtin_amdgcn_s_waitcnt(0); (obj).st_last = __builtin_amdgcn_s_memtime(); } while (0)
#define STAMP(i) do { __builtin_amdgcn_s_waitcnt(0); const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(socp_lds + O_STAMPS)[i] += t_ - st_last; \
    st_last = t_; } while (0)
#define STAMP_SUB(i) do { if constexpr (SUBST) STAMP(NSTAMP + 1 + (i)); } while (0)
#define STAMP_X(i) STAMP(NSTAMP + 1 + (i))
#else
#define STAMP_DECL
#define STAMP_START_S(obj) do {} while (0)
#define STAMP(i) do {} while (0)
#define STAMP_SUB(i) do {} while (0)
#define STAMP_X(i) do {} while (0)
#endif
enum { SP_LOAD, SP_SCALING, SP_RESID, SP_U, SP_SYRK, SP_FACTOR_H, SP_SCHUR, SP_SOLVE, SP_STEP, SP_VOP,
       SP_STORE, SP_OTHER };

// Static-analysis build (-DSOCP_MARK, tools/isa_phases.py): region markers as
// assembly comments; never in a product or diagnostic library.
#ifdef SOCP_MARK
#define MARK_BEGIN(name) asm volatile(";@@BEGIN " name)
#define MARK_END(name) asm volatile(";@@END " name)
#else
#define MARK_BEGIN(name) do {} while (0)
#define MARK_END(name) do {} while (0)
#endif

extern __shared__ double socp_lds[];
#define LDS(i) socp_lds[(i)]
// Blocks are one wavefront: LDS instructions of a wave execute in issue order,
// so an LDS hand-off between lanes needs only a wave-scope fence (no s_barrier,
// no lgkmcnt drain) -- the rocPRIM wave_barrier() idiom.
#define SYNC()                                             \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

// A double pinned in two AGPRs (gfx950: VALU cannot read AGPRs; MFMA can).
// G lives here for the whole solve and is copied to VGPRs at each use.
struct AD {
  uint32_t lo, hi;
};
__device__ __forceinline__ void a_put(AD& r, double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(r.lo) : "v"((uint32_t)u));
  asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(r.hi) : "v"((uint32_t)(u >> 32)));
}
// a_put in the lanes of `mask` only (EXEC narrowed inside the statement): the
// other lanes keep what they hold.  With mask = 0 the AGPRs are carried over
// unchanged without a branch around the statement -- the values then live
// across the problem loop as tied operands, which the register allocator keeps
// in place (a conditional a_put makes them phi nodes instead, and clang-22's
// AGPR-copy rewrite has crashed on those).
__device__ __forceinline__ void a_put_masked(AD& r, uint64_t u, uint64_t mask) {
  uint64_t sv;
  asm volatile(
      "s_and_saveexec_b64 %2, %5\n\tv_accvgpr_write_b32 %0, %3\n\tv_accvgpr_write_b32 %1, %4\n\t"
      "s_mov_b64 exec, %2"
      : "+a"(r.lo), "+a"(r.hi), "=&s"(sv)
      : "v"((uint32_t)u), "v"((uint32_t)(u >> 32)), "s"(mask)
      : "scc");
}
__device__ __forceinline__ void a_put4_masked(AD& r0, AD& r1, AD& r2, AD& r3, uint64_t u0, uint64_t u1, uint64_t u2,
                                              uint64_t u3, uint64_t mask) {
  uint64_t sv;
  asm volatile(
      "s_and_saveexec_b64 %8, %17\n\t"
      "v_accvgpr_write_b32 %0, %9\n\tv_accvgpr_write_b32 %1, %10\n\t"
      "v_accvgpr_write_b32 %2, %11\n\tv_accvgpr_write_b32 %3, %12\n\t"
      "v_accvgpr_write_b32 %4, %13\n\tv_accvgpr_write_b32 %5, %14\n\t"
      "v_accvgpr_write_b32 %6, %15\n\tv_accvgpr_write_b32 %7, %16\n\t"
      "s_mov_b64 exec, %8"
      : "+a"(r0.lo), "+a"(r0.hi), "+a"(r1.lo), "+a"(r1.hi), "+a"(r2.lo), "+a"(r2.hi), "+a"(r3.lo), "+a"(r3.hi),
        "=&s"(sv)
      : "v"((uint32_t)u0), "v"((uint32_t)(u0 >> 32)), "v"((uint32_t)u1), "v"((uint32_t)(u1 >> 32)),
        "v"((uint32_t)u2), "v"((uint32_t)(u2 >> 32)), "v"((uint32_t)u3), "v"((uint32_t)(u3 >> 32)), "s"(mask)
      : "scc");
}
__device__ __forceinline__ double a_get(const AD& r) {
  uint32_t lo, hi;
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(lo) : "a"(r.lo));
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(hi) : "a"(r.hi));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// A row step of G (NQ doubles) out of its AGPRs in ONE asm statement: the
// compiler pads one wait state after an asm that defines a VGPR a VALU op
// reads next, so reading the row together pays it once per row, not per value.
template <int NQ>
__device__ __forceinline__ void a_get_row(const AD (&r)[NQ], double (&out)[NQ]) {
  uint32_t lo[4], hi[4];
  if constexpr (NQ == 1) {
    asm("v_accvgpr_read_b32 %0, %2\n\tv_accvgpr_read_b32 %1, %3" : "=v"(lo[0]), "=v"(hi[0]) : "a"(r[0].lo), "a"(r[0].hi));
  } else if constexpr (NQ == 2) {
    asm("v_accvgpr_read_b32 %0, %4\n\tv_accvgpr_read_b32 %1, %5\n\tv_accvgpr_read_b32 %2, %6\n\t"
        "v_accvgpr_read_b32 %3, %7"
        : "=v"(lo[0]), "=v"(hi[0]), "=v"(lo[1]), "=v"(hi[1])
        : "a"(r[0].lo), "a"(r[0].hi), "a"(r[1].lo), "a"(r[1].hi));
  } else if constexpr (NQ == 3) {
    asm("v_accvgpr_read_b32 %0, %6\n\tv_accvgpr_read_b32 %1, %7\n\tv_accvgpr_read_b32 %2, %8\n\t"
        "v_accvgpr_read_b32 %3, %9\n\tv_accvgpr_read_b32 %4, %10\n\tv_accvgpr_read_b32 %5, %11"
        : "=v"(lo[0]), "=v"(hi[0]), "=v"(lo[1]), "=v"(hi[1]), "=v"(lo[2]), "=v"(hi[2])
        : "a"(r[0].lo), "a"(r[0].hi), "a"(r[1].lo), "a"(r[1].hi), "a"(r[2].lo), "a"(r[2].hi));
  } else {
    static_assert(NQ == 4, "NQ <= 4");
    asm("v_accvgpr_read_b32 %0, %8\n\tv_accvgpr_read_b32 %1, %9\n\tv_accvgpr_read_b32 %2, %10\n\t"
        "v_accvgpr_read_b32 %3, %11\n\tv_accvgpr_read_b32 %4, %12\n\tv_accvgpr_read_b32 %5, %13\n\t"
        "v_accvgpr_read_b32 %6, %14\n\tv_accvgpr_read_b32 %7, %15"
        : "=v"(lo[0]), "=v"(hi[0]), "=v"(lo[1]), "=v"(hi[1]), "=v"(lo[2]), "=v"(hi[2]), "=v"(lo[3]), "=v"(hi[3])
        : "a"(r[0].lo), "a"(r[0].hi), "a"(r[1].lo), "a"(r[1].hi), "a"(r[2].lo), "a"(r[2].hi), "a"(r[3].lo),
          "a"(r[3].hi));
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) out[q] = __longlong_as_double((long long)(((uint64_t)hi[q] << 32) | lo[q]));
}

// a_get for a value consumed directly as an MFMA A/B operand: v_accvgpr_read is
// a VALU write, and VALU write -> MFMA operand read needs 2 wait states, which
// hipcc does not insert for a producer inside inline asm (it pads one state).
__device__ __forceinline__ double a_get_mfma(const AD& r) {
  uint32_t lo, hi;
  asm("v_accvgpr_read_b32 %0, %2\n\tv_accvgpr_read_b32 %1, %3\n\ts_nop 1"
      : "=v"(lo), "=v"(hi)
      : "a"(r.lo), "a"(r.hi));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// Scheduling fence: keeps the scheduler from hoisting the next unrolled step's
// loads above this point (with H pinned in VGPRs and G in AGPRs, hoisting
// across steps is what overflows the register file).
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }
__device__ __forceinline__ double sel4(d4 t, int r) {
  double v = t[0];
  v = (r == 1) ? t[1] : v;
  v = (r == 2) ? t[2] : v;
  v = (r == 3) ? t[3] : v;
  return v;
}

// DPP move of a double (two 32-bit halves).  CTRL: 0x111+s = row_shr:s+1,
// 0x142 = row_bcast:15, 0x143 = row_bcast:31 (GFX9 DPP); RM = row mask.
template <int CTRL, int RM>
__device__ __forceinline__ double dpp(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int l2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, RM, 0xF, false);
  const int h2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, RM, 0xF, false);
  return __hiloint2double(h2, l2);
}
// DPP move whose pattern writes every lane (row_newbcast): no old value needed.
// row_newbcast:N (0x150 + N) of a double is one v_mov_b64_dpp; every other
// control has no 64-bit form and moves the two halves.
template <int CTRL>
__device__ __forceinline__ double dpp_all(double v) {
  if constexpr (CTRL >= 0x150 && CTRL <= 0x15F) return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false);
  const int l2 = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int h2 = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(h2, l2);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Lane ids re-read inside each phase (LANE_IDS shadows the members): values
// derived from them (4*pp + g, 16*ti + cl, ...) are then recomputed where they
// are used instead of being hoisted out of the persistent loop and kept live.
#ifndef SOCP_MULTI_WAVE
#define SOCP_MULTI_WAVE 0  // 1: workgroups of several wavefronts (socp_large.hip defines it)
#endif
__device__ __forceinline__ int lane_fresh() {
  int v = SOCP_MULTI_WAVE ? (int)threadIdx.x & 63 : (int)threadIdx.x;  // the lane in its wavefront
  asm volatile("" : "+v"(v));
  return v;
}
#define LANE_IDS()                      \
  const int lane = lane_fresh();        \
  const int g = lane >> 4, cl = lane & 15; \
  (void)g; (void)cl

// Sum over the four 16-lane rows (lanes l, l^16, l^32, l^48) with the gfx950
// row-swap permutes: every lane gets the same total, no LDS round trip.
__device__ __forceinline__ double rows_sum(double x) {
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const double y = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
  const unsigned ylo = (unsigned)__double2loint(y), yhi = (unsigned)__double2hiint(y);
  const auto c = __builtin_amdgcn_permlane16_swap(ylo, ylo, false, false);
  const auto d = __builtin_amdgcn_permlane16_swap(yhi, yhi, false, false);
  return __hiloint2double((int)d[0], (int)c[0]) + __hiloint2double((int)d[1], (int)c[1]);
}

// Cone reductions when every cone is R = 1, 2 or 4 whole 16-lane rows (all
// cones 16, 32 or 64 long): all-reduce inside each row by DPP rotations, then
// across the cone's rows with the row-swap permutes -- every lane of the cone
// gets the total, no predicates, no LDS.  MX: max instead of sum.
template <bool MX>
__device__ __forceinline__ double rop(double a, double b) { return MX ? fmax(a, b) : a + b; }
// Several independent values at once, step by step (each DPP step of one
// chain waits on its predecessor; interleaving the chains fills those wait
// states).  The same operations in the same order per value as
// cone_allreduce_rows.  MXM: bit q set = max for value q.
template <int NV, unsigned MXM>
__device__ __forceinline__ void cone_allreduce_rows_n(double (&v)[NV], int R) {
#define SOCP_AR_STEP(CTRL)                                                                          \
  _Pragma("unroll") for (int q = 0; q < NV; ++q) {                                                  \
    const double y = dpp_all<CTRL>(v[q]);                                                           \
    v[q] = ((MXM >> q) & 1) ? fmax(v[q], y) : v[q] + y;                                             \
  }
  SOCP_AR_STEP(0x128)
  SOCP_AR_STEP(0x124)
  SOCP_AR_STEP(0x122)
  SOCP_AR_STEP(0x121)
#undef SOCP_AR_STEP
  if (R >= 2) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const unsigned lo = (unsigned)__double2loint(v[q]), hi = (unsigned)__double2hiint(v[q]);
      const auto c = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
      const auto d = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
      const double a = __hiloint2double((int)d[0], (int)c[0]), b = __hiloint2double((int)d[1], (int)c[1]);
      v[q] = ((MXM >> q) & 1) ? fmax(a, b) : a + b;
    }
  }
  if (R == 4) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const unsigned lo = (unsigned)__double2loint(v[q]), hi = (unsigned)__double2hiint(v[q]);
      const auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
      const auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      const double a = __hiloint2double((int)d[0], (int)c[0]), b = __hiloint2double((int)d[1], (int)c[1]);
      v[q] = ((MXM >> q) & 1) ? fmax(a, b) : a + b;
    }
  }
}
template <bool MX>
__device__ __forceinline__ double cone_allreduce_rows(double v, int R) {
  v = rop<MX>(v, dpp_all<0x128>(v));  // row_ror:8
  v = rop<MX>(v, dpp_all<0x124>(v));  // row_ror:4
  v = rop<MX>(v, dpp_all<0x122>(v));  // row_ror:2
  v = rop<MX>(v, dpp_all<0x121>(v));  // row_ror:1
  if (R >= 2) {  // rows (2r, 2r+1)
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto c = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto d = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = rop<MX>(__hiloint2double((int)d[0], (int)c[0]), __hiloint2double((int)d[1], (int)c[1]));
  }
  if (R == 4) {  // halves (l, l ^ 32)
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    v = rop<MX>(__hiloint2double((int)d[0], (int)c[0]), __hiloint2double((int)d[1], (int)c[1]));
  }
  return v;
}

// Butterfly partner inside a 16-lane row for reduce-scatter level M, by DPP:
// M=8 row_ror:8 (l^8), M=4 row_half_mirror (l^7: flips bit 2 like l^4, so the
// halving is the same), M=2 quad_perm[2,3,0,1] (l^2), M=1 quad_perm[1,0,3,2].
template <int M>
__device__ __forceinline__ double row_partner(double v) {
  constexpr int CTRL = M == 8 ? 0x128 : (M == 4 ? 0x141 : (M == 2 ? 0x4E : 0xB1));
  return dpp_all<CTRL>(v);
}

// Wave-uniform copies.  LLVM's divergence analysis treats every LDS or global
// load as divergent; a branch on such a value (a pivot test, the
// per-problem `sing` flag, the phase number) is then compiled as exec-masked
// straight-line code: every arm runs and the live ranges of all arms merge.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Inclusive segmented scan over the 64 lanes with DPP (row_shr 1,2,4,8 then
// row_bcast 15/31): lane l accumulates lanes [max(ssl, 0) .. l] with op
// (sum, or max when mx).  ssl = first lane of l's segment.
template <int V>
__device__ __forceinline__ void dpp_scan(double (&x)[V], int lane, int ssl, bool mx) {
  const int rl = lane & 15;
#define SOCP_SCAN_STEP(CTRL, RM, OK)                                 \
  {                                                                  \
    const bool ok_ = (OK);                                           \
    _Pragma("unroll") for (int v = 0; v < V; ++v) {                  \
      const double y = dpp<CTRL, RM>(x[v]);                          \
      const double r = mx ? fmax(x[v], y) : x[v] + y;                \
      x[v] = ok_ ? r : x[v];                                         \
    }                                                                \
  }
  SOCP_SCAN_STEP(0x111, 0xF, rl >= 1 && lane - 1 >= ssl)
  SOCP_SCAN_STEP(0x112, 0xF, rl >= 2 && lane - 2 >= ssl)
  SOCP_SCAN_STEP(0x114, 0xF, rl >= 4 && lane - 4 >= ssl)
  SOCP_SCAN_STEP(0x118, 0xF, rl >= 8 && lane - 8 >= ssl)
  SOCP_SCAN_STEP(0x142, 0xA, ((lane >> 4) & 1) && ((lane & ~15) - 1 >= ssl))
  SOCP_SCAN_STEP(0x143, 0xC, lane >= 32 && 31 >= ssl)
#undef SOCP_SCAN_STEP
}

// whole-wave sum / max (scan to lane 63, broadcast through an SGPR)
__device__ __forceinline__ double wsum(double v) {
  double x[1] = {v};
  dpp_scan<1>(x, threadIdx.x, 0, false);
  return readlane_d(x[0], 63);
}
__device__ __forceinline__ double wmax(double v) {
  double x[1] = {v};
  dpp_scan<1>(x, threadIdx.x, 0, true);
  return readlane_d(x[0], 63);
}

// x^e for an integer exponent (Julia's ^(::Float64, ::Integer); e = 3 is x*x*x)
__device__ __forceinline__ double ipow(double x, int e) {
  if (e == 3) return x * x * x;
  double r = 1.0, b = x;
  for (int q = e; q > 0; q >>= 1) {
    if (q & 1) r *= b;
    b *= b;
  }
  return r;
}

// IEEE classes (v_cmp_class_f64 mask bits) at which the Newton refinement of
// a v_rcp / v_rsq seed would turn an exact 0 or inf into NaN (0 * inf): +-0,
// +-inf.  There the seed is the IEEE result itself and is returned as is.
constexpr int kClassZeroInf = (1 << 2) | (1 << 5) | (1 << 6) | (1 << 9);

// pivot reciprocal: v_rcp_f64 + two Newton steps (within 1 ulp of 1/d; 1/+-0 =
// +-inf and 1/+-inf = +-0 exactly, as IEEE division gives)
__device__ __forceinline__ double recip(double d) {
  const double r0 = __builtin_amdgcn_rcp(d);
  double e = fma(-d, r0, 1.0);
  double r = fma(r0, e, r0);
  e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  return __builtin_amdgcn_class(d, kClassZeroInf) ? r0 : r;
}

// Reduce-scatter over the 16 lanes of a row (xor masks 8,4,2,1): on return the
// lane holds in P[0..CF) the full row-sums of entries base+j.
template <int C, int M>
__device__ __forceinline__ void rs16(double* P, int cl, int& base) {
  if constexpr (M == 0) {
    return;
  } else if constexpr (C % 2 == 0) {
    constexpr int H = C / 2;
    const bool hi = (cl & M) != 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      double mine = hi ? P[H + j] : P[j];
      double other = hi ? P[j] : P[H + j];
      P[j] = mine + row_partner<M>(other);
    }
    if (hi) base += H;
    rs16<H, M / 2>(P, cl, base);
  } else {
#pragma unroll
    for (int j = 0; j < C; ++j) P[j] += row_partner<M>(P[j]);
    rs16<C, M / 2>(P, cl, base);
  }
}
// the lane's first entry index after rs16<C, M> (its `base`), known up front
template <int C, int M>
__device__ __forceinline__ int rs16_base(int cl) {
  if constexpr (M == 0) {
    return 0;
  } else if constexpr (C % 2 == 0) {
    return ((cl & M) != 0 ? C / 2 : 0) + rs16_base<C / 2, M / 2>(cl);
  } else {
    return rs16_base<C, M / 2>(cl);
  }
}
template <int C, int M>
struct RSCount {
  static constexpr int value =
      (M == 0) ? C : ((C % 2 == 0) ? RSCount<C / 2, M / 2>::value : RSCount<C, M / 2>::value);
};
template <int C>
struct RSCount<C, 0> {
  static constexpr int value = C;
};

// what factor() factors: the scaling's H with U still to form (compute_U), the
// identity scaling's (U = 0), or the scaling's with U already in LDS -- formed by
// the residuals' G x pass of the same MP_ITER visit (launches with
// SmallArgs::fuse_u).  The kind is chosen by the phase that asks for the
// factorisation, for that factorisation alone: a problem that leaves MP_ITER
// after U was formed (exit test, DomainError, infeasibility rule, the residuals
// after the last iteration) asks for none, and nothing is carried to the
// wave's next problem.
// FAC_IDENT_H: the identity scaling's, with G'G already in the H tiles -- formed
// by this problem's load_problem from the registers G's loads arrived in
// (launches with SmallArgs::init_overlap).  Only the first factorisation after
// that load may name it: MP_SINGTEST's, or MP_INIT's when no probe ran before it
// (a probe factors the tiles in place, so MP_INIT behind one rebuilds H with
// FAC_IDENT).  factor() then skips form_H's zeroing and row loop and runs the
// rest (A'A, the padded diagonal).  Same bits as FAC_IDENT: with W = I the row
// loop's X is fma(1.0, g, 0.0 * 0.0) = g, except that -0 becomes +0; the
// accumulators start at +0, and a sum in round-to-nearest is -0 only when every
// addend is, so the sign of a zero operand cannot reach H.  Per tile the MFMA
// sequence is the same: row steps ascending from T = 0.
enum : int { FAC_SCALED, FAC_IDENT, FAC_SCALED_U, FAC_IDENT_H };
// The kernels compiled with the pipelined load: the plain solvers (mixed and
// pure-slot; not the plugin entries, the explicit-inverse, detecting or QP
// kernels) of C2's variant.  Every other instantiation keeps load_problem and
// factor() as they were, at compile time.
constexpr bool init_overlap_kernel(int NQ, int NP, int MQ, int KM) {
  const SmallKM K = small_km(KM);
  return NQ == 4 && NP == 24 && MQ == 1 && !K.plugin && !K.xi && !K.di && !K.qp;
}
// driver micro-phases and solve kinds
enum : int {
  MP_SINGTEST, MP_SINGTEST_POST, MP_FACTOR, MP_INIT, MP_ITER, MP_KKT,
  MP_SOLVE_HEAD, MP_SOLVE_MAT, MP_SOLVE_TAIL, MP_SAVE
};
enum : int { RET_INIT, RET_KKT, RET_AFFINE, RET_COMBINED };

// ---------------------------------------- 16x16 tile kernels (shared by the
// register kernel's and the blocked kernel's factorisations)

// Broadcast across the four 16-lane rows: every lane gets x from the lane of
// row R with the same column index (gfx950 v_permlane32_swap / 16_swap).
template <int R>
__device__ __forceinline__ double row_bcast(double x) {
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto a32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const unsigned ylo = (R < 2) ? a32[0] : a32[1], yhi = (R < 2) ? b32[0] : b32[1];
  const auto a16 = __builtin_amdgcn_permlane16_swap(ylo, ylo, false, false);
  const auto b16 = __builtin_amdgcn_permlane16_swap(yhi, yhi, false, false);
  const unsigned zlo = (R & 1) ? a16[1] : a16[0], zhi = (R & 1) ? b16[1] : b16[0];
  return __hiloint2double((int)zhi, (int)zlo);
}

// All four row broadcasts of x at once: out[R] = x of row R, same column index.
__device__ __forceinline__ void row_bcast4(double x, double (&out)[4]) {
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto a32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const auto a16 = __builtin_amdgcn_permlane16_swap(a32[h], a32[h], false, false);
    const auto b16 = __builtin_amdgcn_permlane16_swap(b32[h], b32[h], false, false);
    out[2 * h] = __hiloint2double((int)b16[0], (int)a16[0]);
    out[2 * h + 1] = __hiloint2double((int)b16[1], (int)a16[1]);
  }
}

// x^-1/2: v_rsq_f64 + two Newton steps (within 1 ulp; +-0 -> +-inf and
// +inf -> 0 as 1/sqrt gives them in IEEE arithmetic, negative -> NaN)
__device__ __forceinline__ double rsqrt_nr(double d) {
  const double y0 = __builtin_amdgcn_rsq(d);
  const double h = 0.5 * d;
  double e = fma(-(h * y0), y0, 0.5);
  double y = fma(y0, e, y0);
  e = fma(-(h * y), y, 0.5);
  y = fma(y, e, y);
  return __builtin_amdgcn_class(d, kClassZeroInf) ? y0 : y;
}
// x * q for q = rsqrt_nr(p) where p = 0 makes q = inf: an exact zero factor
// stays zero, as sqrt(0 * y) and sqrt(0 / y) are in IEEE arithmetic (a
// boundary iterate of a POC cone, s_i z_i = 0), instead of 0 * inf = NaN
__device__ __forceinline__ double zmul(double x, double q) { return x == 0.0 ? x : x * q; }
// square root through rsqrt_nr (0 and +inf passed through, negative -> NaN)
__device__ __forceinline__ double sqrt_nr(double d) {
  const double r = d * rsqrt_nr(d);
  return (d == 0.0 || d == INFINITY) ? d : r;
}
// the tile factorisation's pivots: one Newton step (a shorter dependency
// chain, within a few ulp)
__device__ __forceinline__ double rsqrt_tile(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  const double e = fma(-(0.5 * d) * y, y, 0.5);
  return fma(y, e, y);
}

// Row blocks B.. of W = L^-1 for D = L L' (right-looking, 4 rows at a time;
// the rank-4 trailing update of the D and identity tiles is one MFMA each).
// Every lane forms the block's rows of R = L' and of W by forward
// substitution from the broadcast block rows; the 4x4 diagonal block (its
// upper triangle, as potrf('U') reads it) is read out of those rows by in-row
// broadcasts (!LANES: factored beforehand in wave-uniform values, the same
// operations on the same values).
struct NoHook {
  template <int B>
  __device__ __forceinline__ void run() const {}
};
template <int B, bool INPL, bool LANES, class H = NoHook>
__device__ __forceinline__ void tile_block(d4& Dt, d4& It, d4& W, bool& ok, const H& hook = H()) {
  if constexpr (B < 4) {
    LANE_IDS();
    double R, Wb;
    if constexpr (LANES) {
      // V[i], X[i]: rows 4B+i of the D and identity tiles in every row group.
      // Row R_i of L' holds the pivot block's own entries at columns 4B..4B+3
      // (r_ij = R_i at column 4B+j, the pivot d_i = T_i at column 4B+i), so
      // they are in-row broadcasts of values the lanes form anyway
      double V[4], X[4];
      row_bcast4(Dt[B], V);
      row_bcast4(It[B], X);
      const double rs0 = rsqrt_tile(dpp_all<0x150 + 4 * B>(V[0]));
      const double R0 = V[0] * rs0, W0 = X[0] * rs0;
      const double r01 = dpp_all<0x150 + 4 * B + 1>(R0), r02 = dpp_all<0x150 + 4 * B + 2>(R0),
                   r03 = dpp_all<0x150 + 4 * B + 3>(R0);
      const double T1 = fma(-r01, R0, V[1]), Y1 = fma(-r01, W0, X[1]);
      const double rs1 = rsqrt_tile(dpp_all<0x150 + 4 * B + 1>(T1));
      const double R1 = T1 * rs1, W1 = Y1 * rs1;
      const double r12 = dpp_all<0x150 + 4 * B + 2>(R1), r13 = dpp_all<0x150 + 4 * B + 3>(R1);
      const double T2 = fma(-r12, R1, fma(-r02, R0, V[2])), Y2 = fma(-r12, W1, fma(-r02, W0, X[2]));
      const double rs2 = rsqrt_tile(dpp_all<0x150 + 4 * B + 2>(T2));
      const double R2 = T2 * rs2, W2 = Y2 * rs2;
      const double r23 = dpp_all<0x150 + 4 * B + 3>(R2);
      const double T3 = fma(-r23, R2, fma(-r13, R1, fma(-r03, R0, V[3]))),
                   Y3 = fma(-r23, W2, fma(-r13, W1, fma(-r03, W0, X[3])));
      const double rs3 = rsqrt_tile(dpp_all<0x150 + 4 * B + 3>(T3));
      const double R3 = T3 * rs3, W3 = Y3 * rs3;
      R = g == 0 ? R0 : (g == 1 ? R1 : (g == 2 ? R2 : R3));
      Wb = g == 0 ? W0 : (g == 1 ? W1 : (g == 2 ? W2 : W3));
    } else {
      const double v = Dt[B], w = It[B];
      // a_ij = D[4B+i][4B+j] (i <= j): lane (i, 4B+j) of register B
      const double a00 = readlane_d(v, 4 * B), a01 = readlane_d(v, 4 * B + 1),
                   a02 = readlane_d(v, 4 * B + 2), a03 = readlane_d(v, 4 * B + 3);
      const double a11 = readlane_d(v, 16 + 4 * B + 1), a12 = readlane_d(v, 16 + 4 * B + 2),
                   a13 = readlane_d(v, 16 + 4 * B + 3);
      const double a22 = readlane_d(v, 32 + 4 * B + 2), a23 = readlane_d(v, 32 + 4 * B + 3);
      const double a33 = readlane_d(v, 48 + 4 * B + 3);
      const double rs0 = rsqrt_tile(a00);
      const double r01 = a01 * rs0, r02 = a02 * rs0, r03 = a03 * rs0;
      const double s11 = fma(-r01, r01, a11);
      const double rs1 = rsqrt_tile(s11);
      const double r12 = fma(-r01, r02, a12) * rs1, r13 = fma(-r01, r03, a13) * rs1;
      const double s22 = fma(-r12, r12, fma(-r02, r02, a22));
      const double rs2 = rsqrt_tile(s22);
      const double r23 = fma(-r12, r13, fma(-r02, r03, a23)) * rs2;
      const double s33 = fma(-r23, r23, fma(-r13, r13, fma(-r03, r03, a33)));
      const double rs3 = rsqrt_tile(s33);
      double V[4], X[4];
      row_bcast4(v, V);
      row_bcast4(w, X);
      const double R0 = V[0] * rs0;
      const double R1 = fma(-r01, R0, V[1]) * rs1;
      const double R2 = fma(-r12, R1, fma(-r02, R0, V[2])) * rs2;
      const double R3 = fma(-r23, R2, fma(-r13, R1, fma(-r03, R0, V[3]))) * rs3;
      const double W0 = X[0] * rs0;
      const double W1 = fma(-r01, W0, X[1]) * rs1;
      const double W2 = fma(-r12, W1, fma(-r02, W0, X[2])) * rs2;
      const double W3 = fma(-r23, W2, fma(-r13, W1, fma(-r03, W0, X[3]))) * rs3;
      R = g == 0 ? R0 : (g == 1 ? R1 : (g == 2 ? R2 : R3));
      Wb = g == 0 ? W0 : (g == 1 ? W1 : (g == 2 ? W2 : W3));
    }
    hook.template run<B>();  // independent MFMA work interleaved with the chain
    W[B] = Wb;
    if constexpr (B < 3 && INPL) {
      // whole tiles: registers <= B are never read again (the later blocks read
      // registers B+1..3), so the MFMA results replace Dt and It in place
      Dt = __builtin_amdgcn_mfma_f64_16x16x4f64(R, R, Dt, 0, 0, 1);   // Dt -= R'R
      It = __builtin_amdgcn_mfma_f64_16x16x4f64(R, Wb, It, 0, 0, 1);  // It -= R'W
    } else if constexpr (B < 3) {
      const d4 t = __builtin_amdgcn_mfma_f64_16x16x4f64(R, R, Dt, 0, 0, 1);   // Dt -= R'R
      const d4 u = __builtin_amdgcn_mfma_f64_16x16x4f64(R, Wb, It, 0, 0, 1);  // It -= R'W
#pragma unroll
      for (int r = B + 1; r < 4; ++r) {
        Dt[r] = t[r];
        It[r] = u[r];
      }
    }
    tile_block<B + 1, INPL, LANES>(Dt, It, W, ok, hook);
  }
}
// INPL: the trailing updates replace the tiles whole (one factorisation 3,126
// cycles vs 3,406 on one wave, profiles/r03_probe_tile.log); the copying form
// keeps fewer registers live, which the smallest register kernels need to stay
// at two waves per SIMD.
// LANES: the pivot blocks in lanes or in wave-uniform values; the same
// operations on the same values, so the same bits.
template <bool INPL, bool LANES, class H = NoHook>
__device__ __forceinline__ void factor_tile(d4 Dt, d4& W, bool& ok, const H& hook = H()) {
  MARK_BEGIN("factor_tile");
  LANE_IDS();
  d4 It;
#pragma unroll
  for (int r = 0; r < 4; ++r) It[r] = (g + 4 * r == cl) ? 1.0 : 0.0;
  W = It;
  tile_block<0, INPL, LANES>(Dt, It, W, ok, hook);
  // potrf's test once per tile: the diagonal of W = L^-1 holds the pivots'
  // 1/sqrt, which is finite and > 0 exactly when every pivot is > 0 (a pivot
  // <= 0 or NaN makes rsqrt_tile NaN; a NaN anywhere reaches every later pivot)
  bool dg = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) dg = dg && (g + 4 * r != cl || W[r] > 0.0);
  ok = ok && __all(dg);
}


// XI (SOCP_F_EXPLICIT_INVERSE): Li = H^-1 formed on every shape -- the
// reference's operation order (densesolver.jl:47-48 forms Li = L^-T L^-1 from
// cholesky!(H)) -- instead of the triangular solves of the m <= 16 shapes.
// KS0, KS1: the kinds of the two slots this kernel is compiled for (SLOT_*).
// Mixed (every kernel but the pure-slot solver kernels of the two-slot
// shapes): the fixed layout, slot s, lane l = element 64 s + l, and cone ops
// that handle any element.  Pure: SmallArgs::slot_rot is honoured.
// QP: the objective is x'Px/2 + c'x (socp_batch_solve_qp): H = P + G'W^-2 G
// (+A'A) and rd = Px + A'y + G'z + c; P is streamed from global memory (add_P,
// P_mv), never resident.
// EX (KM_EXACT): the exact-fit kernel of kExactFit's (variant, pair) entry:
// n, m, k, nc, al_rows, slot_rot and fuse_u are that entry's constants, not
// the launch's arguments (ExactFit above).  Same operations in the same order:
// only predicates that are always true at this geometry, and code this launch
// never runs, go away.
template <int NQ, int NP, int MQ, bool XI = false, int KS0 = SLOT_MIXED, int KS1 = SLOT_MIXED, bool QP = false,
          bool EX = false>
struct Small {
  using SH = Shape<NQ, NP, MQ>;
  static_assert((KS0 == SLOT_MIXED) == (KS1 == SLOT_MIXED), "both slots pure or both mixed");
  static_assert(KS0 == SLOT_MIXED || 4 * NP > 64, "pure slots: two-slot shapes only");
  static constexpr bool SLK = KS0 != SLOT_MIXED;
  static constexpr int EXI = EX ? exact_fit_index(NQ, NP, MQ, slot_pair_of(KS0, KS1)) : -1;
  static_assert(!EX || (EXI >= 0 && !XI && !QP), "exact fit: a kExactFit entry, plain solver");
  static constexpr ExactFit EXF = kExactFit[EXI >= 0 ? EXI : 0];
  static_assert(!EX || ((EXF.al_rows == 2 || EXF.al_rows == 4) && (EXF.fuse_u & 0x100) && NP % 8 == 0 &&
                        (4 * NP) % (16 * EXF.al_rows) == 0),
                "exact fit: fused U, whole cones of 32 or 64 rows");
  // the launch's geometry: kernel arguments, or the exact-fit kernel's constants
  __device__ __forceinline__ int al_rows() const {
    if constexpr (EX) return EXF.al_rows;
    else return a.al_rows;
  }
  __device__ __forceinline__ int slot_rot() const {
    if constexpr (EX) return EXF.slot_rot;
    else return a.slot_rot;
  }
  __device__ __forceinline__ int fuse_u() const {
    if constexpr (EX) return EXF.fuse_u;
    else return a.fuse_u;
  }
  // which algebra a slot of kind KD can need
  static constexpr bool may_soc(int KD) { return KD != SLOT_POC; }
  static constexpr bool may_poc(int KD) { return KD != SLOT_SOC; }
  static constexpr int NT = NQ * (NQ + 1) / 2;
  static constexpr int MT = MQ * (MQ + 1) / 2;
  static constexpr int NPAD = SH::NPAD, KP = SH::KP, MPAD = SH::MPAD, LDA = SH::LDA;
  static constexpr int O_A = SH::O_A, O_U = SH::O_U, O_AL = SH::O_AL, O_TB = SH::O_TB, O_RC = SH::O_RC,
                       O_KV = SH::O_KV;
  static constexpr bool AL_LDS = SH::AL_LDS;
  // in-place tile updates (factor_tile) except where G is small enough for two
  // waves per SIMD: C1's <2, 12, 1> takes 209 + 48 registers with them, 208 + 48
  // without
  static constexpr bool TILE_INPL = NQ * NP > 24;
  // the tile's pivot blocks in lanes on the m <= 16
  // shapes.  The m > 16 shapes keep the wave-uniform form: with the lane form
  // <2, 4, 2> takes 247 registers instead of 231 and falls to one wave per
  // SIMD, and three more NQ = 4 objects trip the compiler's AGPR-rewrite pass
  static constexpr bool TILE_LANES = MQ == 1;
  // the solves' per-cone constants read ahead of the cone reductions (their
  // latency under the DPP chains) where registers allow: not in the kernels
  // that keep two waves per SIMD (C1's <2, 12, 1> would take 217 + 48; every
  // NQ = 1 shape)
  static constexpr bool HOIST_CST = NQ * NP > 24 && NQ > 1;
  static constexpr int C_ = SH::nv(NV_C), X_ = SH::nv(NV_X), RD = SH::nv(NV_RD),
                       RX = SH::nv(NV_RX), N0 = SH::nv(NV_N0), TN = SH::nv(NV_TN);
  static constexpr int B_ = SH::mv(MV_B), Y_ = SH::mv(MV_Y), RP = SH::mv(MV_RP),
                       RY = SH::mv(MV_RY), M0 = SH::mv(MV_M0);
  static constexpr int kvs(int id) { return O_KV + id * SH::KS; }
  static constexpr int H_ = kvs(KV_H), Z_ = kvs(KV_Z), S_ = kvs(KV_S), DZ = kvs(KV_DZ),
                       DS = kvs(KV_DS), RZ = kvs(KV_RZ), RS = kvs(KV_RS), LAM = kvs(KV_LAM),
                       WB = kvs(KV_WB), CA = kvs(KV_CA), CBV = kvs(KV_CB), K0 = kvs(KV_K0),
                       K1 = kvs(KV_K1), K2 = kvs(KV_K2), T1 = kvs(KV_T1), T2 = kvs(KV_T2),
                       IL = kvs(KV_IL);

  const SmallArgs& a;
  const int lane, g, cl;
  const int n, m, k, nc;
  bool sing;
  int64_t dbg_p = 0;
  // compact-layout element info (element i = 64*s + lane): cone, type code
  // (0 POC, 1 SOC head, 2 SOC tail, 3 none), cone offset, scan segment
  // start / last lane within the slot
  int ci[2], kd[2], eo[2], ssl[2], sle[2];
  bool spn[2];  // the lane's cone spans both slots
  STAMP_DECL

  AD G[NP][NQ];  // AGPR-resident
  d4 T[NT];
  d4 Sv[MT];
  // m <= 16: H = L L' (chol), Z = L^-1 A' in LDS, S = Z'Z; Li is never formed
  // and its products are triangular solves (trsv_fwd / trsv_bwd).
  // !CHOL (XI; the m > 16 shapes): Li = H^-1 is formed from the Cholesky
  // factor, Li = L^-T L^-1 (densesolver.jl:47-48, chol_inv), and likewise
  // S^-1.  Either way the SYRK leaves H in the upper-block form chol() reads.
  static constexpr bool CHOL = AL_LDS && !XI;

  __device__ __forceinline__ Small(const SmallArgs& args)
      : a(args), lane(threadIdx.x), g(threadIdx.x >> 4), cl(threadIdx.x & 15),
        n(EX ? 16 * NQ : args.n), m(EX ? 16 * MQ : args.m), k(EX ? 4 * NP : args.k),
        nc(EX ? 4 * NP / (16 * EXF.al_rows) : args.nc) {}

#ifndef SOCP_KO
#define SOCP_KO 0  // timing knock-outs (tuning builds only; results are wrong): 1 G loaded once per wave,
                   // 2 no residuals, 4 no U (neither compute_U nor the residuals' fused form), 8 no S factorisation,
                   // 16 no Gx (so no fused U either: the factorisation then runs compute_U), 32 no G'z, 128 no A products
                   // (the three of resid_scaling_k's residual half), 256 no triangular solves, 512 / 1024 no G products
                   // in the solves, 2048 no S solves, 4096 no scaling, 8192 no solve head,
                   // 16384 no solve tail, 32768 no corrector, 65536 no SYRK (H = I), 131072 no chol
#endif
  // ---------------------------------------------------------------- setup
  // O_U + cone(row) * NPAD per k-row (int32, launch-wide: the cone table is
  // the batch's), for the SYRK's U rows (Shape::UBT shapes)
  __device__ __forceinline__ int ubt(int row) const { return reinterpret_cast<const int*>(socp_lds + SH::O_UBT)[row]; }
  // The element that lane `ln` holds in slot s.  Pure-slot kernels honour the
  // launch's rotation (SmallArgs::slot_rot, 0 or 64): slot 0 then starts at
  // element k - 64 and slot 1 at element 0 -- a wave-uniform base per slot,
  // no wrap inside a slot.  The k-vectors in LDS, G's rows and HBM keep the
  // problem's order -- only the cone vector ops, which work slot by slot, see
  // the rotation, so a rotated launch moves no data and no row pass.  The lanes
  // 64 s + ln >= k hold no element (their index is only read from).
  __device__ __forceinline__ int el(int s, int ln) const {
    if constexpr (SLK) {
      const int base = slot_rot() ? (s ? 0 : k - 64) : 64 * s;  // wave-uniform
      return base + ln;
    } else {
      return 64 * s + ln;
    }
  }
  __device__ __forceinline__ void init_tables() {
    if (lane < nc) {
      LDS(O_COFF + lane) = a.cones.offs[lane];
      LDS(O_CDIM + lane) = a.cones.dim[lane];
      LDS(O_CKIND + lane) = a.cones.kind[lane];
      if constexpr (HOIST_CST) {
        lc_soc = a.cones.kind[lane] == SOC_K;
        lc_off = a.cones.offs[lane];
        lc_dim = a.cones.dim[lane];
      }
    }
    for (int i = lane; i < KP; i += 64) {
      int code = 3;
      if (i < k) {
        for (int c = 0; c < nc; ++c) {
          const int o = a.cones.offs[c], d = a.cones.dim[c];
          if (i >= o && i < o + d) {
            code = c * 4 + (a.cones.kind[c] == POC_K ? 0 : (i == o ? 1 : 2));
            break;
          }
        }
      }
      LDS(O_RC + i) = (double)code;
      if constexpr (SH::UBT) reinterpret_cast<int*>(socp_lds + SH::O_UBT)[i] = O_U + (code >> 2) * NPAD;
    }
    // segment partials: entry (v, c, slot) is written only when cone c meets the
    // slot, the same for every problem of the launch; the rest stays zero
    for (int e = lane; e < O_TOTC - O_PART; e += 64) LDS(O_PART + e) = 0.0;
#ifdef SOCP_DIAG
    if (lane < 24) LDS(O_STAMPS + lane) = 0.0;  // all-zero bits: the u64 totals start at 0
#endif
    SYNC();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane);
      const bool ev = 64 * s + lane < k;
      const int code = ev ? (int)LDS(O_RC + i) : 3;
      const int c = ev ? (code >> 2) : 0;
      ci[s] = c;
      kd[s] = ev ? (code & 3) : 3;
      const int eo_ = ev ? (int)LDS(O_COFF + c) : i;
      const int d = ev ? (int)LDS(O_CDIM + c) : 1;
      eo[s] = eo_;  // the cone's first element (its index in the k-vectors)
      // the cone's lanes: from its first position in the slots, eo_ rotated
      int o = eo_;
      if constexpr (SLK) {
        const int rot = slot_rot();  // 0 or 64
        o = eo_ + rot >= k && rot ? eo_ + rot - k : eo_ + rot;
      }
      const int st = o > 64 * s ? o : 64 * s;
      const int en = (o + d) < 64 * (s + 1) ? (o + d) : 64 * (s + 1);
      spn[s] = ev && o < 64 && o + d > 64;
      ssl[s] = ev ? st - 64 * s : lane;
      sle[s] = ev ? en - 1 - 64 * s : -1;
    }
  }

  bool ko_gloaded = false;
  // SOCP_F_SHARED_MATRICES: G (AGPRs) and A (LDS block O_A) hold the batch's
  // one G and A since this wave's first problem.  Nothing else writes them:
  // G's AGPRs are written in load_problem alone, O_A is only read after it.
  // A later problem's load_problem keeps its control flow: G's buffer
  // descriptor gets an empty range (every load returns 0 without touching
  // memory) and the AGPR writes run with no lane enabled (a_put_masked).
  // The m > 32 variants (MQ = 4) keep neither: with G's AGPRs live across the
  // problem loop clang-22 crashes on several of them (the MFMA_FORM fallback of
  // the Makefile would then change how they are built); they change only
  // their addressing and reload the shared G and A per problem, from L2.
  static constexpr bool RES_G = MQ < 4, RES_A = MQ < 4;
  bool mat_resident = false;
  // lane c < nc: its cone's kind and offset (per-cone work without the table
  // round trips)
  bool lc_soc = false;
  int lc_off = 0, lc_dim = 0;
  // OV (init_overlap_kernel): the pipelined load.  Two batches of G stay in
  // flight; batch b + 2 is requested, batch b (the compiler's vmcnt waits) written
  // to the AGPRs, and on a forming load (SmallArgs::init_overlap, G really loaded)
  // its row steps are accumulated into the H tiles straight from the registers
  // they arrived in -- form_H's MFMAs with X = G, in its tile order, row steps
  // ascending from T = 0 -- so the initial point's SYRK runs under the load.
  // The LDS fill and the staging of c, b, h, A run under the first round trip.
  // Returns whether T holds G'G: the caller hands it to run(), nothing is kept
  // in the wave.  A resident shared G (keep_g) is not loaded, so it forms
  // nothing; that problem's initial factorisation takes FAC_IDENT.
  template <bool OV = false>
  __device__ __forceinline__ bool load_problem(int64_t p) {
    MARK_BEGIN("load_problem");
    LANE_IDS();
    const bool shared = (a.flags & F_SHARED) != 0;
    const bool keep = shared && mat_resident;  // wave-uniform
    const bool keep_g = RES_G && keep, keep_a = RES_A && keep;
    bool formed = false;
    const double* Gp = a.G + (shared ? 0 : p * (int64_t)k * n);
    // the vectors and the first chunk of A are requested first: their HBM
    // round trip runs under G's (n, m <= 64 here, k <= 128)
    const double cv = lane < n ? a.c[p * n + lane] : 0.0;
    const double bv = lane < m ? a.b[p * m + lane] : 0.0;
    const double hv0 = lane < k ? a.h[p * k + lane] : 0.0;
    const double hv1 = lane + 64 < k ? a.h[p * k + 64 + lane] : 0.0;
    const double* Ap = a.A + (shared ? 0 : p * (int64_t)m * n);
    const int mn = keep_a ? 0 : m * n;  // a resident A is neither loaded nor stored again
    constexpr int AB = HOIST_CST ? 16 : 8;
    double av[AB];
#pragma unroll
    for (int t = 0; t < AB; ++t) av[t] = (64 * t + lane < mn) ? Ap[64 * t + lane] : 0.0;
    // G -> AGPRs.  a_put is an asm statement the scheduler does not move loads
    // across, so the loads are issued in batches of 16 into VGPRs first (one
    // HBM round trip per batch, not per element).  Raw buffer loads over the
    // problem's G (k n doubles): a padding element (row >= k or col >= n)
    // takes an offset past the range and reads 0 -- no address arithmetic in
    // 64 bits, no branch, no mask per element.
    constexpr int GLOAD_BATCH = 16;
    constexpr int GT = NP * NQ, GB = GLOAD_BATCH;
    // (the base made wave-uniform explicitly: a divergent-looking descriptor
    // would be waterfall-looped around every load)
    const uint64_t gpu = (uint64_t)Gp;
    const uint64_t gbase = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(gpu >> 32)) << 32) |
                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gpu);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)gbase, (short)0, __builtin_amdgcn_readfirstlane(keep_g ? 0 : k * n * (int)sizeof(double)), 0x00020000);
    // lanes that take the loaded G (all or none; made wave-uniform explicitly: the statement wants SGPRs)
    const uint32_t wm = (uint32_t)__builtin_amdgcn_readfirstlane(keep_g ? 0 : -1);
    const uint64_t wmask = ((uint64_t)wm << 32) | wm;
    int colk[NQ];  // byte offset of the lane's column in each column tile, or "out of range"
#pragma unroll
    for (int q = 0; q < NQ; ++q) colk[q] = 16 * q + cl < n ? (16 * q + cl) * k * 8 : 0x40000000;
    // (OV) the batches' registers: a batch is live from its request to its MFMAs, three at a time
    constexpr int NB = OV ? GT / GB : 1;
    uint64_t tb[NB][GB];
    if constexpr (OV) {
      static_assert(!OV || (RES_G && GB % NQ == 0 && GB % 4 == 0 && GT % GB == 0 && NB >= 2 && !(SOCP_KO & 1)),
                    "whole batches of whole row steps");
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < GB; ++t) {
          const int e = b * GB + t;
          const int row = 4 * (e / NQ) + g;
          const int off = row < k ? colk[e % NQ] + row * 8 : 0x40000000;
          tb[b][t] = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(grs, off, 0, 0));
        }
      SCHED_FENCE();
    } else if (!(SOCP_KO & 1) || !ko_gloaded) {
    ko_gloaded = true;
#pragma unroll
    for (int b0 = 0; b0 < GT; b0 += GB) {
      uint64_t tmp[GB];
#pragma unroll
      for (int t = 0; t < GB; ++t) {
        const int e = b0 + t;
        if (e < GT) {
          const int pp = e / NQ, q = e % NQ;
          const int row = 4 * pp + g;
          const int off = row < k ? colk[q] + row * 8 : 0x40000000;
          tmp[t] = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(grs, off, 0, 0));
        }
      }
      if constexpr (!RES_G) {
#pragma unroll
        for (int t = 0; t < GB; ++t) {
          const int e = b0 + t;
          if (e < GT) a_put(G[e / NQ][e % NQ], __longlong_as_double((long long)tmp[t]));
        }
      } else {
#pragma unroll
        for (int t = 0; t < GB; t += 4) {
          const int e = b0 + t;
          if (e + 3 < GT) {
            a_put4_masked(G[e / NQ][e % NQ], G[(e + 1) / NQ][(e + 1) % NQ], G[(e + 2) / NQ][(e + 2) % NQ],
                          G[(e + 3) / NQ][(e + 3) % NQ], tmp[t], tmp[t + 1], tmp[t + 2], tmp[t + 3], wmask);
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (e + u < GT) a_put_masked(G[(e + u) / NQ][(e + u) % NQ], tmp[t + u], wmask);
          }
        }
      }
    }
    }
    for (int e = lane; e < NKV * SH::KS; e += 64) LDS(O_KV + e) = 0.0;
    // (a resident A keeps its block, padding zeros included: the fill starts behind it)
    for (int e = lane + (keep_a ? MPAD * LDA : 0); e < O_U + SH::UAL - O_A; e += 64) LDS(O_A + e) = 0.0;
    mat_resident = shared;
    SYNC();
    if (lane < n) LDS(C_ + lane) = cv;
    if (lane < m) LDS(B_ + lane) = bv;
    if (lane < k) LDS(H_ + lane) = hv0;
    if (lane + 64 < k) LDS(H_ + 64 + lane) = hv1;
    if constexpr (OV) {
      // A is one chunk here, so no reload sits behind G's requests: the stores wait
      // for the chunk alone, not for the batches in flight
      static_assert(!OV || 256 * MQ * NQ <= 64 * AB, "A in one chunk");
#pragma unroll
      for (int t = 0; t < AB; ++t) {
        const int e = 64 * t + lane;
        if (e < mn) LDS(O_A + (e % m) * LDA + e / m) = av[t];
      }
    } else
    for (int e0 = 0; e0 < mn; e0 += 64 * AB) {
#pragma unroll
      for (int t = 0; t < AB; ++t) {
        const int e = e0 + 64 * t + lane;
        if (e < mn) LDS(O_A + (e % m) * LDA + e / m) = av[t];
      }
      const int e1 = e0 + 64 * AB;
      if (e1 < mn) {
#pragma unroll
        for (int t = 0; t < AB; ++t) av[t] = (e1 + 64 * t + lane < mn) ? Ap[e1 + 64 * t + lane] : 0.0;
      }
    }
    SYNC();
    if constexpr (OV) {
      // (everything above ran under the first two batches' round trip)
      const bool form = __builtin_amdgcn_readfirstlane(a.init_overlap != 0 && !keep_g) != 0;  // wave-uniform
      // (the lane mask again, next to its statements: they want it in SGPRs)
      const uint32_t wm2 = (uint32_t)__builtin_amdgcn_readfirstlane(keep_g ? 0 : -1);
      const uint64_t wmask2 = ((uint64_t)wm2 << 32) | wm2;
      SCHED_FENCE();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b + 2 < NB) {
#pragma unroll
          for (int t = 0; t < GB; ++t) {
            const int e = (b + 2) * GB + t;
            const int row = 4 * (e / NQ) + g;
            const int off = row < k ? colk[e % NQ] + row * 8 : 0x40000000;
            tb[b + 2 < NB ? b + 2 : 0][t] = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(grs, off, 0, 0));
          }
        }
        SCHED_FENCE();
#pragma unroll
        for (int t = 0; t < GB; t += 4) {
          const int e = b * GB + t;
          a_put4_masked(G[e / NQ][e % NQ], G[(e + 1) / NQ][(e + 1) % NQ], G[(e + 2) / NQ][(e + 2) % NQ],
                        G[(e + 3) / NQ][(e + 3) % NQ], tb[b][t], tb[b][t + 1], tb[b][t + 2], tb[b][t + 3], wmask2);
        }
        SCHED_FENCE();
        if (form) {
          if (b == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) T[t] = (d4){0.0, 0.0, 0.0, 0.0};
          }
#pragma unroll
          for (int r = 0; r < GB / NQ; ++r) {  // the batch's row steps, form_H's products with X = G
            double X[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) X[q] = __longlong_as_double((long long)tb[b][r * NQ + q]);
#pragma unroll
            for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
              for (int tj = 0; tj <= ti; ++tj) T[tri(ti, tj)] = mfma(X[tj], X[ti], T[tri(ti, tj)]);
          }
        }
        SCHED_FENCE();
      }
      formed = form;
    }
    return formed;
  }

  __device__ __forceinline__ double e_of(int i) const {
    const int code = (int)LDS(O_RC + i) & 3;
    return (code == 0 || code == 1) ? 1.0 : 0.0;
  }

  // W = I: the initial-point system (solver.jl:68-84) is the KKT system with
  // W = I, lam = e, ds = 0.
  __device__ __forceinline__ void scaling_identity() {
    for (int i = lane; i < k; i += 64) {
      const double e = e_of(i);
      LDS(WB + i) = e;
      LDS(LAM + i) = e;
      LDS(CA + i) = 1.0;
      LDS(CBV + i) = 0.0;
      LDS(IL + i) = e;  // 1/lambda_i of the POC elements (lambda = e)
    }
    for (int e = lane; e < NCS * NPAD; e += 64) LDS(O_U + e) = 0.0;
    if (lane < nc) {  // W = I, lambda = e: mu = wbar_0 = lambda_0 = 1, wbar_1 = lambda_1 = 0
      const int c = lane;
      LDS(cc(CC_MU, c)) = 1.0;
      LDS(cc(CC_IMU, c)) = 1.0;
      LDS(cc(CC_WB0, c)) = 1.0;
      LDS(cc(CC_I1, c)) = 0.5;
      LDS(cc(CC_W2, c)) = 0.0;
      LDS(cc(CC_L0, c)) = 1.0;
      LDS(cc(CC_AA, c)) = 1.0;
      LDS(cc(CC_IAA, c)) = 1.0;
      LDS(cc(CC_IL0, c)) = 1.0;
      LDS(cc(CC_IL0AA, c)) = 1.0;
      LDS(cc(CC_SA, c)) = 1.0;
      LDS(cc(CC_SAL, c)) = 0.5;
      LDS(cc(CC_WL, c)) = 0.0;
    }
    SYNC();
  }

  // ------------------------------------------------------ cone vector ops
  // The k-vector lives in two 64-element slots (element i = 64 s + lane).  Every
  // SOC operation of the reference (scale!/iscale!, iprod!/vprod!, the SOC
  // branch of compute_scaling, scmax) needs one or two per-cone dot products;
  // they come from cone_reduce, and each op below is straight-line code over
  // registers: the values a cone head holds (x_0, the cone constants) are
  // recomputed or read by every lane of the cone instead of being broadcast.

  // Per-cone (segmented) reduction of NV values per slot.  v[s][q] holds the
  // lane's contribution for element 64 s + lane; on return every lane of a cone
  // holds the cone total -- a sum, or a max for the values flagged in MX.  DPP
  // inclusive scan inside each slot, then the segment-end lanes hand their
  // partials over through LDS (a cone may span both slots).
  // The slots' scans run interleaved step by step (independent DPP chains
  // hide each other's latency); the DPP moves write every lane, so no old value
  // is materialised (lanes a pattern leaves unwritten fail the step's
  // predicate); all partials are read before any is used.
  // Live masks (L0, L1: bit q set = value q of slot 0 / 1 is needed): a pure
  // slot hands the reductions only the values its cone kind uses.  The values
  // are reduced independently of each other, so leaving some out changes no
  // result; with every bit set the code is the unmasked one.
  static constexpr unsigned LIVE_ALL = ~0u;
  static constexpr bool live(unsigned L0, unsigned L1, int s, int q) { return (((s ? L1 : L0) >> q) & 1u) != 0; }
  static constexpr int live_pos(unsigned L0, unsigned L1, int NV, int s, int q) {
    int c = 0;
    for (int t = 0; t < 2; ++t)
      for (int r = 0; r < NV; ++r) {
        if (t == s && r == q) return c;
        if (live(L0, L1, t, r)) ++c;
      }
    return c;
  }
  static constexpr int live_count(unsigned L0, unsigned L1, int NS, int NV) { return live_pos(L0, L1, NV, NS, 0); }
  static constexpr unsigned live_mx(unsigned MX, unsigned L0, unsigned L1, int NS, int NV) {
    unsigned m = 0;
    for (int t = 0; t < NS; ++t)
      for (int r = 0; r < NV; ++r)
        if (live(L0, L1, t, r) && ((MX >> r) & 1u)) m |= 1u << live_pos(L0, L1, NV, t, r);
    return m;
  }
  template <int NV, unsigned MX, unsigned L0 = LIVE_ALL, unsigned L1 = LIVE_ALL>
  __device__ __forceinline__ void cone_reduce(double (&v)[2][NV]) {
    MARK_BEGIN("cone_reduce");
    LANE_IDS();
    constexpr int NS = KP > 64 ? 2 : 1;  // slots that can hold elements of this shape
    if (al_rows()) {  // row-aligned cones: registers only
      const int R = al_rows();
      constexpr int NL = live_count(L0, L1, NS, NV);
      constexpr unsigned MXM = live_mx(MX, L0, L1, NS, NV);
      if constexpr (NL > 0) {
        double w[NL];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int q = 0; q < NV; ++q)
            if (live(L0, L1, s, q)) w[live_pos(L0, L1, NV, s, q)] = v[s][q];
        cone_allreduce_rows_n<NL, MXM>(w, R);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int q = 0; q < NV; ++q)
            if (live(L0, L1, s, q)) v[s][q] = w[live_pos(L0, L1, NV, s, q)];
      }
      return;
    }
    const int rl = lane & 15;
#define SOCP_SCAN_STEP(CTRL, OK)                                         \
  _Pragma("unroll") for (int s = 0; s < NS; ++s) {                       \
    const int st = ssl[s];                                               \
    const bool ok_ = (OK);                                               \
    _Pragma("unroll") for (int q = 0; q < NV; ++q) {                     \
      if (!live(L0, L1, s, q)) continue;                                 \
      const double y = dpp_all<CTRL>(v[s][q]);                           \
      const double r = ((MX >> q) & 1) ? fmax(v[s][q], y) : v[s][q] + y; \
      v[s][q] = ok_ ? r : v[s][q];                                       \
    }                                                                    \
  }
    SOCP_SCAN_STEP(0x111, rl >= 1 && lane - 1 >= st)
    SOCP_SCAN_STEP(0x112, rl >= 2 && lane - 2 >= st)
    SOCP_SCAN_STEP(0x114, rl >= 4 && lane - 4 >= st)
    SOCP_SCAN_STEP(0x118, rl >= 8 && lane - 8 >= st)
    SOCP_SCAN_STEP(0x142, ((lane >> 4) & 1) && ((lane & ~15) - 1 >= st))
    SOCP_SCAN_STEP(0x143, lane >= 32 && 31 >= st)
#undef SOCP_SCAN_STEP
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (lane == sle[s]) {
#pragma unroll
        for (int q = 0; q < NV; ++q)
          if (live(L0, L1, s, q)) LDS(O_PART + (q * NCS + ci[s]) * 2 + s) = v[s][q];
      }
    }
    SYNC();
    double pp[NS][NV][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        if (!live(L0, L1, s, q)) continue;
        pp[s][q][0] = LDS(O_PART + (q * NCS + ci[s]) * 2);
        pp[s][q][1] = LDS(O_PART + (q * NCS + ci[s]) * 2 + 1);
      }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        if (!live(L0, L1, s, q)) continue;
        const double p0 = pp[s][q][0], p1 = pp[s][q][1];
        const double both = ((MX >> q) & 1) ? fmax(p0, p1) : p0 + p1;
        v[s][q] = spn[s] ? both : (s == 0 ? p0 : p1);
      }
  }

  // The scan half of cone_reduce for sums: the segment-end lanes leave the
  // two slot partials of every cone in O_PART; cone_tot(q, c) adds them (the
  // unused (cone, slot) entries stay zero).  For per-cone work done once per
  // cone (on "cone lanes", lane c < nc) instead of once per element.
  template <int NV, unsigned L0 = LIVE_ALL, unsigned L1 = LIVE_ALL>
  __device__ __forceinline__ void cone_partials(double (&v)[2][NV]) {
    MARK_BEGIN("cone_partials");
    LANE_IDS();
    constexpr int NS = KP > 64 ? 2 : 1;
    const int rl = lane & 15;
    if (al_rows()) {  // row-aligned cones: every lane of the cone gets its total
      const int R = al_rows();
      constexpr int NL = live_count(L0, L1, NS, NV);
      if constexpr (NL > 0) {
        double w[NL];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int q = 0; q < NV; ++q)
            if (live(L0, L1, s, q)) w[live_pos(L0, L1, NV, s, q)] = v[s][q];
        cone_allreduce_rows_n<NL, 0u>(w, R);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int q = 0; q < NV; ++q)
            if (live(L0, L1, s, q)) v[s][q] = w[live_pos(L0, L1, NV, s, q)];
      }
    } else {
#define SOCP_SCAN_STEP(CTRL, OK)                         \
  _Pragma("unroll") for (int s = 0; s < NS; ++s) {       \
    const int st = ssl[s];                               \
    const bool ok_ = (OK);                               \
    _Pragma("unroll") for (int q = 0; q < NV; ++q) {     \
      if (!live(L0, L1, s, q)) continue;                 \
      const double y = dpp_all<CTRL>(v[s][q]);           \
      v[s][q] = ok_ ? v[s][q] + y : v[s][q];             \
    }                                                    \
  }
    SOCP_SCAN_STEP(0x111, rl >= 1 && lane - 1 >= st)
    SOCP_SCAN_STEP(0x112, rl >= 2 && lane - 2 >= st)
    SOCP_SCAN_STEP(0x114, rl >= 4 && lane - 4 >= st)
    SOCP_SCAN_STEP(0x118, rl >= 8 && lane - 8 >= st)
    SOCP_SCAN_STEP(0x142, ((lane >> 4) & 1) && ((lane & ~15) - 1 >= st))
    SOCP_SCAN_STEP(0x143, lane >= 32 && 31 >= st)
#undef SOCP_SCAN_STEP
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (lane == sle[s]) {
#pragma unroll
        for (int q = 0; q < NV; ++q)
          if (live(L0, L1, s, q)) LDS(O_PART + (q * NCS + ci[s]) * 2 + s) = v[s][q];
      }
    }
    SYNC();
  }
  __device__ __forceinline__ double cone_tot(int q, int c) const {
    return LDS(O_PART + (q * NCS + c) * 2) + LDS(O_PART + (q * NCS + c) * 2 + 1);
  }

  __device__ __forceinline__ double ccv(int q, int c) const { return LDS(cc(q, c)); }

  // max over cones of the value the first lane of every cone stored at O_TOTC + off
  __device__ __forceinline__ double cone_max(int off) const {
    double t = -INFINITY, v[NCS];  // all reads in one round trip (the entries c >= nc are not used)
#pragma unroll
    for (int c = 0; c < NCS; ++c) v[c] = LDS(O_TOTC + off + c);
#pragma unroll
    for (int c = 0; c < NCS; ++c) t = c < nc ? fmax(t, v[c]) : t;
    return t;
  }

  // reciprocal and reciprocal square root: hardware estimate + Newton steps
  // (within an ulp or two of the IEEE quotient: the parity gates are relative
  // 1e-9, and these replace IEEE divisions in per-element and per-cone math)
  __device__ __forceinline__ static double rcp_nr(double d) { return recip(d); }

  // ---- slot kinds.  Each cone vector op below is a template over the kinds
  // (SL0, SL1) of the two slots, instantiated with the kernel's (KS0, KS1): no
  // branch, one copy of each op per kernel.  In the body, for slot s:
  //   pocs(K, kd): "take the POC value" -- constant in a pure slot (true in a
  //                POC slot, where the lanes without an element compute values
  //                nobody stores), the type code's test in a mixed one;
  //   pocm(K, kd): a POC element is here (a mask: stores, reduction inputs);
  //   tailm / headm: an SOC tail / head element is here, never in a POC slot.
  // The compiler drops the other kind's chain, its constant reads and the
  // selects between the two.  (SL0, SL1) = mixed is the code as it was.
#define SOCP_SK(s) ((s) == 0 ? SL0 : SL1)
  // Rounding: the per-slot bodies below run with FMA contraction off and name
  // every fused product themselves.  Left to -ffp-contract=fast, each compiled
  // instance of a body (slot 0's and slot 1's, mixed and pure) fuses a*b + c*d
  // its own way, and an element then rounds differently depending on the slot
  // it sits in -- a rotated launch would not repeat the bits of a plain one.
  // The code outside these bodies holds no other sum of two products (the cone
  // lanes' nsum is named too); single products fuse the same way everywhere.
  static __device__ __forceinline__ bool pocs(int K, int kd_) { return may_poc(K) && (!may_soc(K) || kd_ == 0); }
  static __device__ __forceinline__ bool pocm(int K, int kd_) { return may_poc(K) && kd_ == 0; }
  static __device__ __forceinline__ bool tailm(int K, int kd_) { return may_soc(K) && kd_ == 2; }
  static __device__ __forceinline__ bool headm(int K, int kd_) { return may_soc(K) && kd_ == 1; }
#define SOCP_SLOT_DISPATCH(F, ...) return F<KS0, KS1>(__VA_ARGS__)

  // compute_scaling (scalings.jl:22-110) and ds = lam o lam (solver.jl:120).
  // Writes WB (wbar / sqrt(s/z)), LAM, IL (1/lambda of the POC elements), the
  // X = W^-1 G row coefficients CA, CBV, DS (write_ds: the iteration's
  // lam o lam; the KKT entry keeps its ds) and the per-cone constants; ll =
  // lam'lam.  Returns the DomainError flag; dm_aa flags a negative
  // lambda_0^2 - |lambda_1|^2 (scmax's sqrt, mats.jl:66), which the reference
  // raises later, at compute_step.
  // Two segmented reductions; the SOC cone math (norms, gamma, mu, lambda_0 and
  // the coefficients of the tail rows) runs once per cone on lane c, not once
  // per element.
  // For MP_KKT only.  These are the operations of resid_scaling_k's scaling
  // half (its scaling-only instantiation is what a SOCP_KO 2 build runs), kept
  // as a body of its own: every solver kernel compiles MP_KKT, and with that
  // instantiation laid into them in this body's place C2's solves ran 1 %
  // slower, though a solve never enters it.
  __device__ __forceinline__ bool scaling_op(double& ll, bool& dm_aa, bool write_ds) {
    SOCP_SLOT_DISPATCH(scaling_op_k, ll, dm_aa, write_ds);
  }
  template <int SL0, int SL1>
  __device__ __forceinline__ bool scaling_op_k(double& ll, bool& dm_aa, bool write_ds) {
    MARK_BEGIN("scaling_op");
    if (SOCP_KO & 4096) {
      ll = 1.0;
      dm_aa = false;
      return false;
    }
    LANE_IDS();
    double v[2][3], zi[2], si[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane);
      zi[s] = LDS(Z_ + i);
      si[s] = LDS(S_ + i);
      const bool tail = tailm(SOCP_SK(s), kd[s]);
      v[s][0] = tail ? zi[s] * zi[s] : 0.0;
      v[s][1] = tail ? si[s] * si[s] : 0.0;
      v[s][2] = tail ? zi[s] * si[s] : 0.0;
    }
    cone_partials<3, may_soc(SL0) ? 7u : 0u, may_soc(SL1) ? 7u : 0u>(v);
    MARK_BEGIN("scal_cone1");
    bool dm = false;
    // ---- cone lanes: the SOC branch of compute_scaling (scalings.jl:32-99)
    if (HOIST_CST ? lc_soc : (lane < nc && (int)LDS(O_CKIND + lane) == SOC_K)) {
      const int c = lane, o = HOIST_CST ? lc_off : (int)LDS(O_COFF + c);
      const double z0 = LDS(Z_ + o), s0 = LDS(S_ + o);
      const double onrmz = z0 * z0 - cone_tot(0, c), onrms = s0 * s0 - cone_tot(1, c);
      // the square roots and their reciprocals from one Newton-refined rsq each
      const double fz = rsqrt_nr(onrmz), fs = rsqrt_nr(onrms);
      const double nrmz = onrmz * fz, nrms = onrms * fs;
      const double zb0 = z0 * fz, sb0 = s0 * fs;
      const double nsum = fma(zb0, sb0, cone_tot(2, c) * fz * fs);  // (named: two products, one sum)
      const double garg = (1.0 + nsum) * 0.5;
      const double rg = rsqrt_nr(garg);
      const double gamma = garg * rg;
      const double fg = 0.5 * rg;
      const double wb0 = (sb0 + zb0) * fg;
      const double ratio = nrms * fz, prod = nrms * nrmz;
      const double im = rsqrt_nr(ratio), mu = ratio * im, tmv1 = sqrt_nr(prod);
      const double mult = tmv1 * recip(zb0 + sb0 + 2.0 * gamma);
      const double l0 = gamma * tmv1;
      dm = (onrmz < 0.0) || (onrms < 0.0) || (garg < 0.0) || (ratio < 0.0) || (prod < 0.0);
      LDS(cc(CC_MU, c)) = mu;
      LDS(cc(CC_IMU, c)) = im;
      LDS(cc(CC_WB0, c)) = wb0;
      LDS(cc(CC_I1, c)) = recip(1.0 + wb0);
      LDS(cc(CC_L0, c)) = l0;
      LDS(cc(CC_AS, c)) = fs * fg;  // wbar_i = (s_i/|s| - z_i/|z|) / (2 gamma)
      LDS(cc(CC_AZ, c)) = fz * fg;
      LDS(cc(CC_BS, c)) = fs * (gamma + zb0) * mult;  // lambda_i (scalings.jl:91-97)
      LDS(cc(CC_BZ, c)) = fz * (gamma + sb0) * mult;
      LDS(WB + o) = wb0;
      LDS(LAM + o) = l0;
      LDS(CA + o) = -im;
      LDS(CBV + o) = -(1.0 + wb0) * im;
    }
    SYNC();
    MARK_BEGIN("scal_elem");
    // ---- elements: POC (scalings.jl:22-30) and the SOC tails
    double li[2], wbi[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
      const int i = el(s, lane), c = ci[s];
      const bool poc = pocs(SOCP_SK(s), kd[s]), pm = pocm(SOCP_SK(s), kd[s]), tail = tailm(SOCP_SK(s), kd[s]);
      // POC: one 1/sqrt(s z) gives sqrt(s/z) = s q, sqrt(z/s) = z q, sqrt(s z) = (s z) q
      const double pr = si[s] * zi[s];
      const double q = rsqrt_nr(pr);
      const double as = ccv(CC_AS, c), az = ccv(CC_AZ, c), bs = ccv(CC_BS, c), bz = ccv(CC_BZ, c);
      const double imu = ccv(CC_IMU, c), l0 = ccv(CC_L0, c);
      const double wt = fma(si[s], as, -(zi[s] * az));
      const double lt = fma(si[s], bs, zi[s] * bz);
      dm = dm || (pm && pr < 0.0);
      wbi[s] = poc ? zmul(si[s], q) : (tail ? wt : ccv(CC_WB0, c));
      li[s] = poc ? zmul(pr, q) : (tail ? lt : l0);
      if (pm || tail) {
        LDS(WB + i) = wbi[s];
        LDS(LAM + i) = li[s];
        LDS(CA + i) = poc ? zmul(zi[s], q) : imu;
        LDS(CBV + i) = poc ? 0.0 : wt * imu;
        if (pm) LDS(IL + i) = q;
        if (write_ds) LDS(DS + i) = -(poc ? li[s] * li[s] : fma(l0, li[s], l0 * li[s]));  // -ds: the RHS
      }
      // lam o lam head (vprod!, vectors.jl:58-75) and |lambda_1|^2 (POC: the
      // cone's sum of lambda_i^2, its share of lam'lam), |wbar_1|^2, wbar_1'lambda_1
      v[s][0] = (pm || tail) ? li[s] * li[s] : 0.0;
      v[s][1] = tail ? wbi[s] * wbi[s] : 0.0;
      v[s][2] = tail ? wbi[s] * li[s] : 0.0;
    }
    cone_partials<3, may_soc(SL0) ? 7u : 1u, may_soc(SL1) ? 7u : 1u>(v);
    MARK_BEGIN("scal_cone2");
    bool da = false;
    double tl = 0.0;
    if (lane < nc) {
      const int c = lane;
      const double l1 = cone_tot(0, c);
      if (HOIST_CST ? lc_soc : (int)LDS(O_CKIND + c) == SOC_K) {
        const int o = HOIST_CST ? lc_off : (int)LDS(O_COFF + c);
        const double l0 = LDS(cc(CC_L0, c));
        const double aa = l0 * l0 - l1;
        da = aa < 0.0;
        const double sa = rsqrt_nr(aa);
        LDS(cc(CC_W2, c)) = cone_tot(1, c);
        LDS(cc(CC_WL, c)) = cone_tot(2, c);
        LDS(cc(CC_AA, c)) = aa;
        LDS(cc(CC_IAA, c)) = recip(aa);
        LDS(cc(CC_IL0, c)) = recip(l0);
        LDS(cc(CC_IL0AA, c)) = recip(l0 * aa);
        LDS(cc(CC_SA, c)) = sa;
        LDS(cc(CC_SAL, c)) = recip(sa * l0 + 1.0);
        tl = l0 * l0 + l1;
        if (write_ds) LDS(DS + o) = -tl;
      } else {
        tl = l1;
      }
    }
    SYNC();
    ll = wsum(tl);
    dm_aa = __any(da);
    return __any(dm);
  }

  // The per-cone SOC branch of compute_scaling (scalings.jl:32-99) on cone lane
  // c = lane, computed on every lane (branch-free: its instructions share the
  // caller's scheduling region) and stored by the SOC cone lanes only.
  struct ScalCone1 {
    double mu, im, wb0, i1, l0, as, az, bs, bz;
    bool dm;
  };
  __device__ __forceinline__ ScalCone1 scal_cone1_math(int o, int c) const {
    ScalCone1 r;
    const double z0 = LDS(Z_ + o), s0 = LDS(S_ + o);
    const double onrmz = z0 * z0 - cone_tot(0, c), onrms = s0 * s0 - cone_tot(1, c);
    const double fz = rsqrt_nr(onrmz), fs = rsqrt_nr(onrms);
    const double nrmz = onrmz * fz, nrms = onrms * fs;
    const double zb0 = z0 * fz, sb0 = s0 * fs;
    const double nsum = fma(zb0, sb0, cone_tot(2, c) * fz * fs);  // (named: two products, one sum)
    const double garg = (1.0 + nsum) * 0.5;
    const double rg = rsqrt_nr(garg);
    const double gamma = garg * rg;
    const double fg = 0.5 * rg;
    r.wb0 = (sb0 + zb0) * fg;
    const double ratio = nrms * fz, prod = nrms * nrmz;
    r.im = rsqrt_nr(ratio);
    r.mu = ratio * r.im;
    const double tmv1 = sqrt_nr(prod);
    const double mult = tmv1 * recip(zb0 + sb0 + 2.0 * gamma);
    r.l0 = gamma * tmv1;
    r.dm = (onrmz < 0.0) || (onrms < 0.0) || (garg < 0.0) || (ratio < 0.0) || (prod < 0.0);
    r.i1 = recip(1.0 + r.wb0);
    r.as = fs * fg;
    r.az = fz * fg;
    r.bs = fs * (gamma + zb0) * mult;
    r.bz = fz * (gamma + sb0) * mult;
    return r;
  }
  __device__ __forceinline__ void scal_cone1_store(const ScalCone1& r, int o, int c) {
    LDS(cc(CC_MU, c)) = r.mu;
    LDS(cc(CC_IMU, c)) = r.im;
    LDS(cc(CC_WB0, c)) = r.wb0;
    LDS(cc(CC_I1, c)) = r.i1;
    LDS(cc(CC_L0, c)) = r.l0;
    LDS(cc(CC_AS, c)) = r.as;  // wbar_i = (s_i/|s| - z_i/|z|) / (2 gamma)
    LDS(cc(CC_AZ, c)) = r.az;
    LDS(cc(CC_BS, c)) = r.bs;  // lambda_i (scalings.jl:91-97)
    LDS(cc(CC_BZ, c)) = r.bz;
    LDS(WB + o) = r.wb0;
    LDS(LAM + o) = r.l0;
    LDS(CA + o) = -r.im;
    LDS(CBV + o) = -(1.0 + r.wb0) * r.im;
  }

  // gemv_Gt hook: the cone-lane chain in the first batch of G'z
  struct ScalHook {
    Small& S;
    ScalCone1& r;
    int o, c;
    template <int B>
    __device__ __forceinline__ void run() {
      if constexpr (B == 0) r = S.scal_cone1_math(o, c);
    }
  };

  // MP_ITER: the residuals (solver.jl:109-118) and compute_scaling (:106) with
  // ds = lam o lam (:120) in one pass.  They are independent (the scaling
  // reads z and s, the residuals x, y, z, s), so their phases share
  // scheduling regions: the scaling's cone-lane chains (rsqrt / recip
  // latency on three lanes) run inside the residuals' G'z pass and beside
  // their G x pass (VALU issue), the element part beside the A products (LDS
  // latency).  The only copy of the residuals, and the iteration's only copy
  // of the scaling (MP_KKT has scaling_op).  RESID / SCAL pick the halves that
  // run: the SOCP_KO 2 / 4096 builds drop the residuals / the scaling -- each
  // half's operations, and so its bits, are those of the interleaved pass.
  // Returns the DomainError flag.
  template <bool RESID = true, bool SCAL = true>
  __device__ __forceinline__ bool resid_scaling(double& nd, double& np_, double& gap, double& ll, bool& dm_aa) {
    return resid_scaling_k<KS0, KS1, RESID, SCAL>(nd, np_, gap, ll, dm_aa);
  }
  template <int SL0, int SL1, bool RESID, bool SCAL>
  __device__ __forceinline__ bool resid_scaling_k(double& nd, double& np_, double& gap, double& ll, bool& dm_aa) {
    MARK_BEGIN("resid_scaling");
    LANE_IDS();
    constexpr int NS = KP > 64 ? 2 : 1;
    // rd = A'y + G'z + c (QP: + Px), rp = Ax - b, rz = Gx + s - h (solver.jl:109-118):
    // the small operands read up front, in one round trip: c and x (column
    // layout), z and s (slot layout)
    double cq[NQ], xq[NQ], zv[NS], sv[NS];
    double pq[NQ];  // QP: (P x)[16q+cl], formed first, while few registers are live
    if constexpr (RESID) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        cq[q] = LDS(C_ + 16 * q + cl);
        xq[q] = LDS(X_ + 16 * q + cl);
      }
#pragma unroll
      for (int t = 0; t < NS; ++t) {  // z's: summed over the fixed pairing 64 t + lane, rotated slots or not
        zv[t] = LDS(Z_ + 64 * t + lane);
        sv[t] = LDS(S_ + 64 * t + lane);
      }
      if constexpr (QP) P_mv(X_, pq);
    }
    // ---- scaling, first reduction: |z_1|^2, |s_1|^2, z_1's_1 per cone
    double v[2][3], zi[2], si[2];
    if constexpr (SCAL) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int i = el(s, lane);
        zi[s] = LDS(Z_ + i);
        si[s] = LDS(S_ + i);
        const bool tail = tailm(SOCP_SK(s), kd[s]);
        v[s][0] = tail ? zi[s] * zi[s] : 0.0;
        v[s][1] = tail ? si[s] * si[s] : 0.0;
        v[s][2] = tail ? zi[s] * si[s] : 0.0;
      }
      cone_partials<3, may_soc(SL0) ? 7u : 0u, may_soc(SL1) ? 7u : 0u>(v);
    }
    // ---- the cone-lane chain inside G'z's first batch (on its own where no G'z pass runs)
    const bool socl = HOIST_CST ? lc_soc : (lane < nc && (int)LDS(O_CKIND + lane) == SOC_K);
    const int cc_ = lane < nc ? lane : 0;
    const int oc = socl ? (HOIST_CST ? lc_off : (int)LDS(O_COFF + lane)) : 0;
    ScalCone1 c1;
    double acc[NQ], at[NQ];
    if constexpr (!RESID || (SOCP_KO & 32)) {
      if constexpr (SCAL) c1 = scal_cone1_math(oc, cc_);
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    } else if constexpr (SCAL) {
      gemv_Gt(Z_, acc, ScalHook{*this, c1, oc, cc_});
    } else {
      gemv_Gt(Z_, acc);
    }
    bool dm = false;
    if constexpr (SCAL) {
      if (socl) scal_cone1_store(c1, oc, cc_);
      dm = socl && c1.dm;
      SYNC();
      // ---- the elements (POC, scalings.jl:22-30; SOC tails) beside A'y
      MARK_BEGIN("scal_elem");
      double li[2], wbi[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
        const int i = el(s, lane), c = ci[s];
        const bool poc = pocs(SOCP_SK(s), kd[s]), pm = pocm(SOCP_SK(s), kd[s]), tail = tailm(SOCP_SK(s), kd[s]);
        // POC: one 1/sqrt(s z) gives sqrt(s/z) = s q, sqrt(z/s) = z q, sqrt(s z) = (s z) q
        const double pr = si[s] * zi[s];
        const double q = rsqrt_nr(pr);
        const double as = ccv(CC_AS, c), az = ccv(CC_AZ, c), bs = ccv(CC_BS, c), bz = ccv(CC_BZ, c);
        const double imu = ccv(CC_IMU, c), l0 = ccv(CC_L0, c);
        const double wt = fma(si[s], as, -(zi[s] * az));
        const double lt = fma(si[s], bs, zi[s] * bz);
        dm = dm || (pm && pr < 0.0);
        wbi[s] = poc ? zmul(si[s], q) : (tail ? wt : ccv(CC_WB0, c));
        li[s] = poc ? zmul(pr, q) : (tail ? lt : l0);
        if (pm || tail) {
          LDS(WB + i) = wbi[s];
          LDS(LAM + i) = li[s];
          LDS(CA + i) = poc ? zmul(zi[s], q) : imu;
          LDS(CBV + i) = poc ? 0.0 : wt * imu;
          if (pm) LDS(IL + i) = q;
          LDS(DS + i) = -(poc ? li[s] * li[s] : fma(l0, li[s], l0 * li[s]));  // -ds: the RHS
        }
        // lam o lam head (vprod!, vectors.jl:58-75) and |lambda_1|^2 (POC: the
        // cone's sum of lambda_i^2, its share of lam'lam), |wbar_1|^2, wbar_1'lambda_1
        v[s][0] = (pm || tail) ? li[s] * li[s] : 0.0;
        v[s][1] = tail ? wbi[s] * wbi[s] : 0.0;
        v[s][2] = tail ? wbi[s] * li[s] : 0.0;
      }
    }
    if constexpr (RESID && !(SOCP_KO & 128)) {
      At_mv(Y_, at);
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) at[q] = 0.0;
    }
    if constexpr (SCAL) cone_partials<3, may_soc(SL0) ? 7u : 1u, may_soc(SL1) ? 7u : 1u>(v);
    // ---- rd, the second cone-lane part beside A x and G x + s - h
    double d2 = 0.0, p2 = 0.0, zs = 0.0;
    if constexpr (RESID) {
      if (g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int j = 16 * q + cl;
          if (j < n) {
            double vv = (at[q] + acc[q]) + cq[q];
            if constexpr (QP) vv += pq[q];
            LDS(RD + j) = -vv;  // the residuals are stored negated: the affine RHS (solver.jl:124)
            d2 = fma(vv, vv, d2);
          }
        }
      }
      if constexpr (!(SOCP_KO & 128)) p2 = A_mv(X_, B_, RP, O_A, true);
    }
    bool da = false;
    double tl = 0.0;
    {
      MARK_BEGIN("scal_cone2");
      // (computed on every lane, stored by the SOC cone lanes; without SCAL nothing below uses them)
      const double l1 = cone_tot(0, cc_);
      const double l0 = LDS(cc(CC_L0, cc_));
      const double aa = l0 * l0 - l1;
      const double sa = rsqrt_nr(aa);
      const double w2 = cone_tot(1, cc_), wl = cone_tot(2, cc_);
      const double iaa = recip(aa), il0 = recip(l0), il0aa = recip(l0 * aa), sal = recip(sa * l0 + 1.0);
      // Fused launches: the pass forms U as well -- WB and CC_I1 of this
      // scaling are stored and fenced by now.  One wave-uniform branch per
      // pass picks the instance, and the fused one is laid out of line (expected not taken): a launch that does not fuse
      // runs the instruction stream it ran before the fusion existed.  With
      // the U parts behind branches inside one shared instance those launches
      // lost 0.2-0.6 ms at C2's shape.
      if constexpr (RESID && !(SOCP_KO & 16)) {
        if (__builtin_expect(SCAL && !(SOCP_KO & 4) && fuse_u(), 0))
          gemv_G_r<true, true>(xq, S_, H_, DZ);
        else
          gemv_G_r<true>(xq, S_, H_, DZ);
      }
      if constexpr (SCAL) {
        if (lane < nc) {
          if (socl) {
            da = aa < 0.0;
            LDS(cc(CC_W2, cc_)) = w2;
            LDS(cc(CC_WL, cc_)) = wl;
            LDS(cc(CC_AA, cc_)) = aa;
            LDS(cc(CC_IAA, cc_)) = iaa;
            LDS(cc(CC_IL0, cc_)) = il0;
            LDS(cc(CC_IL0AA, cc_)) = il0aa;
            LDS(cc(CC_SA, cc_)) = sa;
            LDS(cc(CC_SAL, cc_)) = sal;
            tl = l0 * l0 + l1;
            LDS(DS + oc) = -tl;
          } else {
            tl = l1;
          }
        }
      }
    }
    SYNC();
    if constexpr (RESID) {
#pragma unroll
      for (int t = 0; t < NS; ++t)
        if (64 * t + lane < k) zs = fma(zv[t], sv[t], zs);  // (explicit: every instantiation sums z's alike, socp_batch_solve_qp's res at P = 0 included)
      double r3[3] = {d2, p2, zs};  // the three whole-wave sums in one interleaved scan
      dpp_scan<3>(r3, lane, 0, false);
      nd = sqrt(readlane_d(r3[0], 63));
      np_ = sqrt(readlane_d(r3[1], 63));
      gap = readlane_d(r3[2], 63);
    } else {
      nd = np_ = gap = 1.0;
    }
    ll = SCAL ? wsum(tl) : 1.0;
    dm_aa = __any(da);
    return __any(dm);
  }

  // First half of solve_kkt(::DenseSolver) (densesolver.jl:61-66):
  //   k0 = lam^-1 o ds (iprod!), k1 = W k0 (scale!), k2 = dz - k1,
  //   t2 = iWiW k2 = W^-1 (W^-1 k2).
  // Every SOC dot product the chain needs follows by linearity from three dots
  // of the inputs, taken in ONE reduction: t = lambda_1'ds_1 (iprod!'s),
  // u = wbar_1'ds_1, w = wbar_1'dz_1, with the scaling's wbar_1'lambda_1 and
  // |wbar_1|^2:  wbar_1'k0_1 = -ds_0 WL/aa + u/lambda_0 + WL t/(lambda_0 aa),
  // wbar_1'k1_1 = mu (delta + (k0_0 + delta/(1+wbar_0)) |wbar_1|^2), and the
  // second W^-1 reuses the first one's dot.  POC: k0 = ds / lambda by the
  // reciprocal kept in IL.  In: DS, DZ.  Out: K0, K2, T2, DLT (per cone).
  __device__ __forceinline__ void solve_head() { SOCP_SLOT_DISPATCH(solve_head_k); }
  template <int SL0, int SL1>
  __device__ __forceinline__ void solve_head_k() {
    MARK_BEGIN("solve_head");
    if (SOCP_KO & 8192) return;
    LANE_IDS();
    double v[2][3], x[2], x0[2], dz[2], dz0[2], lam[2], wb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane);
      x[s] = LDS(DS + i);
      x0[s] = LDS(DS + eo[s]);
      dz[s] = LDS(DZ + i);
      dz0[s] = LDS(DZ + eo[s]);
      lam[s] = LDS(LAM + i);
      wb[s] = LDS(WB + i);
      const bool tail = tailm(SOCP_SK(s), kd[s]);
      v[s][0] = tail ? lam[s] * x[s] : 0.0;
      v[s][1] = tail ? wb[s] * x[s] : 0.0;
      v[s][2] = tail ? wb[s] * dz[s] : 0.0;
    }
    // the scaling's per-cone constants and the element coefficients are read
    // before the reduction: their LDS latency hides under its DPP chain
    double cst[2][12];
    auto read_cst = [&]() {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane), c = ci[s];
      cst[s][0] = ccv(CC_L0, c);
      cst[s][1] = ccv(CC_IAA, c);
      cst[s][2] = ccv(CC_IL0, c);
      cst[s][3] = ccv(CC_IL0AA, c);
      cst[s][4] = ccv(CC_MU, c);
      cst[s][5] = ccv(CC_IMU, c);
      cst[s][6] = ccv(CC_WB0, c);
      cst[s][7] = ccv(CC_I1, c);
      cst[s][8] = ccv(CC_W2, c);
      cst[s][9] = ccv(CC_WL, c);
      cst[s][10] = LDS(IL + i);
      cst[s][11] = LDS(CA + i);
    }
    };
    if constexpr (HOIST_CST) read_cst();
    cone_reduce<3, 0, may_soc(SL0) ? 7u : 0u, may_soc(SL1) ? 7u : 0u>(v);
    STAMP_X(8);
    MARK_BEGIN("head_post");
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
      const int i = el(s, lane), c = ci[s];
      const double t = v[s][0], u = v[s][1], w = v[s][2];
#define CST(j, expr) (HOIST_CST ? cst[s][j] : (expr))
      const double l0 = CST(0, ccv(CC_L0, c)), iaa = CST(1, ccv(CC_IAA, c)), il0 = CST(2, ccv(CC_IL0, c)),
                   il0aa = CST(3, ccv(CC_IL0AA, c));
      const double mu = CST(4, ccv(CC_MU, c)), imu = CST(5, ccv(CC_IMU, c)), wb0 = CST(6, ccv(CC_WB0, c)),
                   i1 = CST(7, ccv(CC_I1, c));
      const double w2 = CST(8, ccv(CC_W2, c)), wl = CST(9, ccv(CC_WL, c));
      // iprod! (vectors.jl:105-125)
      const double k00 = fma(x0[s], l0, -t) * iaa;
      const double k0t = fma(lam[s] * t, il0aa, fma(x[s], il0, -(x0[s] * lam[s] * iaa)));
      const double dlt = fma(wl * t, il0aa, fma(u, il0, -(x0[s] * wl * iaa)));  // wbar_1'k0_1
      // scale! (scalings.jl:159-165)
      const double kd1 = fma(dlt, i1, k00);  // k0_0 + delta/(1+wbar_0)
      const double k10 = mu * fma(wb0, k00, dlt);
      const double k1t = mu * fma(kd1, wb[s], k0t);
      const double k20 = dz0[s] - k10;
      const double a1 = fma(-mu, fma(kd1, w2, dlt), w);  // wbar_1'k2_1 = w - mu (delta + kd1 |wbar_1|^2)
      // iscale! twice (scalings.jl:167-173)
      const double cy = fma(a1, i1, -k20);
      const double y0 = imu * fma(wb0, k20, -a1);
      const double a2 = imu * fma(cy, w2, a1);
      // POC: elementwise, with 1/lambda and 1/w = CA
      const double k0p = x[s] * CST(10, LDS(IL + i));
      const double k2p = fma(-wb[s], k0p, dz[s]);
      const double ca = CST(11, LDS(CA + i));
      const bool poc = pocs(SOCP_SK(s), kd[s]), hd = headm(SOCP_SK(s), kd[s]);
      const double k0 = poc ? k0p : (hd ? k00 : k0t);
      const double k2 = poc ? k2p : dz[s] - (hd ? k10 : k1t);
      const double yt = imu * fma(cy, wb[s], k2);
      const double zs = hd ? imu * fma(wb0, y0, -a2) : imu * fma(fma(a2, i1, -y0), wb[s], yt);
      if (kd[s] != 3) {
        LDS(K0 + i) = k0;
        LDS(K2 + i) = k2;
        LDS(T2 + i) = poc ? ca * (ca * k2p) : zs;
      }
      if (hd) LDS(cc(CC_DLT, c)) = dlt;
    }
    SYNC();
  }

  // Second half of solve_kkt (densesolver.jl:83-88): cz = iWiW k1 = W^-1 (W^-1 k1),
  // k0 -= W cz (W cz = W^-1 k1 = y), cs = W k0.  wbar_1'(k0 - y)_1 is DLT
  // (solve_head's) minus wbar_1'y_1, so cs needs no reduction of its own.
  // With do_step, compute_step (mats.jl:30-40) of the direction
  // (solver.jl:128-130, 143-145) follows: kt3 = W rz and kt2 = W^-1 rs are y
  // and k0 - y exactly; and the dot kt2'kt3 (rho's, solver.jl:132) and each
  // cone's kt2'kt3 (the head of kt2 o kt3, :136) come out of the step's
  // reduction.  In: K1 (= G cx - k2), K0.  Out: RZ, RS, and with do_step
  // T1 = kt3, K0 = kt2, KK (per cone), O_TOTC[1][0] = kt2'kt3, the step
  // length (dom: DomainError).
  __device__ __forceinline__ double solve_tail(bool do_step, bool dm_aa, int& dom) {
    SOCP_SLOT_DISPATCH(solve_tail_k, do_step, dm_aa, dom);
  }
  template <int SL0, int SL1>
  __device__ __forceinline__ double solve_tail_k(bool do_step, bool dm_aa, int& dom) {
    MARK_BEGIN("solve_tail");
    if (SOCP_KO & 16384) {
      dom = 0;
      return 1.0;
    }
    LANE_IDS();
    double v[2][3], k1[2], k10[2], k0[2], k00[2], wb[2], lam[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane);
      k1[s] = LDS(K1 + i);
      k10[s] = LDS(K1 + eo[s]);
      k0[s] = LDS(K0 + i);
      k00[s] = LDS(K0 + eo[s]);
      wb[s] = LDS(WB + i);
      lam[s] = LDS(LAM + i);
      const bool tail = tailm(SOCP_SK(s), kd[s]);
      v[s][0] = tail ? wb[s] * k1[s] : 0.0;
      v[s][1] = tail ? lam[s] * k1[s] : 0.0;
      v[s][2] = tail ? lam[s] * k0[s] : 0.0;
    }
    double cst[2][12];  // read before the reduction (as in solve_head)
    auto read_cst = [&]() {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane), c = ci[s];
      cst[s][0] = ccv(CC_MU, c);
      cst[s][1] = ccv(CC_IMU, c);
      cst[s][2] = ccv(CC_WB0, c);
      cst[s][3] = ccv(CC_I1, c);
      cst[s][4] = ccv(CC_W2, c);
      cst[s][5] = ccv(CC_WL, c);
      cst[s][6] = LDS(CA + i);
      cst[s][7] = ccv(CC_DLT, c);
      cst[s][8] = ccv(CC_SA, c);
      cst[s][9] = ccv(CC_L0, c);
      cst[s][10] = ccv(CC_SAL, c);
      cst[s][11] = LDS(IL + i);
    }
    };
    if constexpr (HOIST_CST) read_cst();
    cone_reduce<3, 0, may_soc(SL0) ? 7u : 0u, may_soc(SL1) ? 7u : 0u>(v);
    STAMP_X(9);
    MARK_BEGIN("tail_post1");
    double y[2], y0v[2], kn[2], kn0[2], ly[2], lkn[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
      const int i = el(s, lane), c = ci[s];
      const double a1 = v[s][0];
      const double mu = CST(0, ccv(CC_MU, c)), imu = CST(1, ccv(CC_IMU, c)), wb0 = CST(2, ccv(CC_WB0, c)),
                   i1 = CST(3, ccv(CC_I1, c));
      const double w2 = CST(4, ccv(CC_W2, c)), wl = CST(5, ccv(CC_WL, c));
      const double ca = CST(6, LDS(CA + i));
      const bool poc = pocs(SOCP_SK(s), kd[s]), hd = headm(SOCP_SK(s), kd[s]);
      const double cy = fma(a1, i1, -k10[s]);
      const double y0 = imu * fma(wb0, k10[s], -a1);
      const double a2 = imu * fma(cy, w2, a1);  // wbar_1'y_1
      y[s] = poc ? ca * k1[s] : (hd ? y0 : imu * fma(cy, wb[s], k1[s]));
      const double zs = hd ? imu * fma(wb0, y0, -a2) : imu * fma(fma(a2, i1, -y0), wb[s], y[s]);
      y0v[s] = y0;
      kn[s] = k0[s] - y[s];
      kn0[s] = k00[s] - y0;
      const double del = CST(7, ccv(CC_DLT, c)) - a2;  // wbar_1'kn_1
      const double cs = poc ? wb[s] * kn[s]
                            : (hd ? mu * fma(wb0, kn0[s], del) : mu * fma(fma(del, i1, kn0[s]), wb[s], kn[s]));
      ly[s] = imu * fma(cy, wl, v[s][1]);  // lambda_1'y_1
      lkn[s] = v[s][2] - ly[s];           // lambda_1'kn_1
      if (kd[s] != 3) {
        LDS(RZ + i) = poc ? ca * y[s] : zs;
        LDS(RS + i) = cs;
      }
    }
    if (!do_step) {
      SYNC();
      return 0.0;
    }
    // scmax (mats.jl:42-86) of kt3 = y and kt2 = kn, and kt2'kt3
    double w[2][5], r1y[2], r1k[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
      const int i = el(s, lane), c = ci[s];
      if (kd[s] != 3) {
        LDS(T1 + i) = y[s];
        LDS(K0 + i) = kn[s];
      }
      const bool tail = tailm(SOCP_SK(s), kd[s]), poc = pocm(SOCP_SK(s), kd[s]), real = kd[s] != 3;
      const double sa = CST(8, ccv(CC_SA, c)), l0 = CST(9, ccv(CC_L0, c)), sal = CST(10, ccv(CC_SAL, c));
      r1y[s] = fma(sa * l0, y0v[s], -(sa * ly[s]));
      r1k[s] = fma(sa * l0, kn0[s], -(sa * lkn[s]));
      const double cyy = (r1y[s] + y0v[s]) * sal, cyk = (r1k[s] + kn0[s]) * sal;
      const double qy = sa * fma(-(cyy * sa), lam[s], y[s]), qk = sa * fma(-(cyk * sa), lam[s], kn[s]);
      const double il = CST(11, LDS(IL + i));
      w[s][0] = tail ? qy * qy : 0.0;
      w[s][1] = tail ? qk * qk : 0.0;
      w[s][2] = poc ? -y[s] * il : -INFINITY;
      w[s][3] = poc ? -kn[s] * il : -INFINITY;
      w[s][4] = real ? y[s] * kn[s] : 0.0;
    }
    // SOC: |q_y|^2, |q_k|^2; POC: the two maxima; both: the cone's kt2'kt3
    cone_reduce<5, 0xC, may_soc(SL0) ? (may_poc(SL0) ? 0x1Fu : 0x13u) : 0x1Cu,
                may_soc(SL1) ? (may_poc(SL1) ? 0x1Fu : 0x13u) : 0x1Cu>(w);
    STAMP_X(10);
    MARK_BEGIN("tail_post2");
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
      const int c = ci[s];
      if (64 * s >= k || kd[s] == 3 || el(s, lane) != eo[s]) continue;
      const double sa = CST(8, ccv(CC_SA, c));
#undef CST
      const double vy = fma(-sa, r1y[s], sqrt_nr(w[s][0]));
      const double vk = fma(-sa, r1k[s], sqrt_nr(w[s][1]));
      LDS(O_TOTC + c) = pocs(SOCP_SK(s), kd[s]) ? fmax(w[s][2], w[s][3]) : fmax(vy, vk);
      LDS(cc(CC_KK, c)) = w[s][4];
    }
    SYNC();
    dom = dm_aa ? 1 : 0;
    const double t = fmax(cone_max(0), 0.0);
    return !(t > 1.0) ? 1.0 : (t == INFINITY ? 0.0 : recip(t));  // min(1, 1/t)
  }

  // rho, sigma, mu (solver.jl:132-134) and the corrector right-hand side
  // (:136-140): kt1 = kt2 o kt3, ds += sigma mu e - kt1, dx, dy, dz *= 1 - sigma.
  // kt2'kt3 and the SOC heads of kt2 o kt3 come from solve_tail's reduction.
  // In: K0 (kt2), T1 (kt3), KK, DS, DZ, RD, RP.
  __device__ __forceinline__ void affine_post(double tstep, double ll) { SOCP_SLOT_DISPATCH(affine_post_k, tstep, ll); }
  template <int SL0, int SL1>
  __device__ __forceinline__ void affine_post_k(double tstep, double ll) {
    MARK_BEGIN("affine_post");
    if (SOCP_KO & 32768) return;
    LANE_IDS();
    double kk = 0.0, kv[NCS];  // one round trip
#pragma unroll
    for (int c = 0; c < NCS; ++c) kv[c] = LDS(cc(CC_KK, c));
#pragma unroll
    for (int c = 0; c < NCS; ++c) kk = c < nc ? kk + kv[c] : kk;
    const double t = tstep;
    const double rho = 1.0 - t - t * t * kk / ll;
    const double cr = isnan(rho) ? rho : (rho < 0.0 ? 0.0 : (rho > 1.0 ? 1.0 : rho));
    const double sig = ipow(cr, a.sigma_exp);  // max(0,min(1,rho))^3 (solver.jl:133)
    const double mu_ipm = ll / a.deg;
    const double scf = 1.0 - sig;
    const double smu = sig * mu_ipm;
    if constexpr (HOIST_CST) {
      // every read first (one round trip; n, m <= 64 here), then the updates
      double a2[2], a3[2], a20[2], a30[2], kkc[2], dsv[2], dzv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int i = el(s, lane);
        a2[s] = LDS(K0 + i);
        a3[s] = LDS(T1 + i);
        a20[s] = LDS(K0 + eo[s]);
        a30[s] = LDS(T1 + eo[s]);
        kkc[s] = LDS(cc(CC_KK, ci[s]));
        dsv[s] = LDS(DS + i);
        dzv[s] = LDS(DZ + i);
      }
      const double rdv = LDS(RD + lane), rpv = LDS(RP + (lane < MPAD ? lane : 0));
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
        const int i = el(s, lane);
        if (kd[s] == 3) continue;
        const double kt1 = pocs(SOCP_SK(s), kd[s]) ? a2[s] * a3[s]
                                                   : (headm(SOCP_SK(s), kd[s]) ? kkc[s] : fma(a20[s], a3[s], a30[s] * a2[s]));
        const double e = tailm(SOCP_SK(s), kd[s]) ? 0.0 : 1.0;
        LDS(DS + i) = dsv[s] + (smu * e - kt1);  // (smu e is exact)
        LDS(DZ + i) = dzv[s] * scf;
      }
      if (lane < n) LDS(RD + lane) = rdv * scf;
      if (lane < m) LDS(RP + lane) = rpv * scf;
      SYNC();
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma clang fp contract(off)
        const int i = el(s, lane);
        if (kd[s] == 3) continue;
        const double a2 = LDS(K0 + i), a3 = LDS(T1 + i);
        const double a20 = LDS(K0 + eo[s]), a30 = LDS(T1 + eo[s]);
        const double kt1 = kd[s] == 0 ? a2 * a3 : (kd[s] == 1 ? LDS(cc(CC_KK, ci[s])) : fma(a20, a3, a30 * a2));
        const double e = kd[s] == 2 ? 0.0 : 1.0;
        LDS(DS + i) = LDS(DS + i) + (smu * e - kt1);
        LDS(DZ + i) = LDS(DZ + i) * scf;
      }
      for (int j = lane; j < n; j += 64) LDS(RD + j) = LDS(RD + j) * scf;
      for (int i = lane; i < m; i += 64) LDS(RP + i) = LDS(RP + i) * scf;
      SYNC();
    }
  }

  // max_step(-iz), max_step(iz) (mats.jl:1-28) for the initial shift (solver.jl:88-101)
  __device__ __forceinline__ void maxstep_op(int xv, double& alphp, double& alphd) {
    SOCP_SLOT_DISPATCH(maxstep_op_k, xv, alphp, alphd);
  }
  template <int SL0, int SL1>
  __device__ __forceinline__ void maxstep_op_k(int xv, double& alphp, double& alphd) {
    MARK_BEGIN("maxstep_op");
    LANE_IDS();
    double v[2][3], x[2], x0[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = el(s, lane);
      x[s] = LDS(xv + i);
      x0[s] = LDS(xv + eo[s]);
      v[s][0] = tailm(SOCP_SK(s), kd[s]) ? x[s] * x[s] : 0.0;
      v[s][1] = pocm(SOCP_SK(s), kd[s]) ? x[s] : -INFINITY;
      v[s][2] = pocm(SOCP_SK(s), kd[s]) ? -x[s] : -INFINITY;
    }
    cone_reduce<3, 0x6, may_soc(SL0) ? (may_poc(SL0) ? 7u : 1u) : 6u, may_soc(SL1) ? (may_poc(SL1) ? 7u : 1u) : 6u>(v);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (64 * s >= k || kd[s] == 3 || el(s, lane) != eo[s]) continue;
      const double nr = sqrt_nr(v[s][0]);
      const bool poc = pocs(SOCP_SK(s), kd[s]);
      LDS(O_TOTC + ci[s]) = poc ? v[s][1] : nr + x0[s];
      LDS(O_TOTC + NCS + ci[s]) = poc ? v[s][2] : nr - x0[s];
    }
    SYNC();
    alphp = cone_max(0);
    alphd = cone_max(NCS);
  }

  // U[c,:] = (sum_{i in cone c} w_i G[i,:]) / (1+wb0), w_head = -(1+wb0), w_tail = wb_i
  // The row steps a cone covers are taken four at a time, their four weight reads
  // issued together (one LDS round trip per four row steps), the weights
  // masked branch-free.
  __device__ __forceinline__ void compute_U() {
    MARK_BEGIN("compute_U");
    LANE_IDS();
    // HOIST_CST shapes: every row's weight read once, in one round trip
    double wall[HOIST_CST ? NP : 1];
    if constexpr (HOIST_CST) {
#pragma unroll
      for (int pp = 0; pp < NP; ++pp) wall[pp] = LDS(WB + 4 * pp + g);
    }
    // every SOC cone's offset, dim, head weight and 1/(1+wb0) on its cone lane
    // (lane c < nc), read in one round trip with the row weights; the loop
    // takes them by readlane (no scalar-memory or LDS wait per cone)
    bool socl = false;
    int ol = 0, dl = 0;
    double hwl = 0.0, invl = 0.0;
    if (lane < nc) {
      socl = HOIST_CST ? lc_soc : (int)LDS(O_CKIND + lane) == SOC_K;
      ol = HOIST_CST ? lc_off : (int)LDS(O_COFF + lane);
      dl = HOIST_CST ? lc_dim : (int)LDS(O_CDIM + lane);
      hwl = -(1.0 + LDS(WB + ol));
      invl = LDS(cc(CC_I1, lane));
    }
    for (uint64_t mk = __ballot(socl); mk; mk &= mk - 1) {
      const int c = __builtin_ctzll(mk);
      const int o = __builtin_amdgcn_readlane(ol, c), d = __builtin_amdgcn_readlane(dl, c);
      const double hw = readlane_d(hwl, c);  // the head row's weight
      const double inv = readlane_d(invl, c);
      const int p0 = o >> 2, p1 = (o + d + 3) >> 2;  // row steps [p0, p1) meet the cone
      double acc[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
      for (int pb = 0; pb < NP; pb += 4) {
        if (pb + 4 <= p0 || pb >= p1) continue;  // wave-uniform
        constexpr int U4 = 4;
        double w[U4];
#pragma unroll
        for (int u = 0; u < U4; ++u) {
          const int row = 4 * (pb + u) + g;  // < KP: in the LDS k-vector
          if constexpr (HOIST_CST)
            w[u] = (pb + u < NP) ? wall[pb + u < NP ? pb + u : 0] : 0.0;
          else
            w[u] = (pb + u < NP) ? LDS(WB + row) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U4; ++u) {
          const int row = 4 * (pb + u) + g;
          const bool in = row >= o && row < o + d;
          const double wu = in ? (row == o ? hw : w[u]) : 0.0;
          if (pb + u < NP) {
            {
              double gr[NQ];
              a_get_row<NQ>(G[pb + u < NP ? pb + u : 0], gr);
#pragma unroll
              for (int q = 0; q < NQ; ++q) acc[q] = fma(wu, gr[q], acc[q]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = rows_sum(acc[q]);
      if (g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) LDS(O_U + c * NPAD + 16 * q + cl) = acc[q] * inv;
      }
    }
    SYNC();
  }

  // ----------------------------------------------------- H = X'X (+A'A)
  // row step pp of X = W^-1 G: X[i,:] = CA_i G[i,:] + CBV_i U[cone(i),:],
  // in two halves, for a two-deep pipeline: the row coefficients (and the
  // cone id that addresses U) first, the U row and the products a step later
  struct XCoef {
    double ca, cb;
    int ub;  // LDS index of the cone's U row + cl
  };
  // (UBT shapes: the lane ids of form_H, computed once for the whole product,
  // and the U row from the launch's table)
  __device__ __forceinline__ XCoef xcoef(int pp, int g_, int cl_) {
    XCoef c;
    if constexpr (SH::UBT) {
      const int row = 4 * pp + g_;
      c.ca = LDS(CA + row);
      c.cb = LDS(CBV + row);
      if constexpr (EX)
        c.ub = O_U + (pp / (4 * EXF.al_rows)) * NPAD + cl_;  // a row step lies in one cone
      else
        c.ub = ubt(row) + cl_;  // O_U + cone(row) * NPAD
    } else {
      LANE_IDS();
      const int row = 4 * pp + g;
      c.ca = LDS(CA + row);
      c.cb = LDS(CBV + row);
      c.ub = O_U + (((int)LDS(O_RC + row)) >> 2) * NPAD + cl;
    }
    return c;
  }
  __device__ __forceinline__ void xrow(int pp, const XCoef& c, double (&X)[NQ]) {
    double u[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) u[q] = LDS(c.ub + 16 * q);
    {
      double gr[NQ];
      a_get_row<NQ>(G[pp], gr);
#pragma unroll
      for (int q = 0; q < NQ; ++q) X[q] = fma(c.ca, gr[q], c.cb * u[q]);
    }
  }
  // ---------------------------------------------------------------- QP
  // This problem's P (set by run()) and the byte range form_H may read of it:
  // n n 8, or 0 for MP_SINGTEST's G'G, whose loads then all return 0.
  const double* qp_P = nullptr;
  int qp_hrange = 0;
  // raw buffer over P: an element outside n x n takes an offset past the range
  // and reads 0 (load_problem's G descriptor does the same)
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t qp_rsrc(int range) const {
    const uint64_t pu = (uint64_t)qp_P;
    const uint64_t base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pu >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pu);
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, __builtin_amdgcn_readfirstlane(range), 0x00020000);
  }
  // T += P, tile by tile in the tiles' own layout: lane (g, cl), register r of
  // block (bi, bj) holds row 16 bi + g + 4r, column 16 bj + cl.  P is symmetric,
  // so the element is read as P(column, row): 16 lanes read 128 contiguous bytes.
  __device__ __forceinline__ void add_P() {
    LANE_IDS();
    const __amdgpu_buffer_rsrc_t rs = qp_rsrc(qp_hrange);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
      for (int tj = 0; tj <= ti; ++tj) {
        const int bi = tj, bj = ti;  // the upper-block form
        const int Cc = 16 * bj + cl;
        double pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int R = 16 * bi + g + 4 * r;
          const int off = (R < n && Cc < n) ? (R * n + Cc) * 8 : 0x40000000;
          pv[r] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) T[tri(ti, tj)][r] += pv[r];
        // two tiles' loads per round trip: the registers the loads hold stay bounded (<4,24,1> is at the cap)
        if (tri(ti, tj) % 2 == 1) SCHED_FENCE();
      }
  }
  // acc[q] (all lanes) = (P v)[16q+cl], v an n-vector in LDS: rows split over
  // the 4 lane groups as in At_mv; row i of P is read as its column i
  __device__ __forceinline__ void P_mv(int v, double (&acc)[NQ]) {
    LANE_IDS();
    const __amdgpu_buffer_rsrc_t rs = qp_rsrc(n * n * (int)sizeof(double));
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    // PB row steps (of 4 NQ), up to 16 loads, per round trip (At_mv's batching)
    constexpr int PB = NQ == 2 ? 8 : 4;
    static_assert((4 * NQ) % PB == 0, "whole batches");
#pragma unroll
    for (int s0 = 0; s0 < NQ * 4; s0 += PB) {
      double vi[PB], pv[PB][NQ];
#pragma unroll
      for (int s = 0; s < PB; ++s) {
        const int i = g + 4 * (s0 + s);
        vi[s] = i < n ? LDS(v + i) : 0.0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int j = 16 * q + cl;
          const int off = (i < n && j < n) ? (i * n + j) * 8 : 0x40000000;
          pv[s][q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
        }
      }
      SCHED_FENCE();
#pragma unroll
      for (int s = 0; s < PB; ++s)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = fma(pv[s][q], vi[s], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = rows_sum(acc[q]);
  }

  static constexpr bool diag_tile(int t) {
    for (int i = 0; i < NQ; ++i)
      if (tri(i, i) == t) return true;
    return false;
  }
  // rows_in_T (FAC_IDENT_H): T already holds the row steps' sum X'X, only the
  // rest is added
  __device__ __forceinline__ void form_H(bool addAA, bool rows_in_T = false) {
    MARK_BEGIN("form_H");
    LANE_IDS();
    if (SOCP_KO & 65536) {  // H = I
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[t][r] = (diag_tile(t) && g + 4 * r == cl) ? 1.0 : 0.0;
      return;
    }
    if (!rows_in_T) {
#pragma unroll
    for (int t = 0; t < NT; ++t) T[t] = (d4){0.0, 0.0, 0.0, 0.0};
    // two-deep pipeline: row coefficients two steps ahead, U rows one step ahead
    constexpr int SYRK_V = 8;  // VALU instructions scheduled behind each of the later MFMAs
    double Xc[NQ];
    XCoef c1;
    {
      const XCoef c0 = xcoef(0, g, cl);
      if (NP > 1) c1 = xcoef(1 < NP ? 1 : 0, g, cl);
      xrow(0, c0, Xc);
    }
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      XCoef c2 = c1;
      if (pp + 2 < NP) c2 = xcoef(pp + 2 < NP ? pp + 2 : 0, g, cl);
      double Xn[NQ];
      if (pp + 1 < NP) xrow(pp + 1 < NP ? pp + 1 : 0, c1, Xn);
#pragma unroll
      for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) T[tri(ti, tj)] = mfma(Xc[tj], Xc[ti], T[tri(ti, tj)]);  // block (tj, ti)
      if (pp + 1 < NP) {
        // the step's LDS reads behind the first MFMAs, its VALU after them
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int r = 2; r < NT; ++r) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, SYRK_V, 0);
        }
      }
      SCHED_FENCE();
      c1 = c2;
#pragma unroll
      for (int q = 0; q < NQ; ++q) Xc[q] = Xn[q];
    }
    } else {
      // (the tiles pass through a statement of this branch, so that whatever
      // moves them to the row loop's registers sits here, once per problem,
      // and not ahead of the branch on every factorisation)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(T[t][r]));
    }
    if (addAA) {
#pragma unroll
      for (int tm = 0; tm < MQ; ++tm)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int rowA = 16 * tm + g + 4 * s;
          double Aq[NQ];
#pragma unroll
          for (int q = 0; q < NQ; ++q) Aq[q] = LDS(O_A + rowA * LDA + 16 * q + cl);
#pragma unroll
          for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj) T[tri(ti, tj)] = mfma(Aq[tj], Aq[ti], T[tri(ti, tj)]);
        }
    }
    if constexpr (QP) add_P();
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = 16 * ti + g + 4 * r, Cc = 16 * ti + cl;
        if (R == Cc && R >= n) T[tri(ti, ti)][r] = 1.0;
      }
  }

  // ------------------------------------------------------- tile algebra
  // C/D-tile algebra: lane (g, cl) holds X[g+4r][cl] in register r, so
  // register s of a tile is the k-step-s operand of mfma_f64_16x16x4, and
  // sum_s mfma(U[s], V[s]) = U'V for any two tiles U, V.

  // sum_s mfma(U[s], V[s], C) with the NEG modifiers of gfx950 f64 MFMA
  // (blgp bit 0 negates A, bit 2 negates C)
  template <int NEG>
  __device__ __forceinline__ static d4 mm(const d4& U, const d4& V, d4 C) {
#pragma unroll
    for (int s = 0; s < 4; ++s) C = __builtin_amdgcn_mfma_f64_16x16x4f64(U[s], V[s], C, 0, 0, NEG);
    return C;
  }

  // ------------------------------------ H = L L' by 16x16 tiles (CHOL shapes)
  // densesolver.jl:47 cholesky!(Hermitian(H)), right-looking by tile panels.
  // The explicit Li of :48 is never formed: ALi = A Li enters as Z = L^-1 A'
  // (S = A Li A' = Z'Z, :49-50) and Li v as two triangular solves.  Storage:
  // the SYRK leaves block (i, j), i <= j, of H in T[tri(j, i)] (upper tiles),
  // so the panel row U_Pi needs no transpose; after panel P, T[tri(P, P)]
  // holds W_P = L_PP^-1 (factor_tile) and T[tri(i, P)] = L_iP' (i > P).
  // Panel P: Y_i = W_P U_Pi = L_iP' (MFMA), U_ij -= Y_i'Y_j (P < i <= j).
  // Look-ahead: Y_{P+1} and U_{P+1,P+1} first, then the next pivot tile is
  // factored with the rest of the panel's MFMA work -- and the panel's tile
  // row of Z -- dealt out between its row blocks.  Every pivot is a Cholesky
  // pivot of H (potrf's test).
  struct CholOp {
    int kind, i, j;  // 0: Y_i = W_P U_Pi, 1: U_ij -= Y_i'Y_j, 2: the Z row of panel P, -1: none
  };
  template <int P>
  static constexpr CholOp chol_op(int idx) {
    int cnt = 0;
    for (int i = P + 2; i < NQ; ++i)
      if (cnt++ == idx) return CholOp{0, i, 0};
    for (int j = P + 1; j < NQ; ++j)  // column-major: U_{P+1,P+2} and U_{P+2,P+2} (the next panel's) first
      for (int i = P + 1; i <= j; ++i) {
        if (i == P + 1 && j == P + 1) continue;
        if (cnt++ == idx) return CholOp{1, i, j};
      }
    if (cnt++ == idx) return CholOp{2, P, 0};
    return CholOp{-1, 0, 0};
  }
  template <int P>
  static constexpr int chol_op_count() {
    int c = 0;
    while (chol_op<P>(c).kind >= 0) ++c;
    return c;
  }
  // Z_P = W_P (A'_P - sum_{Q<P} L_PQ Z_Q) (left-looking: one accumulator tile),
  // S += Z_P'Z_P (Sv[0]); Z' row-major in LDS at O_AL (where the explicit-inverse
  // kernels keep A Li): Z'[c][j] = LDS(O_AL + c*LDA + j).
  template <int P>
  __device__ __forceinline__ void z_row(const d4& WT) {
    LANE_IDS();
    SYNC();
    d4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = LDS(O_A + cl * LDA + 16 * P + g + 4 * r);  // A'[16P+g+4r][cl]
#pragma unroll
    for (int Q = 0; Q < P; ++Q) {
      d4 Zq;
#pragma unroll
      for (int r = 0; r < 4; ++r) Zq[r] = LDS(O_AL + cl * LDA + 16 * Q + g + 4 * r);
      acc = mm<1>(T[tri(P, Q)], Zq, acc);  // -= L_PQ Z_Q
    }
    const d4 Z = mm<0>(WT, acc, (d4){0.0, 0.0, 0.0, 0.0});
    Sv[0] = mm<0>(Z, Z, Sv[0]);
#pragma unroll
    for (int r = 0; r < 4; ++r) LDS(O_AL + cl * LDA + 16 * P + g + 4 * r) = Z[r];
  }
  template <int P, int OP>
  __device__ __forceinline__ void chol_op_run(const d4& WT) {
    constexpr CholOp o = chol_op<P>(OP);
    if constexpr (o.kind == 0) {
      T[tri(o.i, P)] = mm<0>(WT, T[tri(o.i, P)], (d4){0.0, 0.0, 0.0, 0.0});
    } else if constexpr (o.kind == 1) {
      T[tri(o.j, o.i)] = mm<1>(T[tri(o.i, P)], T[tri(o.j, P)], T[tri(o.j, o.i)]);
    } else if constexpr (o.kind == 2) {
      z_row<P>(WT);
    }
  }
  template <int P, int LO, int HI>
  __device__ __forceinline__ void chol_ops(const d4& WT) {
    if constexpr (LO < HI) {
      chol_op_run<P, LO>(WT);
      chol_ops<P, LO + 1, HI>(WT);
    }
  }
  template <int P>
  struct CholHook {
    Small& s;
    const d4& WT;
    template <int B>
    __device__ __forceinline__ void run() const {
      constexpr int N = chol_op_count<P>();
      s.template chol_ops<P, (N * B) / 4, (N * (B + 1)) / 4>(WT);
    }
  };
  template <int P>
  __device__ __forceinline__ void chol_panel(const d4& W, bool& ok) {
    if constexpr (P < NQ) {
      MARK_BEGIN("chol_panel");
      const d4 WT = transpose(W);
      if constexpr (P + 1 < NQ) {
        T[tri(P + 1, P)] = mm<0>(WT, T[tri(P + 1, P)], (d4){0.0, 0.0, 0.0, 0.0});
        T[tri(P + 1, P + 1)] = mm<1>(T[tri(P + 1, P)], T[tri(P + 1, P)], T[tri(P + 1, P + 1)]);
        d4 Wn;
        factor_tile<TILE_INPL, TILE_LANES>(T[tri(P + 1, P + 1)], Wn, ok, CholHook<P>{*this, WT});
        T[tri(P, P)] = W;
        chol_panel<P + 1>(Wn, ok);
      } else {
        z_row<P>(WT);
        T[tri(P, P)] = W;
      }
    }
  }
  __device__ __forceinline__ bool chol() {
    if (SOCP_KO & 131072) {
      LANE_IDS();
#pragma unroll
      for (int r = 0; r < 4; ++r) Sv[0][r] = (g + 4 * r == cl) ? 1.0 : 0.0;
      return true;
    }
    Sv[0] = (d4){0.0, 0.0, 0.0, 0.0};
    bool ok = true;
    d4 W;
    factor_tile<TILE_INPL, TILE_LANES>(T[tri(0, 0)], W, ok);
    chol_panel<0>(W, ok);
    SYNC();
    return ok;
  }

  // ---------------- the explicit inverse from the Cholesky factor (chol_inv)
  // densesolver.jl:47-48: Li = H^-1 from cholesky!(H), the reference's
  // ldiv!(Li, fact, I) -- H = L L', then Li = L^-T L^-1 -- on 16x16 tiles:
  // (1) H = L L' right-looking by tile panels as chol() does it (its look-ahead:
  //     the next pivot tile factored with the panel's other MFMA work dealt out
  //     between its row blocks), leaving M[tri(P, P)] = W_P = L_PP^-1 and
  //     M[tri(i, P)] = L_iP' (i > P); every pivot is potrf's (status 2 / 3);
  // (2) Y = L^-1 in place, row by row: Y_PP = W_P,
  //     Y_ab = -W_a sum_{b <= q < a} L_aq Y_qb (a > b);
  // (3) Li = Y'Y in place, row by row: Li_ab = sum_{q >= a} Y_qa' Y_qb (a >= b),
  //     symmetric by construction.
  // In: M in the upper-block form (M[tri(j, i)] = block (i, j), i <= j, the
  // SYRK's output); out: the lower tiles of the inverse in the natural
  // C/D layout (M[tri(a, b)] = block (a, b)), as symv and the record read them.
  struct GCholOp {
    int kind, i, j;  // 0: M_iP = W_P M_iP (= L_iP'), 1: M_ij -= L_iP L_jP', -1: none
  };
  template <int Q, int P>
  static constexpr GCholOp gchol_op(int idx) {
    int cnt = 0;
    for (int i = P + 2; i < Q; ++i)
      if (cnt++ == idx) return GCholOp{0, i, 0};
    for (int j = P + 1; j < Q; ++j)
      for (int i = P + 1; i <= j; ++i) {
        if (i == P + 1 && j == P + 1) continue;
        if (cnt++ == idx) return GCholOp{1, i, j};
      }
    return GCholOp{-1, 0, 0};
  }
  template <int Q, int P>
  static constexpr int gchol_op_count() {
    int c = 0;
    while (gchol_op<Q, P>(c).kind >= 0) ++c;
    return c;
  }
  template <int Q, int P, int LO, int HI>
  __device__ __forceinline__ static void gchol_ops(d4 (&M)[Q * (Q + 1) / 2], const d4& WT) {
    if constexpr (LO < HI) {
      constexpr GCholOp o = gchol_op<Q, P>(LO);
      if constexpr (o.kind == 0)
        M[tri(o.i, P)] = mm<0>(WT, M[tri(o.i, P)], (d4){0.0, 0.0, 0.0, 0.0});
      else
        M[tri(o.j, o.i)] = mm<1>(M[tri(o.i, P)], M[tri(o.j, P)], M[tri(o.j, o.i)]);
      gchol_ops<Q, P, LO + 1, HI>(M, WT);
    }
  }
  template <int Q, int P>
  struct GCholHook {
    d4 (&M)[Q * (Q + 1) / 2];
    const d4& WT;
    template <int B>
    __device__ __forceinline__ void run() const {
      constexpr int N = gchol_op_count<Q, P>();
      gchol_ops<Q, P, (N * B) / 4, (N * (B + 1)) / 4>(M, WT);
    }
  };
  template <int Q, int P>
  __device__ __forceinline__ void gchol_panel(d4 (&M)[Q * (Q + 1) / 2], const d4& W, bool& ok) {
    if constexpr (P < Q) {
      MARK_BEGIN("chol_inv_panel");
      if constexpr (P + 1 < Q) {
        const d4 WT = transpose(W);
        M[tri(P + 1, P)] = mm<0>(WT, M[tri(P + 1, P)], (d4){0.0, 0.0, 0.0, 0.0});
        M[tri(P + 1, P + 1)] = mm<1>(M[tri(P + 1, P)], M[tri(P + 1, P)], M[tri(P + 1, P + 1)]);
        d4 Wn;
        factor_tile<TILE_INPL, TILE_LANES>(M[tri(P + 1, P + 1)], Wn, ok, GCholHook<Q, P>{M, WT});
        M[tri(P, P)] = W;
        gchol_panel<Q, P + 1>(M, Wn, ok);
      } else {
        M[tri(P, P)] = W;
      }
    }
  }
  template <int Q>
  __device__ __forceinline__ bool chol_inv(d4 (&M)[Q * (Q + 1) / 2]) {
    MARK_BEGIN("chol_inv");
    const d4 z = (d4){0.0, 0.0, 0.0, 0.0};
    bool ok = true;
    {
      d4 W;
      factor_tile<TILE_INPL, TILE_LANES>(M[tri(0, 0)], W, ok);
      gchol_panel<Q, 0>(M, W, ok);
    }
    // Y = L^-1: row a reads rows q < a of Y (done) and row a of L from column b up
#pragma unroll
    for (int a = 1; a < Q; ++a) {
      const d4 WTa = transpose(M[tri(a, a)]);
#pragma unroll
      for (int b = 0; b < a; ++b) {
        d4 S = mm<0>(M[tri(a, b)], M[tri(b, b)], z);  // L_ab W_b
#pragma unroll
        for (int q = b + 1; q < a; ++q) S = mm<0>(M[tri(a, q)], M[tri(q, b)], S);  // + L_aq Y_qb
        M[tri(a, b)] = mm<1>(WTa, S, z);  // -W_a S
      }
    }
    // Li = Y'Y: tile (a, b) is the last reader of Y_ab (row-major order)
#pragma unroll
    for (int a = 0; a < Q; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        d4 acc = z;
#pragma unroll
        for (int q = a; q < Q; ++q) acc = mm<0>(M[tri(q, a)], M[tri(q, b)], acc);
        M[tri(a, b)] = acc;
      }
    return ok;
  }

  // the transpose buffer, when it lives in dead k-vectors, is zeroed again at
  // the end of a factorisation: their padding rows [k, KP) are never written
  // by the solves and must read as zero (G'T2 reads them against G's zero rows)
  __device__ __forceinline__ void clear_tb() {
    if constexpr (SH::TB_ALIAS) {
      SYNC();
      for (int e = lane; e < 16 * 17; e += 64) LDS(O_TB + e) = 0.0;
      SYNC();
    }
  }
  __device__ __forceinline__ d4 transpose(d4 t) {
    MARK_BEGIN("transpose");
    LANE_IDS();
    SYNC();
#pragma unroll
    for (int r = 0; r < 4; ++r) LDS(O_TB + (g + 4 * r) * 17 + cl) = t[r];
    SYNC();
    d4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = LDS(O_TB + cl * 17 + g + 4 * r);
    return o;
  }

  __device__ __forceinline__ void dump_sym(double* out, bool upper = false) {
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
      for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int R = (upper ? 16 * tj : 16 * ti) + g + 4 * r, Cc = (upper ? 16 * ti : 16 * tj) + cl;
          if (R < n && Cc < n) {
            out[R * n + Cc] = T[tri(ti, tj)][r];
            if (ti != tj) out[Cc * n + R] = T[tri(ti, tj)][r];
          }
        }
  }

  // H (+A'A) = L L'.  CHOL: Z = L^-1 A', S = Z'Z, S^-1.  Otherwise Li = L^-T L^-1;
  // ALi' = Li A' (n x m);  S = A ALi';  S^-1.
  // OV: a kernel with the pipelined load (the only ones that name FAC_IDENT_H)
  template <bool OV = false>
  __device__ __forceinline__ int factor(int kind, bool addAA) {
    const bool identity = kind == FAC_IDENT;
    MARK_BEGIN("factor");
    LANE_IDS();
    STAMP(SP_OTHER);
    if (kind == FAC_SCALED && !(SOCP_KO & 4)) compute_U();
    STAMP(SP_U);
    if constexpr (OV) {
      form_H(addAA, kind == FAC_IDENT_H);
    } else {
      form_H(addAA);
    }
    SYNC();
    STAMP(SP_SYRK);
#ifdef SOCP_DIAG
    // diagnostic dump per problem: H, H^-1 (n x n each), lam, wbar (k each), Li A' (n x m), S (m x m)
    double* dbg = (a.dbg && a.mode == MODE_KKT) ? a.dbg + dbg_p * (int64_t)(2 * n * n + 2 * k + n * m + m * m) : nullptr;
    if (dbg && !CHOL) dump_sym(dbg, true);
#endif
    if constexpr (CHOL) {
      const bool okH = chol();
      STAMP(SP_FACTOR_H);
      if (!okH) {
        clear_tb();
        return ST_CHOL_H;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (g + 4 * r == cl && cl >= m) Sv[0][r] = 1.0;
      // S = L L' on one tile (potrf's pivot test), S^-1 = W'W with W = L^-1:
      // one MFMA tile chain and four MFMAs
      bool okS = true;
      if (!(SOCP_KO & 8)) {
        d4 Ws;
        factor_tile<TILE_INPL, TILE_LANES>(Sv[0], Ws, okS);
        Sv[0] = mm<0>(Ws, Ws, (d4){0.0, 0.0, 0.0, 0.0});
      }
      clear_tb();
      STAMP(SP_SCHUR);
      if (!okS) return ST_CHOL_S;
      return 0;
    }
    const bool okH = chol_inv<NQ>(T);
    STAMP(SP_FACTOR_H);
    if (!okH) {
      clear_tb();
      return ST_CHOL_H;
    }
#ifdef SOCP_DIAG
    if (dbg) {
      dump_sym(dbg + n * n);
      for (int i = lane; i < k; i += 64) {
        dbg[2 * n * n + i] = LDS(LAM + i);
        dbg[2 * n * n + k + i] = LDS(WB + i);
      }
    }
#endif
    // S = A Li A' (densesolver.jl:49-50: ALi = A*Li, S = ALi*A'), one 16-column
    // tile of Li A' at a time: it lives only here, the solves use A (Li n0).
#pragma unroll
    for (int tq = 0; tq < MQ; ++tq) {
      d4 ALc[NQ];
#pragma unroll
      for (int ti = 0; ti < NQ; ++ti) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int tk = 0; tk < NQ; ++tk) {
          d4 Ut;
          if (tk >= ti)
            Ut = T[tri(tk, ti)];
          else
            Ut = transpose(T[tri(ti, tk)]);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = mfma(Ut[s], LDS(O_A + (16 * tq + cl) * LDA + 16 * tk + g + 4 * s), acc);
        }
        ALc[ti] = acc;
      }
#ifdef SOCP_DIAG
      if (dbg) {
        double* dA = dbg + 2 * n * n + 2 * k;
#pragma unroll
        for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int R = 16 * ti + g + 4 * r, Cc = 16 * tq + cl;
            if (R < n && Cc < m) dA[R * m + Cc] = ALc[ti][r];
          }
      }
#endif
#pragma unroll
      for (int tm = tq; tm < MQ; ++tm) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int tk = 0; tk < NQ; ++tk)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double av = LDS(O_A + (16 * tm + cl) * LDA + 16 * tk + g + 4 * s);
            // block (tq, tm) of S, the upper-block form chol_inv reads
            acc = mfma(ALc[tk][s], av, acc);
          }
        Sv[tri(tm, tq)] = acc;
      }
      if constexpr (AL_LDS) {
        // A Li row-major in LDS: lane (g, cl) holds (A Li)[16tq+cl][16ti+g+4r]
#pragma unroll
        for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) LDS(O_AL + (16 * tq + cl) * LDA + 16 * ti + g + 4 * r) = ALc[ti][r];
      }
    }
#pragma unroll
    for (int tm = 0; tm < MQ; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = 16 * tm + g + 4 * r, Cc = 16 * tm + cl;
        if (R == Cc && R >= m) Sv[tri(tm, tm)][r] = 1.0;
      }
#ifdef SOCP_DIAG
    if (dbg) {
      double* dS = dbg + 2 * n * n + 2 * k + n * m;
#pragma unroll
      for (int tm = 0; tm < MQ; ++tm)
#pragma unroll
        for (int tq = 0; tq <= tm; ++tq)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int R = 16 * tq + g + 4 * r, Cc = 16 * tm + cl;
            if (R < m && Cc < m) dS[R * m + Cc] = dS[Cc * m + R] = Sv[tri(tm, tq)][r];
          }
    }
#endif
    SYNC();
    const bool okS = chol_inv<MQ>(Sv);
    clear_tb();  // the factorisations' and A Li's transposes ran in the dead k-vectors (TB_ALIAS)
    STAMP(SP_SCHUR);
    if (!okS) return ST_CHOL_S;
    return 0;
  }

  // out = M*v for a symmetric matrix stored as lower tiles (C/D layout).
  // Lower part: per tile row, reduce over the 16 column lanes; strictly upper
  // part (transposed off-diagonal tiles): reduce over the 4 row groups.
  template <int Q>
  __device__ __forceinline__ void symv(const d4 (&M)[Q * (Q + 1) / 2], int vin, int vout) {
    MARK_BEGIN("symv");
    LANE_IDS();
    double vc[Q], P2[Q];
#pragma unroll
    for (int t = 0; t < Q; ++t) {
      vc[t] = LDS(vin + 16 * t + cl);
      P2[t] = 0.0;
    }
    double P1row[Q];
#pragma unroll
    for (int ti = 0; ti < Q; ++ti) {
      double vr[4], P1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        vr[r] = LDS(vin + 16 * ti + g + 4 * r);
        double acc = 0.0;
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) acc = fma(M[tri(ti, tj)][r], vc[tj], acc);
        P1[r] = acc;
      }
#pragma unroll
      for (int tj = 0; tj < ti; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) P2[tj] = fma(M[tri(ti, tj)][r], vr[r], P2[tj]);
      int base = 0;
      rs16<4, 8>(P1, cl, base);  // one value per lane: row 16ti + g + 4*base
      P1row[ti] = P1[0] + 0.0 * base;
      // stash the row index in base via the lane's own cl bits (see write below)
    }
    if constexpr (Q > 1) {
#pragma unroll
      for (int t = 0; t < Q; ++t) P2[t] = rows_sum(P2[t]);
    }
    SYNC();
    {
      // rs16<4,8>: bit 8 of cl picks entries 2-3, bit 4 picks the odd one; masks
      // 2 and 1 are all-reduce steps, so the lane holds entry (cl>>3&1)*2 + (cl>>2&1)
      const int r = ((cl >> 3) & 1) * 2 + ((cl >> 2) & 1);
#pragma unroll
      for (int ti = 0; ti < Q; ++ti) LDS(vout + 16 * ti + g + 4 * r) = P1row[ti];
    }
    SYNC();
    if constexpr (Q > 1) {  // one tile has no strictly upper part
      if (g == 0) {
#pragma unroll
        for (int t = 0; t < Q; ++t) LDS(vout + 16 * t + cl) += P2[t];
      }
      SYNC();
    }
  }

  // symv<1> with v in column layout in registers (vc = v[cl], every lane); out
  // to LDS as symv's, and in registers in row layout, yr[s] = out[g + 4s]
  __device__ __forceinline__ void symv1_r(const d4& M, double vc, int vout, double (&yr)[4]) {
    MARK_BEGIN("symv");
    LANE_IDS();
    double P1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) P1[r] = fma(M[r], vc, 0.0);
    int base = 0;
    rs16<4, 8>(P1, cl, base);  // row g + 4 (cl >> 2)
    LDS(vout + g + 4 * (cl >> 2)) = P1[0];
    yr[0] = dpp_all<0x150>(P1[0]);
    yr[1] = dpp_all<0x154>(P1[0]);
    yr[2] = dpp_all<0x158>(P1[0]);
    yr[3] = dpp_all<0x15C>(P1[0]);
  }

  // Triangular solves against chol()'s factor (T[tri(P, P)] = W_P = L_PP^-1,
  // T[tri(i, P)] = L_iP').  Tile products alternate between the two vector
  // layouts of a C/D tile, so no LDS round trip sits on the chain: W v
  // (v[cl] in every lane of column cl) gives (W v)[g+4r] after a 16-lane
  // all-reduce; M'u (u[g+4r] in the lanes of row group g) gives (M'u)[cl]
  // after the four-row sum.  The off-diagonal products of earlier tiles are
  // accumulated lane-locally and reduced once per tile.
  __device__ __forceinline__ static void allred16(double (&v)[4]) {
    // reduce-scatter (entry r ends in lanes 4r..4r+3 of the row: rs16's base is
    // cl >> 2), then each entry broadcast from lane 4r by row_newbcast: 9 DPP
    // moves and 6 adds per 64-bit lane value instead of 16 and 16
    LANE_IDS();
    int base = 0;
    rs16<4, 8>(v, cl, base);
    const double t = v[0];
    v[0] = dpp_all<0x150>(t);
    v[1] = dpp_all<0x154>(t);
    v[2] = dpp_all<0x158>(t);
    v[3] = dpp_all<0x15C>(t);
  }
  // out = L^-1 v: t_P = W_P (v_P - sum_{Q<P} L_PQ t_Q).  rc: v in column
  // layout (every lane holds v[16i+cl]); tv: t in row layout (tv[P][r] =
  // t[16P+g+4r] in every lane of row group g), for a product that takes its
  // operand in that layout without the LDS round trip.
  __device__ __forceinline__ void trsv_fwd_r(const double (&rc)[NQ], int vout, double (&tv)[NQ][4]) {
    MARK_BEGIN("trsv_fwd");
    LANE_IDS();
    double pa[NQ];  // lane partials of sum_Q L_iQ t_Q
#pragma unroll
    for (int i = 0; i < NQ; ++i) pa[i] = 0.0;
#pragma unroll
    for (int P = 0; P < NQ; ++P) {
      const double rp = P > 0 ? rc[P] - rows_sum(pa[P]) : rc[P];
      double t4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) t4[r] = T[tri(P, P)][r] * rp;
      allred16(t4);  // t_P[g+4r]
#pragma unroll
      for (int i = P + 1; i < NQ; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) pa[i] = fma(T[tri(i, P)][r], t4[r], pa[i]);
      if (cl < 4) LDS(vout + 16 * P + g + 4 * cl) = cl == 0 ? t4[0] : (cl == 1 ? t4[1] : (cl == 2 ? t4[2] : t4[3]));
#pragma unroll
      for (int r = 0; r < 4; ++r) tv[P][r] = t4[r];
    }
    SYNC();
  }
  // out = L^-T v: x_P = W_P' (v_P - sum_{i>P} L_iP' x_i); in place is allowed.
  // xs: x in column layout (every lane holds x[16P+cl]).
  __device__ __forceinline__ void trsv_bwd(int vin, int vout, double (&xs)[NQ]) {
    MARK_BEGIN("trsv_bwd");
    LANE_IDS();
    double ur[NQ][4], pa[NQ][4];  // v (row layout), lane partials of sum_i L_iP' x_i
#pragma unroll
    for (int P = 0; P < NQ; ++P)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ur[P][r] = LDS(vin + 16 * P + g + 4 * r);
        pa[P][r] = 0.0;
      }
#pragma unroll
    for (int P = NQ - 1; P >= 0; --P) {
      double u4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) u4[r] = pa[P][r];
      if (P < NQ - 1) allred16(u4);
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = fma(T[tri(P, P)][r], P < NQ - 1 ? ur[P][r] - u4[r] : ur[P][r], acc);
      const double x = rows_sum(acc);  // x_P[cl]
      xs[P] = x;
#pragma unroll
      for (int Q = 0; Q < P; ++Q)
#pragma unroll
        for (int r = 0; r < 4; ++r) pa[Q][r] = fma(T[tri(P, Q)][r], x, pa[Q][r]);
    }
    SYNC();
    if (g == 0) {
#pragma unroll
      for (int P = 0; P < NQ; ++P) LDS(vout + 16 * P + cl) = xs[P];
    }
    SYNC();
  }

  // out[row] = (G u)[row] + add1[row] - add2[row] for rows < k (u in column layout).
  // Rows are reduced over the 16 column lanes in chunks of up to 8 row-steps.
  //
  // FU (the residuals' pass on launches with SmallArgs::fuse_u): the pass also
  // forms the SYRK's cone rows, U[c,:] = (sum_{i in c} w_i G[i,:]) / (1+wb0),
  // from the G rows it has taken out of the AGPRs anyway, in compute_U's
  // operation order (per cone: ascending row steps from 0.0, rows_sum, * CC_I1),
  // so the same bits.  Every cone is 32 or 64 rows there and starts on a
  // multiple of its length: a chunk of 8 row steps lies in one cone, a cone is
  // one chunk or two, and it can only end with a chunk -- one flush site per
  // chunk.  ua: the accumulators, carried from chunk to chunk.  The chunk's
  // weights and 1/(1+wb0) are read with its addends (one round trip); a POC
  // chunk skips the U work by a wave-uniform branch.  The U part stands apart
  // from the products, after them: a branch per row step cuts the products'
  // scheduling region into pieces (+0.5 ms at C2).
  template <int P0, int CH, bool NEG = false, bool FU = false>
  __device__ __forceinline__ void gemv_G_chunk(const double (&uq)[NQ], int add1, int add2, int out,
                                               double (&ua)[NQ]) {
    LANE_IDS();
    constexpr int CF = RSCount<CH, 8>::value;
    // the addends of the rows this lane ends up holding, read before the products
    double a1[CF], a2[CF];
    {
      const int b0 = rs16_base<CH, 8>(cl);
#pragma unroll
      for (int j = 0; j < CF; ++j) {
        const int row = 4 * (P0 + b0 + j) + g;  // < KP: in the k-vector
        a1[j] = add1 >= 0 ? LDS(add1 + row) : 0.0;
        a2[j] = LDS(add2 + row);
      }
    }
    static_assert(!FU || P0 % 8 == 0, "whole chunks");
    double uw[FU ? CH : 1], ui = 0.0;
    bool usoc = false;  // wave-uniform: the chunk's cone is SOC
    int ucone = 0, upos = 0, ulast = 0;
    if constexpr (FU && CH == 8) {
      ulast = al_rows() == 4;  // a cone is two chunks (64 rows) or one (32)
      ucone = (P0 / 8) >> ulast;
      upos = (P0 / 8) & ulast;  // the chunk's place in its cone
      usoc = (fuse_u() >> ucone) & 1;
      if (usoc) {
#pragma unroll
        for (int j = 0; j < CH; ++j) uw[j] = LDS(WB + 4 * (P0 + j) + g);
        ui = LDS(cc(CC_I1, ucone));
      }
    }
    double P[CH];
    double gk[FU ? CH : 1][NQ];  // FU: the chunk's G rows, kept for the U part below
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      double acc = 0.0;
      {
        double gr[NQ];
        a_get_row<NQ>(G[P0 + j], gr);
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc = fma(gr[q], uq[q], acc);
        if constexpr (FU) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) gk[j][q] = gr[q];
        }
      }
      P[j] = acc;
    }
    if constexpr (FU && CH == 8) {
      if (usoc) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          double w = uw[j];
          if (j == 0) w = (g == 0 && upos == 0) ? -(1.0 + w) : w;  // the cone's head row
#pragma unroll
          for (int q = 0; q < NQ; ++q) ua[q] = fma(w, gk[j][q], ua[q]);
        }
        if (upos == ulast) {  // the cone's last chunk
#pragma unroll
          for (int q = 0; q < NQ; ++q) ua[q] = rows_sum(ua[q]);
          if (g == 0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) LDS(O_U + ucone * NPAD + 16 * q + cl) = ua[q] * ui;
          }
#pragma unroll
          for (int q = 0; q < NQ; ++q) ua[q] = 0.0;
        }
      }
    }
    int base = 0;
    rs16<CH, 8>(P, cl, base);
#pragma unroll
    for (int j = 0; j < CF; ++j) {
      const int row = 4 * (P0 + base + j) + g;
      if (row < k) {
        double v = P[j];
        if (add1 >= 0) v = v + a1[j];
        v = v - a2[j];
        LDS(out + row) = NEG ? -v : v;
      }
    }
    if constexpr (P0 + CH < NP) {
      constexpr int NXT = (NP - P0 - CH) < 8 ? (NP - P0 - CH) : 8;
      gemv_G_chunk<P0 + CH, NXT, NEG, FU>(uq, add1, add2, out, ua);
    }
  }
  __device__ __forceinline__ void gemv_G(int u, int add1, int add2, int out) {
    MARK_BEGIN("gemv_G");
    LANE_IDS();
    double uq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) uq[q] = LDS(u + 16 * q + cl);
    double ua[NQ];  // (FU off: unused)
    gemv_G_chunk<0, (NP < 8 ? NP : 8)>(uq, add1, add2, out, ua);
    SYNC();
  }
  // the same with u in column layout in registers (uq[q] = u[16q+cl]); NEG:
  // store the negated rows; FU: form U as well where the launch fuses it
  template <bool NEG = false, bool FU = false>
  __device__ __forceinline__ void gemv_G_r(const double (&uq)[NQ], int add1, int add2, int out) {
    MARK_BEGIN("gemv_G");
    double ua[NQ];
    if constexpr (FU) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) ua[q] = 0.0;
    }
    gemv_G_chunk<0, (NP < 8 ? NP : 8), NEG, FU>(uq, add1, add2, out, ua);
    SYNC();
  }

  // acc[q] (all lanes) = (G' v)[16q+cl].  The v reads of the next batch of
  // row steps are issued before the current batch's products (one exposed
  // LDS round trip per call, not one per pair of row steps).  hook.run<b>()
  // runs inside batch b's scheduling region (b < 2): independent work whose
  // latency the batch's VALU stream hides (resid_scaling).
  struct NoGtHook {
    template <int B>
    __device__ __forceinline__ void run() {}
  };
  template <class HK = NoGtHook>
  __device__ __forceinline__ void gemv_Gt(int v, double (&acc)[NQ], HK&& hook = HK()) {
    MARK_BEGIN("gemv_Gt");
    LANE_IDS();
    constexpr int VB = 8;
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    double vb[VB];
#pragma unroll
    for (int j = 0; j < VB; ++j) vb[j] = j < NP ? LDS(v + 4 * j + g) : 0.0;
#pragma unroll
    for (int p0 = 0; p0 < NP; p0 += VB) {
      double vn[VB];
#pragma unroll
      for (int j = 0; j < VB; ++j) vn[j] = p0 + VB + j < NP ? LDS(v + 4 * (p0 + VB + j) + g) : 0.0;
      SCHED_FENCE();
      if (p0 == 0) hook.template run<0>();
      if (p0 == VB) hook.template run<1>();
#pragma unroll
      for (int j = 0; j < VB; ++j) {
        if (p0 + j < NP) {
          {
            double gr[NQ];
            a_get_row<NQ>(G[p0 + j < NP ? p0 + j : 0], gr);
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = fma(gr[q], vb[j], acc[q]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < VB; ++j) vb[j] = vn[j];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      acc[q] = rows_sum(acc[q]);
    }
  }

  static constexpr int LDS_BATCH = 16;  // LDS reads issued per round trip in the A products (8 where HOIST_CST is off)
  static constexpr int LDB = HOIST_CST ? LDS_BATCH : 8;
  static constexpr int AMB = (NQ * 4) % LDB == 0 ? LDB : 4;
  static constexpr int ATB = (MQ * 4) % (LDB / NQ > 0 ? LDB / NQ : 1) == 0 ? (LDB / NQ > 0 ? LDB / NQ : 1) : 1;
  // acc[q] (all lanes) = (A' v)[16q+cl]: rows split over the 4 lane groups
  // vr (optional): v in registers, vr[s] = v[g + 4s] (s < 4 MQ), instead of LDS
  __device__ __forceinline__ void At_mv(int v, double (&acc)[NQ], int base = O_A, const double* vr = nullptr) {
    MARK_BEGIN("At_mv");
    LANE_IDS();
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    // the reads of a step batch issued before its products (one LDS round
    // trip per LDB rows, not one per row: the scheduler otherwise
    // interleaves read, wait, fma)
#pragma unroll
    for (int s0 = 0; s0 < MQ * 4; s0 += ATB) {
      double vi[ATB], av[ATB][NQ];
#pragma unroll
      for (int s = 0; s < ATB; ++s) {
        const int i = g + 4 * (s0 + s);
        vi[s] = vr ? vr[s0 + s] : LDS(v + i);
#pragma unroll
        for (int q = 0; q < NQ; ++q) av[s][q] = LDS(base + i * LDA + 16 * q + cl);
      }
      SCHED_FENCE();
#pragma unroll
      for (int s = 0; s < ATB; ++s)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = fma(av[s][q], vi[s], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      acc[q] = rows_sum(acc[q]);
    }
  }
  // out[i] = (A u)[i] - sub[i] for i < m (columns split over the 4 lane groups);
  // returns sum of out[i]^2 on lanes g == 0
  __device__ __forceinline__ double A_mv(int u, int sub, int out, int base = O_A, bool neg = false) {
    MARK_BEGIN("A_mv");
    LANE_IDS();
    double sq = 0.0;
#pragma unroll
    for (int tm = 0; tm < MQ; ++tm) {
      const int i = 16 * tm + cl;
      double acc = 0.0;
#pragma unroll
      for (int t0 = 0; t0 < NQ * 4; t0 += AMB) {
        double av[AMB], uv[AMB];
#pragma unroll
        for (int t = 0; t < AMB; ++t) {
          av[t] = LDS(base + i * LDA + g + 4 * (t0 + t));
          uv[t] = LDS(u + g + 4 * (t0 + t));
        }
        SCHED_FENCE();
#pragma unroll
        for (int t = 0; t < AMB; ++t) acc = fma(av[t], uv[t], acc);
      }
      acc = rows_sum(acc);
      if (g == 0 && i < m) {
        const double v = acc - LDS(sub + i);
        LDS(out + i) = neg ? -v : v;
        sq = fma(v, v, sq);
      }
    }
    return sq;
  }

  // A_mv with u in row layout in registers (tv[P][r] = u[16P+g+4r], trsv_fwd_r's
  // output): the same products in the same order
  // (mc: the result in column layout in every lane, mc[tm] = out[16 tm + cl],
  // 0 for rows >= m)
  __device__ __forceinline__ double A_mv_r(const double (&tv)[NQ][4], int sub, int out, int base, double (&mc)[MQ]) {
    MARK_BEGIN("A_mv");
    LANE_IDS();
    double sq = 0.0;
#pragma unroll
    for (int tm = 0; tm < MQ; ++tm) {
      const int i = 16 * tm + cl;
      const double sb = LDS(sub + i);
      double acc = 0.0;
#pragma unroll
      for (int t0 = 0; t0 < NQ * 4; t0 += AMB) {
        double av[AMB];
#pragma unroll
        for (int t = 0; t < AMB; ++t) av[t] = LDS(base + i * LDA + g + 4 * (t0 + t));
        SCHED_FENCE();
#pragma unroll
        for (int t = 0; t < AMB; ++t) acc = fma(av[t], tv[(t0 + t) >> 2][(t0 + t) & 3], acc);
      }
      acc = rows_sum(acc);
      const double v = acc - sb;
      if (g == 0 && i < m) {
        LDS(out + i) = v;
        sq = fma(v, v, sq);
      }
      mc[tm] = i < m ? v : 0.0;
    }
    return sq;
  }

  // The matrix part of solve_kkt(::DenseSolver) (densesolver.jl:66-85), between
  // the cone ops: n0 = GWiWi*k2 + dx (+A'dy if sing); m0 = ALi*n0 - dy, taken as
  // A*(Li*n0) - dy; cy = S^-1 m0; m0 = sing ? dy - cy : -cy (init: -cy);
  // n0 += A'm0; cx = Li n0; k1 = G cx - k2.   In: RD RP T2(=W^-2 k2) K2.  Out: RX RY K1.
  __device__ __forceinline__ void solve_matrix_part(bool init) {
    MARK_BEGIN("solve_matrix_part");
    LANE_IDS();
    // n0 in column layout, in every lane (the CHOL path hands it to trsv_fwd_r
    // in registers; the explicit-inverse kernels' symv reads it from N0)
    double n0[NQ];
    {
      double acc[NQ], at[NQ];
      if (SOCP_KO & 512) {
        for (int q = 0; q < NQ; ++q) acc[q] = LDS(T2 + 16 * q + cl);
      } else {
        gemv_Gt(T2, acc);
      }
      if (sing) At_mv(RP, at);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = 16 * q + cl;
        double v = acc[q] + LDS(RD + j);
        if (sing) v = v + at[q];
        n0[q] = v;
      }
      if (!CHOL && g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) LDS(N0 + 16 * q + cl) = n0[q];
      }
    }
    if constexpr (!CHOL) SYNC();
    STAMP_X(4);
    double tv[NQ][4];  // t = L^-1 n0 in row layout (CHOL)
    double cxr[NQ];    // cx in column layout (CHOL: trsv_bwd's output)
    if constexpr (CHOL) {
      if (SOCP_KO & 256) {
        if (g == 0)
          for (int q = 0; q < NQ; ++q) LDS(TN + 16 * q + cl) = n0[q];
        SYNC();
        for (int P = 0; P < NQ; ++P)
          for (int r = 0; r < 4; ++r) tv[P][r] = LDS(TN + 16 * P + g + 4 * r);
      } else {
        trsv_fwd_r(n0, TN, tv);  // t = L^-1 n0
      }
    } else
      symv<NQ>(T, N0, TN);   // Li n0
    STAMP_X(5);
    // CHOL with one S tile: m0, cy and the next m0 stay in registers
    constexpr bool MREG = CHOL && MQ == 1;
    double m0c[MQ], m0r[4];
    if (SOCP_KO & 2048) {
      for (int j = lane; j < m; j += 64) LDS(M0 + j) = LDS(TN + j);
    } else if constexpr (CHOL)
      A_mv_r(tv, RP, M0, O_AL, m0c);  // m0 = A Li n0 - dy = Z't - dy
    else if constexpr (AL_LDS)
      A_mv(N0, RP, M0, O_AL);  // m0 = (A Li) n0 - dy: no wait for Li n0
    else
      A_mv(TN, RP, M0);        // m0 = A (Li n0) - dy
    if constexpr (MREG) {
      if (SOCP_KO & 2048) {
        SYNC();
        for (int j = lane; j < m; j += 64) LDS(RY + j) = LDS(M0 + j);
        SYNC();
        for (int s = 0; s < 4; ++s) m0r[s] = LDS(RY + g + 4 * s);
      } else {
        double rp[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) rp[s] = LDS(RP + g + 4 * s);
        symv1_r(Sv[0], m0c[0], RY, m0r);  // cy = S^-1 m0
#pragma unroll
        for (int s = 0; s < 4; ++s)
          m0r[s] = g + 4 * s < m ? ((sing && !init) ? rp[s] - m0r[s] : -m0r[s]) : 0.0;
      }
    } else {
      SYNC();
      if (SOCP_KO & 2048) {
        for (int j = lane; j < m; j += 64) LDS(RY + j) = LDS(M0 + j);
        SYNC();
      } else {
        symv<MQ>(Sv, M0, RY);  // cy = S^-1 m0
      }
      if (lane < m) LDS(M0 + lane) = (sing && !init) ? LDS(RP + lane) - LDS(RY + lane) : -LDS(RY + lane);
      SYNC();
    }
    STAMP_X(6);
    if constexpr (AL_LDS) {
      // cx = Li (n0 + A'm0) = Li n0 + (A Li)' m0: one Li product per solve
      // (CHOL: cx = L^-T (t + Z m0))
      double at[NQ], tn[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) tn[q] = LDS(TN + 16 * q + cl);  // read with At_mv's operands
      if (SOCP_KO & 2048) {
        for (int q = 0; q < NQ; ++q) at[q] = 0.0;
      } else {
        At_mv(M0, at, O_AL, MREG ? m0r : nullptr);
      }
      if (g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) LDS(RX + 16 * q + cl) = tn[q] + at[q];
      }
      SYNC();
      if constexpr (CHOL) {
        if (!(SOCP_KO & 256)) {
          trsv_bwd(RX, RX, cxr);
        } else {
#pragma unroll
          for (int q = 0; q < NQ; ++q) cxr[q] = LDS(RX + 16 * q + cl);
        }
      }
      STAMP_X(7);
    } else {
      double at[NQ];
      At_mv(M0, at);
      if (g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) LDS(N0 + 16 * q + cl) = LDS(N0 + 16 * q + cl) + at[q];
      }
      SYNC();
      symv<NQ>(T, N0, RX);  // cx = Li n0
    }
    if (SOCP_KO & 1024) {
      for (int i = lane; i < k; i += 64) LDS(K1 + i) = LDS(RX + (i & 63)) - LDS(K2 + i);
      SYNC();
    } else if constexpr (CHOL) {
      gemv_G_r(cxr, -1, K2, K1);  // cx from trsv_bwd's registers
    } else {
      gemv_G(RX, -1, K2, K1);
    }
  }

  // ------------------------------------------------------- factor record
  // setup_iter's products for the later solve_kkt calls: H^-1 and S^-1 in
  // register-tile (lane) order, the scaling vectors and per-cone constants the
  // solves read, and `sing` (densesolver.jl:41-52 keeps them in the solver
  // object; here one record per problem in HBM).
  static __device__ constexpr int rec_kv(int v) {
    return v == 0 ? KV_LAM : v == 1 ? KV_WB : v == 2 ? KV_CA : v == 3 ? KV_CB : KV_IL;
  }
  static constexpr int64_t REC_SING = (int64_t)(NT + MT) * 256 + 5 * KP + 20 * NCS + (AL_LDS ? MPAD * LDA : 0);
  static constexpr int64_t REC_STATUS = REC_SING + 1;  // setup_iter's status, read first by solve_kkt
  static_assert(REC_SING + 8 == small_rec_doubles(NQ, NP, MQ), "the host's record stride");
  __device__ __forceinline__ void store_record(int64_t p) {
    LANE_IDS();
    double* r = a.rec + p * a.rec_stride;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) r[(t * 4 + q) * 64 + lane] = T[t][q];
    r += NT * 256;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) r[(t * 4 + q) * 64 + lane] = Sv[t][q];
    r += MT * 256;
#pragma unroll
    for (int v = 0; v < 5; ++v)
      for (int i = lane; i < KP; i += 64) r[v * KP + i] = LDS(kvs(rec_kv(v)) + i);
    r += 5 * KP;
    for (int i = lane; i < 20 * NCS; i += 64) r[i] = LDS(O_CC + i);
    if constexpr (AL_LDS)
      for (int i = lane; i < MPAD * LDA; i += 64) r[20 * NCS + i] = LDS(O_AL + i);
    if (lane == 0) r[REC_SING - (NT + MT) * 256 - 5 * KP] = sing ? 1.0 : 0.0;  // REC_SING
  }
  __device__ __forceinline__ void load_record(int64_t p) {
    LANE_IDS();
    const double* r = a.rec + p * a.rec_stride;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) T[t][q] = r[(t * 4 + q) * 64 + lane];
    r += NT * 256;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) Sv[t][q] = r[(t * 4 + q) * 64 + lane];
    r += MT * 256;
#pragma unroll
    for (int v = 0; v < 5; ++v)
      for (int i = lane; i < KP; i += 64) LDS(kvs(rec_kv(v)) + i) = r[v * KP + i];
    r += 5 * KP;
    for (int i = lane; i < 20 * NCS; i += 64) LDS(O_CC + i) = r[i];
    if constexpr (AL_LDS)
      for (int i = lane; i < MPAD * LDA; i += 64) LDS(O_AL + i) = r[20 * NCS + i];
    sing = uni(r[REC_SING - (NT + MT) * 256 - 5 * KP]) != 0.0;
    SYNC();
  }

  // SOCP_F_DETECT_INFEASIBLE: the rule of include/socp.h at the iterate whose
  // residuals MP_ITER has just formed.  The residual vectors are stored
  // negated (RD = -(A'y + G'z + c), RP = b - Ax, DZ = h - Gx - s), so
  // A'y + G'z = -RD - c, Ax = b - RP, Gx + s = h - DZ.  One interleaved
  // whole-wave scan of the five sums.
  __device__ __forceinline__ int infeas_check(double& scale) {
    LANE_IDS();
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < k; i += 64) {
      const double hi = LDS(H_ + i);
      const double gs = hi - LDS(DZ + i);
      v[0] = fma(hi, LDS(Z_ + i), v[0]);
      v[4] = fma(gs, gs, v[4]);
    }
    for (int i = lane; i < m; i += 64) {
      const double bi = LDS(B_ + i);
      const double ax = bi - LDS(RP + i);
      v[0] = fma(bi, LDS(Y_ + i), v[0]);
      v[3] = fma(ax, ax, v[3]);
    }
    for (int j = lane; j < n; j += 64) {
      const double cj = LDS(C_ + j);
      const double t = -LDS(RD + j) - cj;
      v[1] = fma(t, t, v[1]);
      v[2] = fma(cj, LDS(X_ + j), v[2]);
    }
    dpp_scan<5>(v, lane, 0, false);
    return infeas_verdict(readlane_d(v[0], 63), readlane_d(v[1], 63), readlane_d(v[2], 63), readlane_d(v[3], 63),
                          readlane_d(v[4], 63), small_itol(a), scale);
  }

  // ------------------------------------------------------------- driver
  // solve_socp (solver.jl:40-153) as a micro-phase loop.  solve_kkt
  // (densesolver.jl:54-90) is MP_SOLVE_HEAD -> MP_SOLVE_MAT -> MP_SOLVE_TAIL;
  // `ret` says which solve it is (init, KKT entry, affine, combined).
  // KM = 0: the solver kernel (MODE_SOLVE); KM = 1: the plugin-entry kernel
  // (MODE_KKT, MODE_SETUP, MODE_SOLVEKKT), compiled apart so the solver's
  // register allocation does not carry the entry paths.  DI: the solver with
  // SOCP_F_DETECT_INFEASIBLE, an instantiation of its own for the same reason.
  // OV, h_formed: a kernel with the pipelined load, and whether this problem's
  // load_problem left G'G in T (a value of this call, not of the wave)
  template <int KM, bool DI = false, bool OV = false>
  __device__ __forceinline__ void run(int64_t p, bool h_formed = false) {
    const int mode = KM ? a.mode : (a.mode == MODE_KKT ? (int)MODE_KKT : (int)MODE_SOLVE);
    STAMP(SP_LOAD);
    dbg_p = p;
    int status = ST_MAXIT, iters = 0, it = 0;
    double nd = NAN, np_ = NAN, gap = NAN;
    double ll = 0.0;
    int fac_kind = FAC_SCALED;
    bool fac_aa = false, dm_aa = false;
    int fret = 0, ret = 0, fst = 0;
    double isc = 1.0;  // DI: the certificate's factor
    int after_singtest;
    bool have_sing = false;
    if constexpr (QP) {
      // (MODE_SOLVEKKT solves against the record and never reads it)
      qp_P = (KM ? small_qp_plugin(a) : small_qp(a)) + ((a.flags & F_SHARED) ? 0 : p * (int64_t)n * n);
      qp_hrange = n * n * (int)sizeof(double);
    }
    if (mode == MODE_SOLVEKKT) {  // setup_iter failed for this problem: NaN solution, its status
      const int st0 = (int)uni(a.rec[p * a.rec_stride + REC_STATUS]);
      if (st0) {
        for (int j = lane; j < n; j += 64) a.cx[p * n + j] = NAN;
        for (int i = lane; i < m; i += 64) a.cy[p * m + i] = NAN;
        for (int i = lane; i < k; i += 64) {
          a.cz[p * k + i] = NAN;
          a.cs[p * k + i] = NAN;
        }
        if (lane == 0) a.status[p] = st0;
        return;
      }
    }
    if (mode == MODE_KKT || mode == MODE_SETUP || mode == MODE_SOLVEKKT) {
      for (int i = lane; i < k; i += 64) {
        if (mode != MODE_SOLVEKKT) {
          LDS(S_ + i) = a.s[p * k + i];
          LDS(Z_ + i) = a.z[p * k + i];
        }
        if (mode != MODE_SETUP) {
          LDS(DZ + i) = a.dz[p * k + i];
          LDS(DS + i) = a.ds[p * k + i];
        }
      }
      if (mode != MODE_SETUP) {
        for (int j = lane; j < n; j += 64) LDS(RD + j) = a.dx[p * n + j];
        for (int i = lane; i < m; i += 64) LDS(RP + i) = a.dy[p * m + i];
      }
      after_singtest = MP_KKT;
      if (mode == MODE_SOLVEKKT) {  // solve_kkt against the setup_iter record
        load_record(p);
        have_sing = true;
        after_singtest = MP_SOLVE_HEAD;
        ret = RET_KKT;
      }
    } else if (a.flags & F_WARM) {
      for (int j = lane; j < n; j += 64) LDS(X_ + j) = a.x[p * n + j];
      for (int i = lane; i < m; i += 64) LDS(Y_ + i) = a.y[p * m + i];
      for (int i = lane; i < k; i += 64) {
        LDS(Z_ + i) = a.z[p * k + i];
        LDS(S_ + i) = a.s[p * k + i];
      }
      after_singtest = MP_ITER;
    } else {
      after_singtest = MP_INIT;
    }
    SYNC();
    int phase;
    if (have_sing) {
      phase = after_singtest;
    } else if (a.sing) {
      sing = uni((int)a.sing[(a.flags & F_SHARED) ? 0 : p]) != 0;
      phase = after_singtest;
    } else {
      sing = false;
      phase = MP_SINGTEST;
    }
    bool done = false;
    while (!done) {
      LANE_IDS();
      if (KM && phase == MP_SAVE) {  // setup_iter done: keep the factorisation for the solves
        // (outside the switch: the solver kernel's phase switch is left as it
        // was tuned -- an extra case there re-lays the loop and costs ~4%)
        store_record(p);
        status = 0;
        break;
      }
      int next = phase;
      switch (phase) {
        case MP_SINGTEST:  // Problem's `sing` (Socp.jl:49-56): is G'G positive definite?
          MARK_BEGIN("case MP_SINGTEST");
          if constexpr (QP) qp_hrange = 0;  // cholesky(G'G): without P
          scaling_identity();
          fac_kind = FAC_IDENT;
          // (the probe is a problem's first factorisation whenever it runs)
          if constexpr (OV) fac_kind = h_formed ? FAC_IDENT_H : FAC_IDENT;
          fac_aa = false;
          fret = MP_SINGTEST_POST;
          next = MP_FACTOR;
          break;
        case MP_SINGTEST_POST:
          MARK_BEGIN("case MP_SINGTEST_POST");
          sing = (fst == ST_CHOL_H);
          if constexpr (QP) qp_hrange = n * n * (int)sizeof(double);
          next = after_singtest;
          break;
        case MP_FACTOR:  // setup_iter (densesolver.jl:41-52)
          MARK_BEGIN("case MP_FACTOR");
          fst = factor<OV>(fac_kind, fac_aa);
          if (fst && fret != MP_SINGTEST_POST) {
            status = fst;
            done = true;
          }
          next = fret;
          break;
        case MP_INIT:  // initial point: the KKT system with W = I (solver.jl:68-84)
          MARK_BEGIN("case MP_INIT");
          scaling_identity();
          for (int j = lane; j < n; j += 64) LDS(RD + j) = -LDS(C_ + j);
          for (int i = lane; i < m; i += 64) LDS(RP + i) = LDS(B_ + i);
          for (int i = lane; i < k; i += 64) {
            LDS(DZ + i) = LDS(H_ + i);
            LDS(DS + i) = 0.0;
          }
          SYNC();
          fac_kind = FAC_IDENT;
          // (the first factorisation only with `sing` given: a probe has factored T in place)
          if constexpr (OV) fac_kind = (h_formed && a.sing) ? FAC_IDENT_H : FAC_IDENT;
          fac_aa = sing;
          fret = MP_SOLVE_HEAD;
          ret = RET_INIT;
          next = MP_FACTOR;
          break;
        case MP_ITER: {  // residuals (solver.jl:109-118), compute_scaling (:106), exit test (:122)
          MARK_BEGIN("case MP_ITER");
          STAMP(SP_OTHER);
          // after the last iteration the reference loop ends without another
          // residual evaluation (solver.jl:105-151): they are formed then only
          // when the caller asked for the final residual norms
          if (it >= a.maxit && !a.res) {
            done = true;
            break;
          }
          // residuals and compute_scaling interleaved
          // (after the last iteration the scaling is computed too, and unused)
          const bool dm = resid_scaling<!(SOCP_KO & 2), !(SOCP_KO & 4096)>(nd, np_, gap, ll, dm_aa);
          STAMP(SP_RESID);
          if (it >= a.maxit) {
            done = true;
            break;
          }
          STAMP(SP_VOP);
          if (dm) {
            status = ST_DOMAIN;
            done = true;
            break;
          }
          if (nd + np_ + gap < a.tol) {
            status = ST_CONVERGED;
            done = true;
            break;
          }
          if constexpr (DI) {
            const int iv = infeas_check(isc);
            if (iv) {
              status = iv;
              done = true;
              break;
            }
          }
          // (rmul!(dx, -1) etc., solver.jl:124: the residuals and ds were stored negated)
          // (fused launches: resid_scaling's G x pass has left this scaling's U in LDS)
          fac_kind = (!(SOCP_KO & (2 | 4 | 16 | 4096)) && fuse_u()) ? FAC_SCALED_U : FAC_SCALED;
          fac_aa = sing;
          fret = MP_SOLVE_HEAD;
          ret = RET_AFFINE;
          next = MP_FACTOR;
          break;
        }
        case MP_KKT: {
          MARK_BEGIN("case MP_KKT");
          const bool dm = scaling_op(ll, dm_aa, false);
          if (dm) {
            status = ST_DOMAIN;
            done = true;
            break;
          }
          fac_kind = FAC_SCALED;
          fac_aa = sing;
          fret = mode == MODE_SETUP ? MP_SAVE : MP_SOLVE_HEAD;
          ret = RET_KKT;
          next = MP_FACTOR;
          break;
        }
        case MP_SOLVE_HEAD: {
          // a solve (densesolver.jl:54-90) -- head, matrix part, tail -- and,
          // after the affine one, the combined one: without trips through the
          // phase dispatch (each costs ~1 %)
          for (;;) {
            MARK_BEGIN("case MP_SOLVE_HEAD");
            STAMP(SP_OTHER);
            solve_head();
            STAMP(SP_VOP);
            MARK_BEGIN("case MP_SOLVE_MAT");
            solve_matrix_part(ret == RET_INIT);
            STAMP(SP_SOLVE);
            MARK_BEGIN("case MP_SOLVE_TAIL");
            const bool do_step = ret == RET_AFFINE || ret == RET_COMBINED;
            int dom = 0;
            const double tstep = solve_tail(do_step, dm_aa, dom);
            STAMP(SP_VOP);
            if (ret == RET_KKT) {
              status = 0;
              for (int j = lane; j < n; j += 64) a.cx[p * n + j] = LDS(RX + j);
              for (int i = lane; i < m; i += 64) a.cy[p * m + i] = LDS(RY + i);
              for (int i = lane; i < k; i += 64) {
                a.cz[p * k + i] = LDS(RZ + i);
                a.cs[p * k + i] = LDS(RS + i);
              }
              done = true;
              break;
            }
            if (ret == RET_INIT) {  // cone shift (solver.jl:86-104)
              double alphp, alphd;  // max_step(-iz), max_step(iz)
              maxstep_op(RZ, alphp, alphd);
              for (int j = lane; j < n; j += 64) LDS(X_ + j) = LDS(RX + j);
              for (int i = lane; i < m; i += 64) LDS(Y_ + i) = LDS(RY + i);
              for (int i = lane; i < k; i += 64) {
                const double iz = LDS(RZ + i), e = e_of(i);
                LDS(S_ + i) = (fabs(alphp) < a.init_eps) ? -iz : -iz + (1.0 + alphp) * e;
                LDS(Z_ + i) = (fabs(alphd) < a.init_eps) ? iz : iz + (1.0 + alphd) * e;
              }
              SYNC();
              next = MP_ITER;
              break;
            }
            if (dom) {
              status = ST_DOMAIN;
              done = true;
              break;
            }
            if (ret == RET_AFFINE) {  // centering + corrector, then the combined solve
              affine_post(tstep, ll);
              STAMP(SP_STEP);
              ret = RET_COMBINED;
              continue;
            }
            // combined direction: step and update (solver.jl:143-150)
            const double stp = tstep * a.step;
            {  // every read first (n, m <= 64, k <= 128 here), then the updates
              constexpr int NS = KP > 64 ? 2 : 1;
              const int ly = lane < MPAD ? lane : 0;
              const double xo = LDS(X_ + lane), rx = LDS(RX + lane), yo = LDS(Y_ + ly), ry = LDS(RY + ly);
              double zo[NS], rz[NS], so[NS], rs[NS];
#pragma unroll
              for (int t = 0; t < NS; ++t) {
                const int i = 64 * t + lane;
                zo[t] = LDS(Z_ + i);
                rz[t] = LDS(RZ + i);
                so[t] = LDS(S_ + i);
                rs[t] = LDS(RS + i);
              }
              if (lane < n) LDS(X_ + lane) = xo + rx * stp;
              if (lane < m) LDS(Y_ + lane) = yo + ry * stp;
#pragma unroll
              for (int t = 0; t < NS; ++t) {
                const int i = 64 * t + lane;
                if (i < k) {
                  LDS(Z_ + i) = zo[t] + rz[t] * stp;
                  LDS(S_ + i) = so[t] + rs[t] * stp;
                }
              }
            }
            SYNC();
            STAMP(SP_STEP);
            iters = ++it;
            next = MP_ITER;
            break;
          }
          break;
        }
        default:
          done = true;
          break;
      }
      if (done) break;
      phase = uni(next);
    }
    if (mode != MODE_SOLVE) {
      if constexpr (QP && KM != 0) {
        // the fused QP entry returns what setup_iter + solve_kkt return for a failed problem
        // (socp.h: bitwise the split calls), as the blocked kernel's does: a NaN solution
        if (status && mode == MODE_KKT) {
          for (int j = lane; j < n; j += 64) a.cx[p * n + j] = NAN;
          for (int i = lane; i < m; i += 64) a.cy[p * m + i] = NAN;
          for (int i = lane; i < k; i += 64) {
            a.cz[p * k + i] = NAN;
            a.cs[p * k + i] = NAN;
          }
        }
      }
      if (lane == 0) a.status[p] = status;
      if (mode == MODE_SETUP && lane == 0) a.rec[p * a.rec_stride + REC_STATUS] = (double)status;
      SYNC();
      STAMP(SP_STORE);
      return;
    }
    if constexpr (DI) {  // the certificate's pair times its factor (1 otherwise: x * 1.0 is x)
      const double fp = status == ST_DUAL_INF ? isc : 1.0, fd = status == ST_PRIMAL_INF ? isc : 1.0;
      for (int j = lane; j < n; j += 64) a.x[p * n + j] = LDS(X_ + j) * fp;
      for (int i = lane; i < m; i += 64) a.y[p * m + i] = LDS(Y_ + i) * fd;
      for (int i = lane; i < k; i += 64) {
        a.z[p * k + i] = LDS(Z_ + i) * fd;
        a.s[p * k + i] = LDS(S_ + i) * fp;
      }
    } else {
    for (int j = lane; j < n; j += 64) a.x[p * n + j] = LDS(X_ + j);
    for (int i = lane; i < m; i += 64) a.y[p * m + i] = LDS(Y_ + i);
    for (int i = lane; i < k; i += 64) {
      a.z[p * k + i] = LDS(Z_ + i);
      a.s[p * k + i] = LDS(S_ + i);
    }
    }
    if (lane == 0) {
      if (a.res) {
        a.res[3 * p + 0] = nd;
        a.res[3 * p + 1] = np_;
        a.res[3 * p + 2] = gap;
      }
      a.iters[p] = iters;
      a.status[p] = status;
    }
    SYNC();
    STAMP(SP_STORE);
#ifdef SOCP_DIAG
    if (lane == 0) reinterpret_cast<unsigned long long*>(socp_lds + O_STAMPS)[NSTAMP] += iters;
#endif
  }

  // The exact-fit kernel's driver: solve_socp (solver.jl:40-153) as one loop,
  // a trip per factorisation.  A trip is the probe of G'G (XK_PROBE, only when
  // the call gives no `sing`), the initial point (XK_INIT, unless warm-started)
  // or an iteration (XK_ITER); what differs between them is steered by `kind`,
  // so factor() and the solve body are inlined once, as in run().  The
  // operations and their order are run<0>'s for MODE_SOLVE: the same bits.
  // The trip kind is the only state a trip hands to the next; `fac` kinds are
  // named per request and h_formed is a value of the call, as in run().
  enum : int { XK_PROBE, XK_INIT, XK_ITER };
  template <bool OV>
  __device__ __forceinline__ void run_exact(int64_t p, bool h_formed) {
    static_assert(EX && OV && !QP && !XI, "the exact-fit solver kernel");
    STAMP(SP_LOAD);
    dbg_p = p;
    int status = ST_MAXIT, iters = 0, it = 0;
    double nd = NAN, np_ = NAN, gap = NAN;
    double ll = 0.0;
    bool dm_aa = false;
    int first = XK_INIT;
    if (a.flags & F_WARM) {
      for (int j = lane; j < n; j += 64) LDS(X_ + j) = a.x[p * n + j];
      for (int i = lane; i < m; i += 64) LDS(Y_ + i) = a.y[p * m + i];
      for (int i = lane; i < k; i += 64) {
        LDS(Z_ + i) = a.z[p * k + i];
        LDS(S_ + i) = a.s[p * k + i];
      }
      first = XK_ITER;
    }
    SYNC();
    int kind = first;
    if (a.sing) {
      sing = uni((int)a.sing[(a.flags & F_SHARED) ? 0 : p]) != 0;
    } else {
      sing = false;
      kind = XK_PROBE;
    }
    for (;;) {
      LANE_IDS();
      int fac;
      bool aa;
      if (kind == XK_ITER) {  // residuals (solver.jl:109-118), compute_scaling (:106), exit test (:122)
        MARK_BEGIN("exact pre ITER");
        STAMP(SP_OTHER);
        // (the exits and their order: case MP_ITER of run())
        if (it >= a.maxit && !a.res) break;
        const bool dm = resid_scaling<!(SOCP_KO & 2), !(SOCP_KO & 4096)>(nd, np_, gap, ll, dm_aa);
        STAMP(SP_RESID);
        if (it >= a.maxit) break;
        STAMP(SP_VOP);
        if (dm) {
          status = ST_DOMAIN;
          break;
        }
        if (nd + np_ + gap < a.tol) {
          status = ST_CONVERGED;
          break;
        }
        // (resid_scaling's G x pass has left this scaling's U in LDS)
        fac = (!(SOCP_KO & (2 | 4 | 16 | 4096)) && fuse_u()) ? FAC_SCALED_U : FAC_SCALED;
        aa = sing;
      } else {
        MARK_BEGIN("exact pre IDENT");
        scaling_identity();
        // (FAC_IDENT_H on a problem's first factorisation only: a probe factors the tiles in place)
        if (kind == XK_INIT) {  // initial point: the KKT system with W = I (solver.jl:68-84)
          for (int j = lane; j < n; j += 64) LDS(RD + j) = -LDS(C_ + j);
          for (int i = lane; i < m; i += 64) LDS(RP + i) = LDS(B_ + i);
          for (int i = lane; i < k; i += 64) {
            LDS(DZ + i) = LDS(H_ + i);
            LDS(DS + i) = 0.0;
          }
          SYNC();
          fac = (h_formed && a.sing) ? FAC_IDENT_H : FAC_IDENT;
          aa = sing;
        } else {  // Problem's `sing` (Socp.jl:49-56): is G'G positive definite?
          fac = h_formed ? FAC_IDENT_H : FAC_IDENT;
          aa = false;
        }
      }
      MARK_BEGIN("exact factor");
      const int fst = factor<OV>(fac, aa);
      MARK_BEGIN("exact post factor");
      if (kind == XK_PROBE) {
        sing = (fst == ST_CHOL_H);
        kind = uni(first);
        continue;
      }
      if (fst) {
        status = fst;
        break;
      }
      // the solves (densesolver.jl:54-90): the initial point's one, or the
      // affine and the combined one of an iteration
      int ret = kind == XK_INIT ? RET_INIT : RET_AFFINE;
      bool stop = false;
      for (;;) {
        MARK_BEGIN("case MP_SOLVE_HEAD");
        STAMP(SP_OTHER);
        solve_head();
        STAMP(SP_VOP);
        MARK_BEGIN("case MP_SOLVE_MAT");
        solve_matrix_part(ret == RET_INIT);
        STAMP(SP_SOLVE);
        MARK_BEGIN("case MP_SOLVE_TAIL");
        int dom = 0;
        const double tstep = solve_tail(ret != RET_INIT, dm_aa, dom);
        STAMP(SP_VOP);
        if (ret == RET_INIT) {  // cone shift (solver.jl:86-104)
          double alphp, alphd;  // max_step(-iz), max_step(iz)
          maxstep_op(RZ, alphp, alphd);
          for (int j = lane; j < n; j += 64) LDS(X_ + j) = LDS(RX + j);
          for (int i = lane; i < m; i += 64) LDS(Y_ + i) = LDS(RY + i);
          for (int i = lane; i < k; i += 64) {
            const double iz = LDS(RZ + i), e = e_of(i);
            LDS(S_ + i) = (fabs(alphp) < a.init_eps) ? -iz : -iz + (1.0 + alphp) * e;
            LDS(Z_ + i) = (fabs(alphd) < a.init_eps) ? iz : iz + (1.0 + alphd) * e;
          }
          SYNC();
          kind = XK_ITER;
          break;
        }
        if (dom) {
          status = ST_DOMAIN;
          stop = true;
          break;
        }
        if (ret == RET_AFFINE) {  // centering + corrector, then the combined solve
          affine_post(tstep, ll);
          STAMP(SP_STEP);
          ret = RET_COMBINED;
          continue;
        }
        // combined direction: step and update (solver.jl:143-150)
        const double stp = tstep * a.step;
        {  // every read first, then the updates (n = 64, m = 16, k = 96)
          constexpr int NS = KP > 64 ? 2 : 1;
          const int ly = lane < MPAD ? lane : 0;
          const double xo = LDS(X_ + lane), rx = LDS(RX + lane), yo = LDS(Y_ + ly), ry = LDS(RY + ly);
          double zo[NS], rz[NS], so[NS], rs[NS];
#pragma unroll
          for (int t = 0; t < NS; ++t) {
            const int i = 64 * t + lane;
            zo[t] = LDS(Z_ + i);
            rz[t] = LDS(RZ + i);
            so[t] = LDS(S_ + i);
            rs[t] = LDS(RS + i);
          }
          if (lane < n) LDS(X_ + lane) = xo + rx * stp;
          if (lane < m) LDS(Y_ + lane) = yo + ry * stp;
#pragma unroll
          for (int t = 0; t < NS; ++t) {
            const int i = 64 * t + lane;
            if (i < k) {
              LDS(Z_ + i) = zo[t] + rz[t] * stp;
              LDS(S_ + i) = so[t] + rs[t] * stp;
            }
          }
        }
        SYNC();
        STAMP(SP_STEP);
        iters = ++it;
        break;
      }
      if (stop) break;
    }
    MARK_BEGIN("exact store");
    for (int j = lane; j < n; j += 64) a.x[p * n + j] = LDS(X_ + j);
    for (int i = lane; i < m; i += 64) a.y[p * m + i] = LDS(Y_ + i);
    for (int i = lane; i < k; i += 64) {
      a.z[p * k + i] = LDS(Z_ + i);
      a.s[p * k + i] = LDS(S_ + i);
    }
    if (lane == 0) {
      if (a.res) {
        a.res[3 * p + 0] = nd;
        a.res[3 * p + 1] = np_;
        a.res[3 * p + 2] = gap;
      }
      a.iters[p] = iters;
      a.status[p] = status;
    }
    SYNC();
    STAMP(SP_STORE);
#ifdef SOCP_DIAG
    if (lane == 0) reinterpret_cast<unsigned long long*>(socp_lds + O_STAMPS)[NSTAMP] += iters;
#endif
  }

  __device__ __forceinline__ void flush_stamps() {
#ifdef SOCP_DIAG
    SYNC();
    if (lane == 0 && a.stamps) {
      const unsigned long long* st = reinterpret_cast<const unsigned long long*>(socp_lds + O_STAMPS);
      for (int i = 0; i <= NSTAMP + NSUBSTAMP; ++i) atomicAdd(a.stamps + i, st[i]);
    }
#endif
  }
};

// KM: the kernel's kind, small_km() above
template <int NQ, int NP, int MQ, int KM>
#ifndef SOCP_DEV_MINW
#define SOCP_DEV_MINW 1  // probe builds only: waves per SIMD the register allocation must allow
#endif
__global__ void __launch_bounds__(64, !small_km(KM).plugin && !small_km(KM).xi ? SOCP_DEV_MINW : 1)
    socp_small_kernel(SmallArgs args) {
  constexpr SmallKM K = small_km(KM);
  Small<NQ, NP, MQ, K.xi, slot_pair_kind(K.pair, 0), slot_pair_kind(K.pair, 1), K.qp, K.exact> S(args);
  S.init_tables();
  STAMP_START_S(S);
  while (true) {
    int p = 0;
    if (threadIdx.x == 0) p = atomicAdd(args.counter, 1);
    p = __shfl(p, 0);
    if ((int64_t)p >= args.B) break;
    if constexpr (init_overlap_kernel(NQ, NP, MQ, KM) && !(SOCP_KO & 1)) {
      const bool h_formed = S.template load_problem<true>(p);
      if constexpr (K.exact)
        S.template run_exact<true>(p, h_formed);
      else
        S.template run<0, false, true>(p, h_formed);
    } else {
      S.load_problem(p);
      S.template run<K.plugin, K.di>(p);
    }
  }
  S.flush_stamps();
}

}  // namespace socp
