"""socp_amd — MI355X-native batched dense SOCP solver (host side).

Two layers over libsocp.so (include/socp.h):

* ``batch_solve`` / ``batch_kkt_solve`` / ``generate``: the batched C-ABI
  entry points, taking numpy arrays (host) or torch CUDA tensors (device).
* A mirror of the reference Julia surface for the dense path
  (BenChung/Socp.jl): ``POC``, ``SOC`` (Socp.jl:9-16), ``Problem``
  (Socp.jl:20-60), ``State`` (Socp.jl:62-75), ``DenseSolver`` (the
  KKTSolver plugin, densesolver.jl:1-90, here running on the GPU),
  ``SolverState`` (solver.jl:1-38), ``solve_socp`` (solver.jl:40-153),
  ``compute_scaling`` / ``setup_iter`` / ``solve_kkt`` with the reference's
  argument meaning and error behaviour (PosDefException from cholesky!,
  DomainError from sqrt of a negative number, AssertionError on shapes).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (CHOL_H_FAILED, CHOL_S_FAILED, CONE_POC, CONE_SOC, CONVERGED, DOMAIN_ERROR, DUAL_INFEASIBLE,
                   F_DETECT_INFEASIBLE, F_DEVICE_PTRS, F_EQUILIBRATE, F_EXPLICIT_INVERSE, F_FORCE_LARGE,
                   F_NORMALISE, F_SHARED_MATRICES,
                   F_WARM_START, MAXIT,
                   PRIMAL_INFEASIBLE, Context, SocpError,
                   default_context,
                   default_params)

__all__ = [
    "POC", "SOC", "Problem", "State", "Scaling", "DenseSolver", "HipDenseSolver", "SolverState",
    "solve_socp", "solve_socp_batched", "compute_scaling", "setup_iter", "solve_kkt",
    "PosDefException", "DomainError", "batch_solve", "batch_kkt_solve", "DenseHandle", "Ingest",
    "generate", "pack_csc", "equilibrate", "normalise", "batch_centre", "batch_vjp",
    "Context", "SocpError", "default_context", "cone_arrays",
    "CONVERGED", "MAXIT", "CHOL_H_FAILED", "CHOL_S_FAILED", "DOMAIN_ERROR",
    "PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE",
]

STATUS_NAMES = {CONVERGED: "converged", MAXIT: "maxit", CHOL_H_FAILED: "chol(H) failed",
                CHOL_S_FAILED: "chol(S) failed", DOMAIN_ERROR: "domain error",
                PRIMAL_INFEASIBLE: "primal infeasible", DUAL_INFEASIBLE: "dual infeasible"}


class PosDefException(Exception):
    """Raised where the reference's cholesky! throws (densesolver.jl:47,51)."""


class DomainError(Exception):
    """Raised where the reference's sqrt of a negative number throws."""


# ----------------------------------------------------------------- cones
class POC:
    """Nonnegative orthant cone POC(offs, dim) (Socp.jl:9-12)."""

    kind = CONE_POC

    def __init__(self, offs: int, dim: int):
        self.offs, self.dim = int(offs), int(dim)

    def __repr__(self):
        return f"POC({self.offs},{self.dim})"


class SOC:
    """Second-order cone SOC(offs, dim) (Socp.jl:13-16)."""

    kind = CONE_SOC

    def __init__(self, offs: int, dim: int):
        self.offs, self.dim = int(offs), int(dim)

    def __repr__(self):
        return f"SOC({self.offs},{self.dim})"


def _as_cone_list(cones):
    out = []
    for c in cones:
        if isinstance(c, (POC, SOC)):
            out.append((c.kind, c.offs, c.dim))
        else:
            out.append((int(c[0]), int(c[1]), int(c[2])))
    return out


def cone_arrays(cones):
    cl = _as_cone_list(cones)
    kind = np.array([c[0] for c in cl], dtype=np.int32)
    offs = np.array([c[1] for c in cl], dtype=np.int32)
    dim = np.array([c[2] for c in cl], dtype=np.int32)
    return kind, offs, dim


def slot_plan(cones, k):
    """(rot, kind0, kind1) of socp_debug_slot_plan: how the register-resident
    solver lays a k > 64 cone table over its two 64-lane slots (kinds: 0 mixed,
    1 all SOC, 2 all POC).  Host only."""
    kind, offs, dim = cone_arrays(cones)
    d = _lib.Dims(1, 1, 0, int(k), len(kind))
    rot, k0, k1 = C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.load().socp_debug_slot_plan(C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data,
                                          C.byref(rot), C.byref(k0), C.byref(k1))
    if rc:
        raise SocpError(rc, _lib.load().socp_last_error().decode())
    return rot.value, k0.value, k1.value


def vjp_sum_plan(B, n, m, k):
    """(slabs, slab_problems) of socp_debug_vjp_sum_plan: how ``batch_vjp`` with
    shared_matrices cuts a batch of B problems into runs of consecutive problems
    when it sums dP, dA, dG -- a function of (B, n, m, k) alone.  Host only."""
    d = _lib.Dims(int(B), int(n), int(m), int(k), 0)
    slabs, slab = C.c_int64(), C.c_int64()
    rc = _lib.load().socp_debug_vjp_sum_plan(C.byref(d), C.byref(slabs), C.byref(slab))
    if rc:
        raise SocpError(rc, _lib.load().socp_last_error().decode())
    return slabs.value, slab.value


def exact_fit(cones, n, m, k, *, flags=0):
    """socp_debug_exact_fit: whether a batch_solve of these dims, this cone
    table and these socp_params flags (``_lib.F_*``) runs the solver kernel
    compiled for exactly that launch geometry.  Host only."""
    kind, offs, dim = cone_arrays(cones)
    d = _lib.Dims(1, int(n), int(m), int(k), len(kind))
    ex = C.c_int32()
    rc = _lib.load().socp_debug_exact_fit(C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data,
                                          int(flags), C.byref(ex))
    if rc:
        raise SocpError(rc, _lib.load().socp_last_error().decode())
    return bool(ex.value)


# --------------------------------------------------------------- batched
def _is_torch(a):
    return a is not None and not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _host(a, dtype=np.float64):
    if a is None:
        return None
    return np.ascontiguousarray(a, dtype=dtype)


def _size(a):
    return a.numel() if _is_torch(a) else np.size(a)


def _check_sizes(B, **arrays):
    """Every array must hold exactly its batch-stacked element count (the C ABI
    reads that many elements from each pointer)."""
    if B > _lib.MAX_BATCH:
        raise ValueError(f"batch {B} above 2^31-1")
    for name, (a, want) in arrays.items():
        if a is None:
            continue
        got = _size(a)
        if got != want:
            raise ValueError(f"{name}: {got} elements, expected {want} (batch {B})")


def _check_P(P, G, MB, n):
    """``batch_solve``'s rules for P: on the same side as G; a host array is
    checked for symmetry and returned flat, float64, contiguous."""
    if P is None:
        return None
    if _is_torch(P) != _is_torch(G) or (_is_torch(P) and (
            str(P.dtype) != "torch.float64" or P.device != G.device or not P.is_contiguous())):
        raise ValueError("P must be on the same side as G (host array, or contiguous float64 tensor on G's device)")
    if _is_torch(P):
        return P
    Ph = _host(P).reshape(MB, n, n)
    if not np.allclose(Ph, Ph.transpose(0, 2, 1)):
        raise ValueError("P: every problem's matrix must be symmetric")
    return Ph.reshape(-1)


def batch_solve(cones, n, m, k, c, A, b, G, h, sing=None, *, maxit=40, tol=1e-5, step=0.99,
                sigma_exp=3, init_eps=1e-10, warm=None, ctx=None, res=False, out=None, force_large=False,
                explicit_inverse=False, detect_infeasible=False, shared_matrices=False, P=None,
                equilibrate=False, normalise=False):
    """Solve a batch of independent problems (same dims and cone structure).

    Arrays follow include/socp.h: per-problem column-major A (m x n), G (k x n)
    stacked batch-major, vectors stacked batch-major.  numpy inputs run through
    host staging buffers; torch CUDA tensors are used in place (device mode,
    stream-ordered on the context's stream; call ctx.sync() before reading).
    force_large runs the blocked kernel (socp_large.hip) even where the
    register-resident one applies.  explicit_inverse (SOCP_F_EXPLICIT_INVERSE)
    forms Li = H^-1 as densesolver.jl:48 does -- the reference's op order --
    instead of the Cholesky factor + triangular solves of the m <= 16 shapes.
    detect_infeasible (SOCP_F_DETECT_INFEASIBLE): a problem without a solution
    stops with status PRIMAL_INFEASIBLE (y, z scaled to b'y + h'z = -1: the
    certificate) or DUAL_INFEASIBLE (x, s scaled to c'x = -1) once the
    certificate's residual is below the context's tolerance
    (Context.set_infeasibility_tol, 1e-7) instead of running to maxit; not
    together with explicit_inverse.
    shared_matrices (SOCP_F_SHARED_MATRICES): a parametric batch -- A is ONE
    m x n matrix, G ONE k x n matrix and sing ONE byte (or None), used by every
    problem; c, b, h stay per problem.  The outputs are bitwise those of the
    same call on A, G and sing replicated B times.
    P (socp_batch_solve_qp): a quadratic objective x'Px/2 + c'x -- per problem
    an n x n symmetric positive semidefinite matrix, column-major, stacked
    batch-major (ONE matrix with shared_matrices).  Host arrays are checked
    for symmetry (ValueError); torch tensors are used in place, unchecked.
    The dual residual becomes Px + A'y + G'z + c and H = P + G'W^-2 G; a P
    that makes H indefinite gives that problem CHOL_H_FAILED.  Not together
    with explicit_inverse or detect_infeasible (SOCP_E_UNSUPPORTED).  P=None
    is the plain call.
    equilibrate (SOCP_F_EQUILIBRATE): scale the problem on the device by
    ``equilibrate``'s power-of-two factors, solve, and unscale exactly -- the
    outputs are bitwise those of that three-step pipeline.  tol, init_eps, the
    sing=None probe and res then refer to the scaled problem; the inputs are
    not written.  Not together with warm or detect_infeasible
    (SOCP_E_UNSUPPORTED).
    normalise (SOCP_F_NORMALISE): scale c by one power of two per problem and
    (b, h) by another (``normalise``'s rule: their largest entries come to lie
    in [1, 2)), solve, and unscale exactly -- the outputs are bitwise those of
    that three-step pipeline.  tol, init_eps and res then refer to the
    normalised problem, so the exit test is relative to the sizes of c and of
    (b, h); the inputs are not written.  Not together with detect_infeasible
    (SOCP_E_UNSUPPORTED).
    Returns dict(x, y, z, s, iters, status[, res]).
    """
    L = _lib.load()
    kind, offs, dim = cone_arrays(cones)
    B = _size(c) // n
    if B * n != _size(c):
        raise ValueError(f"c: {_size(c)} elements is not a multiple of n={n}")
    MB = 1 if shared_matrices else B
    _check_sizes(B, A=(A if m else None, MB * m * n), b=(b if m else None, B * m), G=(G, MB * k * n),
                 h=(h, B * k), sing=(sing, MB), P=(P, MB * n * n))
    P = _check_P(P, G, MB, n)
    if warm is not None:
        wx, wy, wz, ws = warm
        _check_sizes(B, warm_x=(wx, B * n), warm_y=(wy if m else None, B * m), warm_z=(wz, B * k),
                     warm_s=(ws, B * k))
    dims = _lib.Dims(B, n, m, k, len(kind))
    ctx = ctx or default_context()
    dev = _is_torch(G)
    flags = F_DEVICE_PTRS if dev else 0
    if warm is not None:
        flags |= F_WARM_START
    if force_large:
        flags |= F_FORCE_LARGE
    if explicit_inverse:
        flags |= F_EXPLICIT_INVERSE
    if detect_infeasible:
        flags |= F_DETECT_INFEASIBLE
    if shared_matrices:
        flags |= F_SHARED_MATRICES
    if equilibrate:
        flags |= F_EQUILIBRATE
    if normalise:
        flags |= F_NORMALISE
    pr = default_params(maxit=maxit, tol=tol, step=step, sigma_exp=sigma_exp, init_eps=init_eps,
                        flags=flags)
    if dev:
        import torch
        devc = G.device
        ctx.bind_torch_stream()  # ordered after torch's producers of the inputs
        if out is None:
            f64 = dict(dtype=torch.float64, device=devc)
            out = dict(x=torch.empty(B * n, **f64), y=torch.empty(max(B * m, 1), **f64),
                       z=torch.empty(B * k, **f64), s=torch.empty(B * k, **f64),
                       iters=torch.empty(B, dtype=torch.int32, device=devc),
                       status=torch.empty(B, dtype=torch.int32, device=devc))
            if res:
                out["res"] = torch.empty(3 * B, **f64)
        if warm is not None:
            for key, v in zip("xyzs", warm):
                if key == "y" and m == 0:
                    continue
                out[key].copy_(v.reshape(-1))
        arrs = dict(c=c, A=A, b=b, G=G, h=h, sing=sing)
    else:
        out = dict(x=np.zeros(B * n), y=np.zeros(max(B * m, 1)), z=np.zeros(B * k),
                   s=np.zeros(B * k), iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
        if res:
            out["res"] = np.zeros(3 * B)
        if warm is not None:
            for key, v in zip("xyzs", warm):
                if key == "y" and m == 0:
                    continue
                out[key][:] = np.asarray(v, dtype=np.float64).reshape(-1)
        arrs = dict(c=_host(c), A=_host(A) if m else None, b=_host(b) if m else None, G=_host(G),
                    h=_host(h), sing=_host(sing, np.uint8) if sing is not None else None)
    p = _lib.ptr
    head = (ctx.handle, dims, p(kind), p(offs), p(dim))
    tail = (p(arrs["c"]), p(arrs["A"] if m else None),
            p(arrs["b"] if m else None), p(arrs["G"]), p(arrs["h"]), p(arrs["sing"]), pr,
            p(out["x"]), p(out["y"] if m else None), p(out["z"]), p(out["s"]), p(out["iters"]),
            p(out["status"]), p(out.get("res")))
    if P is None:
        rc = L.socp_batch_solve_ex(*head, *tail)
    else:
        rc = L.socp_batch_solve_qp(*head, p(P), *tail)
    _lib.check(rc)
    if not dev and m == 0:
        out["y"] = out["y"][:0]
    return out


def equilibrate(cones, n, m, k, A, G, P=None, c=None, b=None, h=None, *, shared_matrices=False, ctx=None):
    """Power-of-two Ruiz equilibration of a batch on the device
    (socp_batch_equilibrate; the rule is in include/socp.h).  A (m x n; None
    when m = 0), G (k x n) and P (n x n, optional) are column-major and stacked
    batch-major, ONE of each with shared_matrices; c, b, h are optional.  numpy
    inputs go through host staging and the call synchronises; torch CUDA
    tensors are used in place, stream-ordered.  The inputs are not written.
    Returns a dict with D (MB x n), E (MB x m), F (MB x k) -- MB is 1 with
    shared_matrices, else the batch -- and the scaled As = E A D, Gs = F G D,
    and Ps = D P D, cs = D c, bs = E b, hs = F h for the inputs given.  The
    batch is taken from c, b or h when one is given, else from G."""
    L = _lib.load()
    kind, offs, dim = cone_arrays(cones)
    given = [(v, q) for v, q in ((c, n), (b, m), (h, k)) if v is not None and q]
    if given:
        B = _size(given[0][0]) // given[0][1]
    elif shared_matrices:
        B = 1
    else:
        B = _size(G) // (k * n)
    MB = 1 if shared_matrices else B
    _check_sizes(B, A=(A if m else None, MB * m * n), G=(G, MB * k * n), P=(P, MB * n * n), c=(c, B * n),
                 b=(b if m else None, B * m), h=(h, B * k))
    dev = _is_torch(G)
    ctx = ctx or default_context()
    ins = dict(P=P, c=c, A=A if m else None, b=b if m else None, G=G, h=h)
    sizes = dict(D=MB * n, E=MB * m, F=MB * k)
    if dev:
        import torch
        ctx.bind_torch_stream()
        new = lambda cnt: torch.empty(max(cnt, 1), dtype=torch.float64, device=G.device)[:cnt]  # noqa: E731
        for key, v in ins.items():
            if v is not None and (not _is_torch(v) or str(v.dtype) != "torch.float64" or v.device != G.device
                                  or not v.is_contiguous()):
                raise ValueError(f"{key} must be a contiguous float64 tensor on G's device")
    else:
        new = lambda cnt: np.zeros(cnt)  # noqa: E731
        ins = {key: _host(v) for key, v in ins.items()}
    out = {key: new(cnt) for key, cnt in sizes.items()}
    for key, v in ins.items():
        if v is not None:
            out[key + "s"] = new(_size(v))
    p = _lib.ptr
    dims = _lib.Dims(B, n, m, k, len(kind))
    flags = (F_DEVICE_PTRS if dev else 0) | (F_SHARED_MATRICES if shared_matrices else 0)

    def po(key):  # NULL for an absent or empty array
        v = out.get(key)
        return p(v) if v is not None and _size(v) else None
    _lib.check(L.socp_batch_equilibrate(
        ctx.handle, dims, p(kind), p(offs), p(dim), p(ins["P"]), p(ins["c"]), p(ins["A"]), p(ins["b"]), p(ins["G"]),
        p(ins["h"]), flags, po("D"), po("E"), po("F"), po("Ps"), po("cs"), po("As"), po("bs"), po("Gs"), po("hs")))
    return out


def normalise(n, m, k, c, b, h, P=None, *, shared_matrices=False, ctx=None):
    """SOCP_F_NORMALISE's rule on the device (socp_batch_normalise; the rule is
    in include/socp.h).  c (n), b (m; None when m = 0) and h (k) are stacked
    batch-major; P (n x n, optional) is column-major, ONE matrix with
    shared_matrices, and then the whole batch takes one pair of exponents.
    numpy inputs go through host staging and the call synchronises; torch CUDA
    tensors are used in place, stream-ordered.  The inputs are not written.
    Returns a dict with expo (2 x batch int32: ec, eb per problem),
    cs = ldexp(c, ec), bs = ldexp(b, eb), hs = ldexp(h, eb) and, with a P,
    Ps = ldexp(P, ec - eb)."""
    L = _lib.load()
    B = _size(c) // n
    if B * n != _size(c):
        raise ValueError(f"c: {_size(c)} elements is not a multiple of n={n}")
    MB = 1 if shared_matrices else B
    _check_sizes(B, b=(b if m else None, B * m), h=(h, B * k), P=(P, MB * n * n))
    dev = _is_torch(c)
    ctx = ctx or default_context()
    ins = dict(P=P, c=c, b=b if m else None, h=h)
    if dev:
        import torch
        ctx.bind_torch_stream()
        new = lambda cnt, dt=torch.float64: torch.empty(max(cnt, 1), dtype=dt, device=c.device)[:cnt]  # noqa: E731
        i32 = torch.int32
        for key, v in ins.items():
            if v is not None and (not _is_torch(v) or str(v.dtype) != "torch.float64" or v.device != c.device
                                  or not v.is_contiguous()):
                raise ValueError(f"{key} must be a contiguous float64 tensor on c's device")
    else:
        new = lambda cnt, dt=np.float64: np.zeros(cnt, dt)  # noqa: E731
        i32 = np.int32
        ins = {key: _host(v) for key, v in ins.items()}
    out = dict(expo=new(2 * B, i32))
    for key, v in ins.items():
        if v is not None:
            out[key + "s"] = new(_size(v))
    p = _lib.ptr
    dims = _lib.Dims(B, n, m, k, 0)
    flags = (F_DEVICE_PTRS if dev else 0) | (F_SHARED_MATRICES if shared_matrices else 0)

    def po(key):  # NULL for an absent or empty array
        v = out.get(key)
        return p(v) if v is not None and _size(v) else None
    _lib.check(L.socp_batch_normalise(ctx.handle, dims, p(ins["P"]), p(ins["c"]), p(ins["b"]), p(ins["h"]), flags,
                                      po("expo"), po("Ps"), po("cs"), po("bs"), po("hs")))
    return out


def batch_kkt_solve(cones, n, m, k, A, G, sing, s, z, dx, dy, dz, ds, *, ctx=None, force_large=False,
                    explicit_inverse=False, shared_matrices=False, P=None):
    """One KKT solve per problem at iterate (s, z): scaling + setup_iter + solve_kkt
    (densesolver.jl:41-90) on the GPU.  Host (numpy) arrays.  shared_matrices: A, G
    and sing are the batch's one (as in ``batch_solve``).  P (``batch_solve``'s:
    n x n per problem, ONE with shared_matrices, checked for symmetry): the
    system's first row is P cx + A'cy + G'cz = dx (socp_batch_kkt_solve_qp); not
    together with explicit_inverse (SOCP_E_UNSUPPORTED).
    Returns dict(cx,cy,cz,cs,status)."""
    L = _lib.load()
    kind, offs, dim = cone_arrays(cones)
    B = np.size(s) // k
    if B * k != np.size(s):
        raise ValueError(f"s: {np.size(s)} elements is not a multiple of k={k}")
    MB = 1 if shared_matrices else B
    _check_sizes(B, A=(A if m else None, MB * m * n), G=(G, MB * k * n), sing=(sing, MB), z=(z, B * k),
                 dx=(dx, B * n), dy=(dy if m else None, B * m), dz=(dz, B * k), ds=(ds, B * k),
                 P=(P, MB * n * n))
    P = _check_P(P, G, MB, n)
    dims = _lib.Dims(B, n, m, k, len(kind))
    ctx = ctx or default_context()
    cx, cy, cz, cs = np.zeros(B * n), np.zeros(max(B * m, 1)), np.zeros(B * k), np.zeros(B * k)
    st = np.zeros(B, np.int32)
    p = _lib.ptr
    sg = None if sing is None else _host(sing, np.uint8)
    tail = (p(_host(A) if m else None), p(_host(G)), p(sg), p(_host(s)), p(_host(z)),
            p(_host(dx)), p(_host(dy) if m else None), p(_host(dz)), p(_host(ds)),
            p(cx), p(cy if m else None), p(cz), p(cs), p(st),
            (F_FORCE_LARGE if force_large else 0)
            | (F_EXPLICIT_INVERSE if explicit_inverse else 0)
            | (F_SHARED_MATRICES if shared_matrices else 0))
    if P is None:
        rc = L.socp_batch_kkt_solve(ctx.handle, dims, p(kind), p(offs), p(dim), *tail)
    else:
        rc = L.socp_batch_kkt_solve_qp(ctx.handle, dims, p(kind), p(offs), p(dim), p(P), *tail)
    _lib.check(rc)
    return dict(cx=cx, cy=cy[:B * m], cz=cz, cs=cs, status=st)


def _vjp_flags(dev, force_large, shared_matrices, explicit_inverse):
    return ((F_DEVICE_PTRS if dev else 0) | (F_FORCE_LARGE if force_large else 0)
            | (F_SHARED_MATRICES if shared_matrices else 0) | (F_EXPLICIT_INVERSE if explicit_inverse else 0))


def _same_side(dev, G, **arrays):
    """With torch inputs every array must be a contiguous tensor on G's device
    (the library reads and writes them in place); with numpy inputs, none."""
    for name, (a, dtype) in arrays.items():
        if a is None:
            continue
        if not dev:
            if _is_torch(a):
                raise ValueError(f"{name} must be a host array, as G is")
        elif not _is_torch(a) or str(a.dtype) != dtype or a.device != G.device or not a.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on G's device")


def batch_centre(cones, n, m, k, c, A, b, G, h, sing, x, y, z, s, *, steps=4, P=None, ctx=None, res=False,
                 force_large=False, shared_matrices=False, explicit_inverse=False):
    """Centre an iterate (socp_batch_centre): `steps` (0..16) pure Newton steps
    towards s o z = mu e at the iterate's own mu = s'z / deg, each one fused
    KKT solve and a full step, halved while it would leave the cone (the last
    step is refined by a second solve, so that the point returned satisfies the
    linear equations to rounding).  The
    gradient of a solve (``batch_vjp``) is exact only at such a point.

    The problem data are ``batch_solve``'s (P optional; ONE P, A, G and sing
    byte with shared_matrices).  numpy inputs go through host staging, the
    iterate is copied and the call synchronises; torch CUDA tensors are used in
    place -- x, y, z, s are overwritten -- stream-ordered on torch's current
    stream.  explicit_inverse is refused (SOCP_E_UNSUPPORTED).
    Returns dict(x, y, z, s, status[, res]): status 0, or what stopped the
    problem at its last good iterate (a KKT status, or DOMAIN_ERROR when no
    step length is found); res holds, per problem, |rd|, |rp|, z's and the
    off-centre measure |lam o lam - mu e| / mu at the returned point."""
    L = _lib.load()
    kind, offs, dim = cone_arrays(cones)
    B = _size(x) // n
    if B * n != _size(x):
        raise ValueError(f"x: {_size(x)} elements is not a multiple of n={n}")
    MB = 1 if shared_matrices else B
    _check_sizes(B, c=(c, B * n), A=(A if m else None, MB * m * n), b=(b if m else None, B * m), G=(G, MB * k * n),
                 h=(h, B * k), sing=(sing, MB), P=(P, MB * n * n), y=(y if m else None, B * m), z=(z, B * k),
                 s=(s, B * k))
    P = _check_P(P, G, MB, n)
    dev = _is_torch(G)
    f64 = "torch.float64"
    _same_side(dev, G, c=(c, f64), A=(A if m else None, f64), b=(b if m else None, f64), h=(h, f64),
               sing=(sing, "torch.uint8"), x=(x, f64), y=(y if m else None, f64), z=(z, f64), s=(s, f64))
    ctx = ctx or default_context()
    if dev:
        import torch
        ctx.bind_torch_stream()
        out = dict(x=x, y=y, z=z, s=s, status=torch.empty(B, dtype=torch.int32, device=G.device))
        if res:
            out["res"] = torch.empty(4 * B, dtype=torch.float64, device=G.device)
        ins = dict(c=c, A=A, b=b, G=G, h=h, sing=sing)
    else:
        out = dict(x=np.array(x, np.float64).reshape(-1), y=np.array(y if m else [], np.float64).reshape(-1),
                   z=np.array(z, np.float64).reshape(-1), s=np.array(s, np.float64).reshape(-1),
                   status=np.zeros(B, np.int32))
        if res:
            out["res"] = np.zeros(4 * B)
        ins = dict(c=_host(c), A=_host(A), b=_host(b), G=_host(G), h=_host(h),
                   sing=None if sing is None else _host(sing, np.uint8))
    p = _lib.ptr
    _lib.check(L.socp_batch_centre(
        ctx.handle, _lib.Dims(B, n, m, k, len(kind)), p(kind), p(offs), p(dim), p(P), p(ins["c"]),
        p(ins["A"] if m else None), p(ins["b"] if m else None), p(ins["G"]), p(ins["h"]), p(ins["sing"]), int(steps),
        _vjp_flags(dev, force_large, shared_matrices, explicit_inverse), p(out["x"]), p(out["y"] if m else None),
        p(out["z"]), p(out["s"]), p(out["status"]), p(out.get("res"))))
    return out


VJP_OUTPUTS = ("dc", "db", "dh", "dP", "dA", "dG", "ux", "uy", "uz")


def batch_vjp(cones, n, m, k, A, G, sing, x, y, z, s, gx=None, gy=None, gz=None, gs=None, *, P=None, skip=None,
              want=None, out=None, centre_steps=0, c=None, b=None, h=None, ctx=None, force_large=False,
              shared_matrices=False, explicit_inverse=False):
    """The gradient of a solve at the point (x, y, z, s) (socp_batch_vjp): given
    the upstream gradients gx, gy, gz, gs = dL/d(x, y, z, s) (None: zero), solve
    the block system of ``batch_kkt_solve`` at (s, z) for the right-hand side
    (gx - G'gs, gy, gz, 0), call the solution (ux, uy, uz, .), set
    w = uz + gs, and return

        dc = -ux    db = uy    dh = w
        dP = -(ux x' + x ux')/2    dA = -(y ux' + uy x')    dG = -(z ux' + w x')

    in the library's layout (column-major matrices, stacked batch-major).  This
    is the derivative of the solution map at a point of the central path; a
    solver's returned iterate is not one, so centre it first -- ``batch_centre``,
    or centre_steps > 0 here, which needs c, b, h, centres a copy and returns
    that point as x, y, z, s (a problem the centring stops is masked).
    want: the outputs to compute, from VJP_OUTPUTS; None is all of them, without
    dP, dA, dG when shared_matrices.  skip: int32 per problem;
    a problem with skip != 0, or whose KKT solve fails, gets zeros in every
    output and that value in status.  On `sing` problems gy must be zero.
    With shared_matrices, dP, dA and dG in `want` are the gradients of the
    batch's ONE P, A and G (socp_batch_vjp_sum): ONE matrix each, of n*n, m*n
    and k*n elements, the sum of the formulas above over the problems with
    status 0 -- deterministic, the same bits on every run and with numpy or
    torch inputs; dP is symmetric in bits.  The per-problem outputs are those
    of the call without the three.
    out: a dict of the caller's own arrays for outputs of `want` (exact size, on
    G's side); the others are allocated.
    numpy arrays go through host staging; torch CUDA tensors are used in place,
    stream-ordered.  Returns a dict of the outputs asked for plus status."""
    L = _lib.load()
    kind, offs, dim = cone_arrays(cones)
    B = _size(x) // n
    if B * n != _size(x):
        raise ValueError(f"x: {_size(x)} elements is not a multiple of n={n}")
    MB = 1 if shared_matrices else B
    if want is None:
        want = [w for w in VJP_OUTPUTS if not (shared_matrices and w in ("dP", "dA", "dG"))]
    for w in want:
        if w not in VJP_OUTPUTS:
            raise ValueError(f"want: unknown output {w!r}")
    _check_sizes(B, A=(A if m else None, MB * m * n), G=(G, MB * k * n), sing=(sing, MB), P=(P, MB * n * n),
                 y=(y if m else None, B * m), z=(z, B * k), s=(s, B * k), gx=(gx, B * n),
                 gy=(gy if m else None, B * m), gz=(gz, B * k), gs=(gs, B * k), skip=(skip, B))
    P = _check_P(P, G, MB, n)
    dev = _is_torch(G)
    f64 = "torch.float64"
    _same_side(dev, G, A=(A if m else None, f64), sing=(sing, "torch.uint8"), x=(x, f64), y=(y if m else None, f64),
               z=(z, f64), s=(s, f64), gx=(gx, f64), gy=(gy if m else None, f64), gz=(gz, f64), gs=(gs, f64),
               skip=(skip, "torch.int32"))
    if centre_steps and (c is None or h is None or (m and b is None)):
        raise ValueError("centre_steps > 0 needs c, b and h")
    sizes = dict(dc=B * n, db=B * m, dh=B * k, dP=MB * n * n, dA=MB * m * n, dG=MB * k * n, ux=B * n, uy=B * m,
                 uz=B * k)
    # the gradients of shared matrices are sums over the batch: the entry that forms them
    sums = shared_matrices and any(w in want for w in ("dP", "dA", "dG"))
    for w in want:
        mine = None if out is None else out.get(w)
        if mine is not None:
            _check_sizes(B, **{w: (mine, sizes[w])})
            _same_side(dev, G, **{w: (mine, f64)})
            if not dev and not (isinstance(mine, np.ndarray) and mine.dtype == np.float64
                                and mine.flags.c_contiguous):
                raise ValueError(f"out[{w!r}] must be a contiguous float64 array")
    ctx = ctx or default_context()
    given, out = out, {}
    if centre_steps:
        pt = [None if v is None else (v.clone() if dev else v) for v in (x, y if m else None, z, s)]
        cen = batch_centre(cones, n, m, k, c, A, b, G, h, sing, *pt, steps=centre_steps, P=P, ctx=ctx,
                           force_large=force_large, shared_matrices=shared_matrices)
        x, y, z, s = cen["x"], cen["y"], cen["z"], cen["s"]
        out.update(x=x, y=y, z=z, s=s)
        if skip is None:
            skip = cen["status"]
        elif dev:
            import torch
            skip = torch.where(skip != 0, skip, cen["status"])
        else:
            skip = np.where(np.asarray(skip) != 0, skip, cen["status"]).astype(np.int32)
    if dev:
        import torch
        ctx.bind_torch_stream()
        new = lambda cnt, dt=torch.float64: torch.empty(cnt, dtype=dt, device=G.device)  # noqa: E731
        status = new(B, torch.int32)
        arg = lambda v, dt=None: v  # noqa: E731
    else:
        new = lambda cnt: np.zeros(cnt)  # noqa: E731
        status = np.zeros(B, np.int32)
        arg = lambda v, dt=np.float64: None if v is None else _host(v, dt)  # noqa: E731
    for w in want:
        mine = None if given is None else given.get(w)
        out[w] = new(sizes[w]) if mine is None else mine
    out["status"] = status
    p = _lib.ptr

    def po(key):  # NULL for an output not asked for, or empty (m = 0)
        v = out.get(key)
        return p(v) if v is not None and key in want and _size(v) else None
    ins = [arg(v) for v in (A if m else None, G)] + [arg(sing, np.uint8)] + [
        arg(v) for v in (x, y if m else None, z, s, gx, gy if m else None, gz, gs)] + [arg(skip, np.int32)]
    _lib.check((L.socp_batch_vjp_sum if sums else L.socp_batch_vjp)(
        ctx.handle, _lib.Dims(B, n, m, k, len(kind)), p(kind), p(offs), p(dim), p(P), *[p(v) for v in ins],
        _vjp_flags(dev, force_large, shared_matrices, explicit_inverse),
        *[po(key) for key in VJP_OUTPUTS], p(status)))
    return out


class DenseHandle:
    """A batch of DenseSolver objects on the device (socp_dense_*): the
    reference's plugin split (densesolver.jl) -- construction keeps A and G
    resident (:19-38), ``setup_iter(s, z)`` computes the NT scaling and the
    factorisation (:41-52) into one record per problem, ``solve_kkt`` solves one
    right-hand side against it (:54-90) as often as called.

    numpy inputs: every call copies its vectors host-to-device (2k doubles per
    problem for setup_iter, n+m+2k for solve_kkt; ``h2d_bytes`` reports the last
    call's count).  torch CUDA inputs (A, G given as tensors): every later
    argument must be a device tensor too; calls are stream-ordered on torch's
    current stream.  Results are bitwise those of ``batch_kkt_solve``.

    shared_matrices=True (SOCP_F_SHARED_MATRICES): A, G and sing are ONE m x n
    matrix, ONE k x n matrix and ONE byte for all ``batch`` problems (``batch``
    must then be given: G no longer tells it); the handle keeps that one copy,
    the factor records stay per problem, and every result is bitwise that of
    the handle built on the replicated matrices.

    P (``batch_solve``'s; on the same side as G, ONE matrix with
    shared_matrices): the handle keeps it beside A and G (socp_dense_create_qp)
    and setup_iter factors H = P + G'W^-2 G (+A'A); results are bitwise those
    of ``batch_kkt_solve(P=...)``.  Not together with explicit_inverse."""

    _pfx = "socp_dense"

    def _fn(self, name):
        return getattr(_lib.load(), f"{self._pfx}_{name}")

    def __init__(self, cones, n, m, k, A, G, sing=None, *, ctx=None, force_large=False, explicit_inverse=False,
                 shared_matrices=False, batch=None, P=None):
        self.cones, self.n, self.m, self.k = cones, n, m, k
        self.kind, self.offs, self.dim = cone_arrays(cones)
        if shared_matrices:
            if batch is None:
                raise ValueError("shared_matrices=True needs batch= (the number of problems)")
            B = int(batch)
            _check_sizes(B, A=(A if m else None, m * n), G=(G, k * n), sing=(sing, 1))
        else:
            B = _size(G) // (k * n)
            if B * k * n != _size(G):
                raise ValueError(f"G: {_size(G)} elements is not a multiple of k*n={k * n}")
            if batch is not None and int(batch) != B:
                raise ValueError(f"batch={batch}, but G holds {B} problems")
            _check_sizes(B, A=(A if m else None, B * m * n), sing=(sing, B))
        self.B = B
        self.shared_matrices = bool(shared_matrices)
        MB = 1 if shared_matrices else B
        _check_sizes(B, P=(P, MB * n * n))
        P = _check_P(P, G, MB, n)
        self.ctx = ctx or default_context()
        self.dev = _is_torch(G)
        flags = ((F_DEVICE_PTRS if self.dev else 0) | (F_FORCE_LARGE if force_large else 0)
                 | (F_EXPLICIT_INVERSE if explicit_inverse else 0)
                 | (F_SHARED_MATRICES if shared_matrices else 0))
        if self.dev:
            self.ctx.bind_torch_stream()
            arrs = (A if m else None, G, sing)
        else:
            arrs = (_host(A) if m else None, _host(G), None if sing is None else _host(sing, np.uint8))
        h = C.c_void_p()
        dims = _lib.Dims(B, n, m, k, len(self.kind))
        p = _lib.ptr
        if P is None:
            _lib.check(self._fn("create")(self.ctx.handle, dims, p(self.kind), p(self.offs), p(self.dim),
                                           p(arrs[0]), p(arrs[1]), p(arrs[2]), flags, C.byref(h)))
        else:  # (DenseHandle only: SqrHandle's constructor takes no P)
            _lib.check(self._fn("create_qp")(self.ctx.handle, dims, p(self.kind), p(self.offs), p(self.dim),
                                              p(P), p(arrs[0]), p(arrs[1]), p(arrs[2]), flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _arg(self, a, dtype=np.float64):
        if self.dev:
            if not _is_torch(a):
                raise TypeError("a device handle takes torch CUDA tensors")
            return a
        return _host(a, dtype)

    def setup_iter(self, s, z, status=None):
        """Scaling + factorisation at (s, z); returns the per-problem status
        (0, CHOL_H_FAILED, CHOL_S_FAILED, DOMAIN_ERROR)."""
        B, k = self.B, self.k
        _check_sizes(B, s=(s, B * k), z=(z, B * k))
        if status is None:
            if self.dev:
                import torch
                status = torch.empty(B, dtype=torch.int32, device=s.device)
            else:
                status = np.zeros(B, np.int32)
        if self.dev:
            self.ctx.bind_torch_stream()
        p = _lib.ptr
        _lib.check(self._fn("setup_iter")(self.handle, p(self._arg(s)), p(self._arg(z)), p(status)))
        return status

    def solve_kkt(self, dx, dy, dz, ds, out=None):
        """One KKT solve per problem against the last setup_iter; returns
        dict(cx, cy, cz, cs, status) (``out`` may supply the arrays)."""
        B, n, m, k = self.B, self.n, self.m, self.k
        _check_sizes(B, dx=(dx, B * n), dy=(dy if m else None, B * m), dz=(dz, B * k), ds=(ds, B * k))
        if out is None:
            if self.dev:
                import torch
                f64 = dict(dtype=torch.float64, device=dz.device)
                out = dict(cx=torch.empty(B * n, **f64), cy=torch.empty(max(B * m, 1), **f64),
                           cz=torch.empty(B * k, **f64), cs=torch.empty(B * k, **f64),
                           status=torch.empty(B, dtype=torch.int32, device=dz.device))
            else:
                out = dict(cx=np.zeros(B * n), cy=np.zeros(max(B * m, 1)), cz=np.zeros(B * k),
                           cs=np.zeros(B * k), status=np.zeros(B, np.int32))
        if self.dev:
            self.ctx.bind_torch_stream()
        p = _lib.ptr
        _lib.check(self._fn("solve_kkt")(
            self.handle, p(self._arg(dx)), p(self._arg(dy) if m else None), p(self._arg(dz)),
            p(self._arg(ds)), p(out["cx"]), p(out["cy"] if m else None), p(out["cz"]), p(out["cs"]),
            p(out["status"])))
        if m == 0 or _size(out["cy"]) != B * m:
            out["cy"] = out["cy"][:B * m]
        return out

    @property
    def h2d_bytes(self) -> int:
        """Host-to-device bytes moved by the last call (socp_dense_h2d_bytes)."""
        v = C.c_int64()
        _lib.check(self._fn("h2d_bytes")(self.handle, C.byref(v)))
        return int(v.value)

    @property
    def record_bytes(self) -> int:
        """Device bytes of one problem's factor record."""
        return int(self._fn("record_bytes")(self.handle))


class SqrHandle(DenseHandle):
    """A batch of SparseSolver objects with SqrScaling on the device
    (socp_sqr_*, the reference's rank-update path: spsolver.jl,
    sqrscalings.jl).  ``setup_iter(s, z)`` computes W^-2 = D + uu' - vv',
    factors G'DG (+A'A), applies one rank-1 update (G'u) and one downdate (G'v)
    per SOC cone and factors S; ``solve_kkt`` solves by triangular solves.
    Same call conventions as DenseHandle; n, m <= 1024, k <= 4096 (one
    wavefront per problem up to n, m = 64, one workgroup above)."""

    _pfx = "socp_sqr"

    def __init__(self, cones, n, m, k, A, G, sing=None, *, ctx=None, shared_matrices=False, batch=None):
        super().__init__(cones, n, m, k, A, G, sing, ctx=ctx, shared_matrices=shared_matrices, batch=batch)

    def factor(self, problem: int):
        """The factor L of H after modify_factors! for one problem (n x n lower
        triangular numpy array; L L' = G'W^-2 G (+A'A)) -- the Gfact of spsolver.jl:13."""
        out = np.zeros(self.n * self.n)
        _lib.check(self._fn("factor")(self.handle, int(problem), _lib.ptr(out)))
        return out.reshape(self.n, self.n, order="F")

    def solve_socp(self, c, b, h, *, maxit=40, tol=1e-5, step=0.99, sigma_exp=3, init_eps=1e-10, res=True,
                   detect_infeasible=False):
        """solve_socp(prob, SolverState(prob, SparseSolver(prob))) (solver.jl:40-153)
        for every problem of the batch, on this plugin (socp_sqr_solve_socp):
        the reference's own tested path, batched.  Returns dict(x, y, z, s,
        iters, status[, res]) like ``batch_solve``; numpy or torch as the handle.
        detect_infeasible as in ``batch_solve``."""
        B, n, m, k = self.B, self.n, self.m, self.k
        _check_sizes(B, c=(c, B * n), b=(b if m else None, B * m), h=(h, B * k))
        if self.dev:
            import torch
            dv = c.device
            f64 = dict(dtype=torch.float64, device=dv)
            out = dict(x=torch.empty(B * n, **f64), y=torch.empty(max(B * m, 1), **f64),
                       z=torch.empty(B * k, **f64), s=torch.empty(B * k, **f64),
                       iters=torch.empty(B, dtype=torch.int32, device=dv),
                       status=torch.empty(B, dtype=torch.int32, device=dv))
            if res:
                out["res"] = torch.empty(3 * B, **f64)
            self.ctx.bind_torch_stream()
        else:
            out = dict(x=np.zeros(B * n), y=np.zeros(max(B * m, 1)), z=np.zeros(B * k), s=np.zeros(B * k),
                       iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
            if res:
                out["res"] = np.zeros(3 * B)
        P = _lib.default_params(maxit=maxit, tol=tol, step=step, sigma_exp=sigma_exp, init_eps=init_eps,
                                flags=F_DETECT_INFEASIBLE if detect_infeasible else 0)
        p = _lib.ptr
        _lib.check(self._fn("solve_socp")(self.handle, p(self._arg(c)), p(self._arg(b)) if m else None,
                                           p(self._arg(h)), C.byref(P), p(out["x"]), p(out["y"]) if m else None,
                                           p(out["z"]), p(out["s"]), p(out["iters"]), p(out["status"]),
                                           p(out.get("res"))))
        out["y"] = out["y"][:B * m]
        return out

    def scaling(self):
        """dict(l, wbs, mu) of the last setup_iter for every problem (host arrays
        B x k, B x k, B x ncones): the SqrScaling fields the driver loop reads."""
        B, k, nc = self.B, self.k, len(self.kind)
        l, wbs, mu = np.zeros(B * k), np.zeros(B * k), np.zeros(B * nc)
        _lib.check(self._fn("scaling")(self.handle, _lib.ptr(l), _lib.ptr(wbs), _lib.ptr(mu)))
        return dict(l=l.reshape(B, k), wbs=wbs.reshape(B, k), mu=mu.reshape(B, nc))


def sqr_supported(n, m, k, ncones) -> bool:
    """Whether the rank-update plugin takes these dims (socp_sqr_supported)."""
    return bool(_lib.load().socp_sqr_supported(_lib.Dims(1, n, m, k, ncones)))


def _csc_arrays(mats, rows, cols, index_base):
    """(nz_offs, colptr, rowval, nzval) host arrays of a list of scipy.sparse
    matrices in canonical CSC form (sorted, duplicates summed)."""
    csc = []
    for M in mats:
        M = M.tocsc(copy=True)
        M.sum_duplicates()
        if M.shape != (rows, cols):
            raise ValueError(f"matrix shape {M.shape}, expected {(rows, cols)}")
        csc.append(M)
    nz = np.cumsum(np.array([0] + [M.nnz for M in csc], dtype=np.int64))
    colptr = (np.concatenate([M.indptr.astype(np.int64) + index_base for M in csc]) if csc
              else np.zeros(1, np.int64))
    rowval = (np.concatenate([M.indices.astype(np.int64) + index_base for M in csc]) if nz[-1]
              else np.zeros(1, np.int64))
    nzval = np.concatenate([M.data.astype(np.float64) for M in csc]) if nz[-1] else np.zeros(1)
    return nz, colptr, rowval, nzval


class Ingest:
    """Pipelined host ingest (socp_ingest_*): host batches through two slots of
    pinned staging, batch i+1's host-to-device copy (and CSC packing) overlapping
    batch i's solve.  ``submit`` / ``submit_csc`` return a ticket, ``wait``
    returns the batch_solve dict; at most two tickets are outstanding.
    ``next_inputs()`` gives numpy views of the next slot's pinned input arrays
    (a producer filling them in place saves the host copy).

    shared_matrices=True (SOCP_F_SHARED_MATRICES): the slots stage no A, G or
    sing; ``set_matrices(A, G, sing=None)`` gives the one A, G and sing byte of
    every later batch (only with no ticket outstanding; again between batches
    as needed), ``submit(c, None, b, None, h)`` carries the vectors alone and
    ``next_inputs()`` has no A, G, sing.

    P (``batch_solve``'s quadratic objective; host arrays, checked for
    symmetry): ``submit(..., P=P)`` runs socp_ingest_submit_qp, bitwise
    ``batch_solve(P=P)``; the slots' room for P is allocated by the first call
    that brings one (``next_inputs(P=True)`` adds the next slot's pinned P
    block to the dict).  A shared ingest takes its one P through
    ``set_matrices(A, G, sing, P=P)`` and ``submit(..., qp=True)`` solves with
    it.  Not together with explicit_inverse or detect_infeasible
    (SOCP_E_UNSUPPORTED, and the slot stays free).  A submit without P is the
    linear solve."""

    def __init__(self, cones, n, m, k, max_batch, *, ctx=None, force_large=False, shared_matrices=False):
        L = _lib.load()
        self.cones, self.n, self.m, self.k, self.max_batch = cones, n, m, k, int(max_batch)
        self.kind, self.offs, self.dim = cone_arrays(cones)
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        dims = _lib.Dims(self.max_batch, n, m, k, len(self.kind))
        p = _lib.ptr
        _lib.check(L.socp_ingest_create(self.ctx.handle, dims, p(self.kind), p(self.offs), p(self.dim),
                                        (F_FORCE_LARGE if force_large else 0)
                                        | (F_SHARED_MATRICES if shared_matrices else 0), C.byref(h)))
        self.handle = h
        self.shared_matrices = bool(shared_matrices)
        self._batch = {}

    def set_matrices(self, A, G, sing=None, P=None):
        """The one A (m x n), G (k x n), column-major, and sing byte (None: the
        device probe) of every later batch of a shared ingest
        (socp_ingest_set_matrices): host arrays, copied synchronously.  P: their
        one n x n P (socp_ingest_set_matrices_qp); without it any earlier P is cleared."""
        n, m, k = self.n, self.m, self.k
        _check_sizes(1, A=(A if m else None, m * n), G=(G, k * n), sing=(sing, 1), P=(P, n * n))
        p = _lib.ptr
        tail = (p(_host(A) if m else None), p(_host(G)), p(None if sing is None else _host(sing, np.uint8)))
        if P is None:
            _lib.check(_lib.load().socp_ingest_set_matrices(self.handle, *tail))
        else:
            _lib.check(_lib.load().socp_ingest_set_matrices_qp(self.handle, p(_check_P(P, _host(G), 1, n)), *tail))

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().socp_ingest_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next_inputs(self, P=False):
        """numpy views of the next slot's pinned input arrays; P=True adds the
        slot's pinned P block (socp_ingest_next_P; not on a shared ingest)."""
        ptrs = [C.c_void_p() for _ in range(6)]
        _lib.check(_lib.load().socp_ingest_next_inputs(self.handle, *[C.byref(q) for q in ptrs]))
        B, n, m, k = self.max_batch, self.n, self.m, self.k
        out = {}
        for key, q, cnt, ct in zip(("c", "A", "b", "G", "h", "sing"), ptrs,
                                   (B * n, B * m * n, B * m, B * k * n, B * k, B),
                                   (C.c_double,) * 5 + (C.c_uint8,)):
            if self.shared_matrices and key in ("A", "G", "sing"):
                continue  # NULL: a shared ingest stages none of them
            out[key] = np.ctypeslib.as_array(C.cast(q, C.POINTER(ct)), shape=(max(cnt, 1),))[:cnt]
        if P:
            q = C.c_void_p()
            _lib.check(_lib.load().socp_ingest_next_P(self.handle, C.byref(q)))
            out["P"] = np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_double)), shape=(B * n * n,))
        return out

    def _params(self, maxit, tol, step, sigma_exp, init_eps, detect_infeasible=False, explicit_inverse=False):
        return default_params(maxit=maxit, tol=tol, step=step, sigma_exp=sigma_exp, init_eps=init_eps,
                              flags=(F_DETECT_INFEASIBLE if detect_infeasible else 0)
                              | (F_EXPLICIT_INVERSE if explicit_inverse else 0))

    def submit(self, c, A, b, G, h, sing=None, *, maxit=40, tol=1e-5, step=0.99, sigma_exp=3, init_eps=1e-10,
               detect_infeasible=False, explicit_inverse=False, P=None, qp=False):
        """P: the batch's matrices (a per-problem ingest); qp=True: a shared
        ingest's solve with the P of ``set_matrices(P=...)``."""
        n, m, k = self.n, self.m, self.k
        B = np.size(c) // n
        _check_sizes(B, c=(c, B * n), A=(A if m else None, B * m * n), b=(b if m else None, B * m),
                     G=(G, B * k * n), h=(h, B * k), sing=(sing, B), P=(P, B * n * n))
        t = C.c_int64()
        pr = self._params(maxit, tol, step, sigma_exp, init_eps, detect_infeasible, explicit_inverse)
        p = _lib.ptr
        arr = [_host(c), _host(A) if m and A is not None else None, _host(b) if m else None, _host(G), _host(h),
               None if sing is None else _host(sing, np.uint8)]
        if P is not None or qp:
            Ph = None if P is None else _check_P(P, arr[0], B, n)
            _lib.check(_lib.load().socp_ingest_submit_qp(self.handle, B, p(Ph), *[p(a) for a in arr], pr,
                                                         C.byref(t)))
        else:
            _lib.check(_lib.load().socp_ingest_submit(self.handle, B, *[p(a) for a in arr], pr, C.byref(t)))
        self._batch[t.value] = B
        return t.value

    def submit_csc(self, c, b, h, sing, A_mats, G_mats, *, index_base=1, maxit=40, tol=1e-5, step=0.99,
                   sigma_exp=3, init_eps=1e-10, detect_infeasible=False):
        """A_mats, G_mats: lists of scipy.sparse matrices (m x n, k x n), or
        tuples (nz_offs, colptr, rowval, nzval) of host arrays."""
        n, m, k = self.n, self.m, self.k
        B = np.size(c) // n
        _check_sizes(B, c=(c, B * n), b=(b if m else None, B * m), h=(h, B * k), sing=(sing, B))
        Acsc = (A_mats if isinstance(A_mats, tuple) else _csc_arrays(A_mats, m, n, index_base)) if m else None
        Gcsc = G_mats if isinstance(G_mats, tuple) else _csc_arrays(G_mats, k, n, index_base)
        Acsc = [np.ascontiguousarray(a) for a in Acsc] if Acsc is not None else [None] * 4
        Gcsc = [np.ascontiguousarray(a) for a in Gcsc]
        t = C.c_int64()
        P = self._params(maxit, tol, step, sigma_exp, init_eps, detect_infeasible)
        p = _lib.ptr
        _lib.check(_lib.load().socp_ingest_submit_csc(
            self.handle, B, p(_host(c)), p(_host(b) if m else None), p(_host(h)),
            p(None if sing is None else _host(sing, np.uint8)), *[p(a) for a in Acsc], *[p(a) for a in Gcsc],
            index_base, P, C.byref(t)))
        self._batch[t.value] = B
        return t.value

    def wait(self, ticket, res=False):
        B = self._batch.pop(ticket, None)
        if B is None:
            raise ValueError(f"unknown ticket {ticket}")
        n, m, k = self.n, self.m, self.k
        out = dict(x=np.zeros(B * n), y=np.zeros(max(B * m, 1)), z=np.zeros(B * k), s=np.zeros(B * k),
                   iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
        if res:
            out["res"] = np.zeros(3 * B)
        p = _lib.ptr
        _lib.check(_lib.load().socp_ingest_wait(self.handle, ticket, p(out["x"]), p(out["y"] if m else None),
                                                p(out["z"]), p(out["s"]), p(out["iters"]), p(out["status"]),
                                                p(out.get("res"))))
        out["y"] = out["y"][:B * m]
        return out


def generate(cones, B, n, m, k, seed, first_problem=0, *, ctx=None, device=None):
    """Device-side generation of B feasible synthetic problems;
    returns torch CUDA tensors (c, A, b, G, h) in the include/socp.h layout."""
    import torch
    ctx = ctx or default_context()
    dev = device or torch.device("cuda", ctx.device)
    f64 = dict(dtype=torch.float64, device=dev)
    c, A, b = torch.empty(B * n, **f64), torch.empty(max(B * m * n, 1), **f64), torch.empty(max(B * m, 1), **f64)
    G, h = torch.empty(B * k * n, **f64), torch.empty(B * k, **f64)
    kind, offs, dim = cone_arrays(cones)
    dims = _lib.Dims(B, n, m, k, len(kind))
    p = _lib.ptr
    ctx.bind_torch_stream()
    _lib.check(_lib.load().socp_generate(ctx.handle, dims, p(kind), p(offs), p(dim), seed,
                                         first_problem, p(c), p(A), p(b), p(G), p(h)))
    return c, A[:B * m * n], b[:B * m], G, h


def pack_csc(mats, rows=None, cols=None, *, index_base=1, ctx=None, device=None):
    """Ingest: pack sparse matrices in SparseMatrixCSC form --
    the storage of Problem.A / Problem.G (Socp.jl:25,29) -- into the dense
    column-major batch layout on the device (socp_pack_csc).  `mats` is a list
    of scipy.sparse matrices (CSC after conversion), or a tuple of device int64
    tensors (nz_offs, colptr, rowval) plus a float64 nzval tensor with rows, cols
    given.  Returns a flat torch float64 tensor of B*rows*cols."""
    import torch
    ctx = ctx or default_context()
    dev = device or torch.device("cuda", ctx.device)
    if isinstance(mats, tuple):
        nz_offs, colptr, rowval, nzval = mats
        B = nz_offs.numel() - 1
    else:
        # canonical CSC (sorted row indices, duplicates summed in order, as
        # Julia's sparse() stores them); the device kernel also sums unsorted
        # or repeated entries, but only this form is bitwise reproducible
        csc = []
        for m in mats:
            m = m.tocsc(copy=True)
            m.sum_duplicates()
            csc.append(m)
        B = len(csc)
        rows, cols = csc[0].shape if B else (rows or 0, cols or 0)
        for m in csc:
            assert m.shape == (rows, cols)
        nnz = np.array([0] + [m.nnz for m in csc], dtype=np.int64)
        nz = np.cumsum(nnz)
        i64 = dict(dtype=torch.int64, device=dev)
        nz_offs = torch.tensor(nz, **i64)
        colptr = torch.tensor(np.concatenate([m.indptr.astype(np.int64) + index_base for m in csc])
                              if B else np.zeros(0, np.int64), **i64)
        rowval = torch.tensor(np.concatenate([m.indices.astype(np.int64) + index_base for m in csc])
                              if B and nz[-1] else np.zeros(1, np.int64), **i64)
        nzval = torch.tensor(np.concatenate([m.data.astype(np.float64) for m in csc])
                             if B and nz[-1] else np.zeros(1), dtype=torch.float64, device=dev)
    out = torch.empty(max(B * rows * cols, 1), dtype=torch.float64, device=dev)
    p = _lib.ptr
    ctx.bind_torch_stream()
    _lib.check(_lib.load().socp_pack_csc(ctx.handle, B, rows, cols, p(nz_offs), p(colptr), p(rowval),
                                         p(nzval), index_base, p(out)))
    return out[:B * rows * cols]


# ------------------------------------------------- reference-shaped mirror
def _colmajor(M, rows, cols):
    M = np.asarray(M, dtype=np.float64).reshape(rows, cols) if rows * cols else np.zeros((rows, cols))
    return np.ascontiguousarray(M.ravel(order="F"))


class Problem:
    """Problem(c, A, b, G, h, cones) (Socp.jl:40-59).  `sing` is true when
    cholesky(G'G) throws, exactly the reference's rule (Socp.jl:49-56).
    P (optional, n x n symmetric positive semidefinite): the objective is
    x'Px/2 + c'x (``batch_solve``'s P); `sing` never sees it."""

    def __init__(self, c, A, b, G, h, cones, P=None):
        c = np.asarray(c, dtype=np.float64).reshape(-1)
        n = len(c)
        A = np.asarray(A, dtype=np.float64)
        A = A.reshape(-1, n) if A.size else np.zeros((0, n))
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        G = np.asarray(G, dtype=np.float64)
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        m = A.shape[0]
        assert len(b) == m
        assert A.shape[1] == n
        assert G.shape[1] == n
        k = G.shape[0]
        assert len(h) == k
        self.c, self.A, self.b, self.G, self.h = c, A, b, G, h
        if P is not None:
            P = np.asarray(P, dtype=np.float64)
            assert P.shape == (n, n)
        self.P = P
        self.cones = tuple(cones)
        self.n, self.m, self.k = n, m, k
        try:
            np.linalg.cholesky(G.T @ G)
            self.sing = False
        except np.linalg.LinAlgError:
            self.sing = True


class State:
    """State(prob, x, y, z, s) (Socp.jl:62-75)."""

    def __init__(self, prob: Problem, x, y, z, s):
        self.x = np.array(x, dtype=np.float64).reshape(-1)
        self.y = np.array(y, dtype=np.float64).reshape(-1)
        self.z = np.array(z, dtype=np.float64).reshape(-1)
        self.s = np.array(s, dtype=np.float64).reshape(-1)
        assert len(self.x) == prob.n
        assert len(self.y) == prob.m
        assert len(self.z) == prob.k
        assert len(self.s) == prob.k


class Scaling:
    """NT scaling handle (scalings.jl:1-20), the plugin's AbstractScaling.  The
    scaling W, W^-1, lambda itself lives on the device, in the DenseSolver's
    factor record; this object records the (s, z) compute_scaling was given."""

    def __init__(self, prob: Problem):
        self.s = np.zeros(prob.k)
        self.z = np.zeros(prob.k)


def compute_scaling(cones, scaling: Scaling, s, z):
    """compute_scaling(cones, scaling, s, z) (scalings.jl:101-110).  The
    arithmetic runs on the GPU in the next setup_iter (it feeds only that)."""
    scaling.s = np.array(s, dtype=np.float64)
    scaling.z = np.array(z, dtype=np.float64)
    return scaling


class DenseSolver:
    """KKTSolver{Scaling} plugin for the dense path (densesolver.jl:1-90) on
    MI355X: DenseSolver(pr) (:19-38) keeps A and G on the device (a one-problem
    DenseHandle); setup_iter factors into the handle's record, solve_kkt solves
    against it, so only n+m+2k doubles move per solve.  A Problem with a P
    gives the handle that P: the plugin loop then solves the QP's KKT system."""

    scaling_type = Scaling

    def __init__(self, prob: Problem, ctx: Context | None = None):
        self.prob = prob
        self.ctx = ctx
        self.handle = DenseHandle(prob.cones, prob.n, prob.m, prob.k, _colmajor(prob.A, prob.m, prob.n),
                                  _colmajor(prob.G, prob.k, prob.n), np.array([prob.sing], np.uint8),
                                  ctx=ctx, P=None if prob.P is None else _colmajor(prob.P, prob.n, prob.n))


HipDenseSolver = DenseSolver


class SqrScaling(Scaling):
    """SqrScaling (sqrscalings.jl:8-48), the scaling type of SparseSolver: the
    factored W^-2 = D + uu' - vv' is computed on the device by setup_iter; this
    object records (s, z) and, after setup_iter, holds the fields the driver
    loop reads (l, wbs, mu), read back from the device."""

    def __init__(self, prob: Problem):
        super().__init__(prob)
        self.l = np.zeros(prob.k)
        self.wbs = np.zeros(prob.k)
        self.mu = np.zeros(len(prob.cones))


class SparseSolver(DenseSolver):
    """KKTSolver{SqrScaling} plugin (spsolver.jl:1-130) on MI355X: the
    rank-update path -- G'DG factored, one rank-1 update and one downdate per
    SOC cone, triangular solves (a one-problem SqrHandle).  The reference runs
    it through CHOLMOD; here the factor is dense and LDS-resident.  The plugin
    methods are setup_iter / solve_kkt; solve_socp with this plugin runs the
    reference's IPM loop on the device with these same kernels
    (SqrHandle.solve_socp, socp_sqr_solve_socp)."""

    scaling_type = SqrScaling

    def __init__(self, prob: Problem, ctx: Context | None = None):
        if prob.P is not None:
            raise ValueError("P: the rank-update solver takes linear objectives only")
        self.prob = prob
        self.ctx = ctx
        self.handle = SqrHandle(prob.cones, prob.n, prob.m, prob.k, _colmajor(prob.A, prob.m, prob.n),
                                _colmajor(prob.G, prob.k, prob.n), np.array([prob.sing], np.uint8), ctx=ctx)


HipSqrSolver = SparseSolver


def setup_iter(solver: DenseSolver, prob: Problem, state: State, scaling: Scaling):
    """setup_iter(::DenseSolver, ...) (densesolver.jl:41-52): scaling, H, H^-1,
    A H^-1 A' and its factorisation, kept on the device.  Raises
    PosDefException where cholesky! throws, DomainError where the scaling's
    sqrt does."""
    st = solver.handle.setup_iter(scaling.s, scaling.z)
    _raise_status(int(st[0]))
    if isinstance(scaling, SqrScaling) and isinstance(solver.handle, SqrHandle):
        sc = solver.handle.scaling()
        scaling.l, scaling.wbs, scaling.mu = sc["l"][0], sc["wbs"][0], sc["mu"][0]


def _raise_status(st):
    if st in (CHOL_H_FAILED, CHOL_S_FAILED):
        raise PosDefException(STATUS_NAMES[st])
    if st == DOMAIN_ERROR:
        raise DomainError(STATUS_NAMES[st])


def solve_kkt(solver: DenseSolver, prob: Problem, state: State, scaling: Scaling, dx, dy, dz, ds,
              cx, cy, cz, cs):
    """solve_kkt(::DenseSolver, ...) (densesolver.jl:54-90) against the last
    setup_iter: writes (cx,cy,cz,cs) in place, leaves (dx,dy,dz,ds) untouched."""
    out = solver.handle.solve_kkt(dx, dy, dz, ds)
    _raise_status(int(out["status"][0]))
    cx[:] = out["cx"]
    cy[:] = out["cy"]
    cz[:] = out["cz"]
    cs[:] = out["cs"]


class SolverState:
    """SolverState(prob, solver) (solver.jl:22-37): the scaling type comes from
    the plugin (KKTSolver{S} -> S(pr)).  `maxit`, `tol` default to the reference
    constants; after a solve `iters` and `status` hold the outcome."""

    def __init__(self, prob: Problem, solver: DenseSolver, maxit=40, tol=1e-5):
        self.scaling = solver.scaling_type(prob)
        self.solver = solver
        self.maxit, self.tol = maxit, tol
        self.iters, self.status = 0, None


def solve_socp(prob: Problem, ss: SolverState, *, normalise=False) -> State:
    """solve_socp(prob, ss) (solver.jl:40-153) on the GPU.  Like the reference it
    returns the final State, and raises where the reference throws.  normalise
    as in ``batch_solve`` (dense solver only)."""
    if normalise and isinstance(ss.solver, SparseSolver):
        raise ValueError("normalise: the rank-update solver does not scale (SOCP_E_UNSUPPORTED)")
    if isinstance(ss.solver, SparseSolver):  # the rank-update plugin's own IPM (spsolver.jl)
        out = ss.solver.handle.solve_socp(prob.c, prob.b if prob.m else None, prob.h, maxit=ss.maxit, tol=ss.tol)
    else:
        out = batch_solve(prob.cones, prob.n, prob.m, prob.k, prob.c, _colmajor(prob.A, prob.m, prob.n),
                          prob.b, _colmajor(prob.G, prob.k, prob.n), prob.h,
                          np.array([prob.sing], np.uint8), maxit=ss.maxit, tol=ss.tol,
                          ctx=ss.solver.ctx, P=None if prob.P is None else _colmajor(prob.P, prob.n, prob.n),
                          normalise=normalise)
    ss.iters, ss.status = int(out["iters"][0]), int(out["status"][0])
    _raise_status(ss.status)
    return State(prob, out["x"], out["y"], out["z"], out["s"])


def solve_socp_batched(problems, maxit=40, tol=1e-5, ctx=None, solver="dense", detect_infeasible=False,
                       shared_matrices=False, equilibrate=False, normalise=False):
    """Batched solve of Problems sharing dims and cones; returns (states, iters, status)
    without raising: failures are reported per problem.  solver="dense": the
    DenseSolver path (the fused register / blocked kernels); "sqr": the
    SparseSolver rank-update path (SqrHandle.solve_socp).  detect_infeasible as
    in ``batch_solve``: statuses PRIMAL_INFEASIBLE / DUAL_INFEASIBLE with the
    certificate in the returned state.  shared_matrices=True: a parametric
    batch -- every problem's A, G and sing must equal the first's (ValueError
    otherwise); one copy of them goes to the device (SOCP_F_SHARED_MATRICES).
    When any problem carries a P the batch runs the QP entry (``batch_solve``'s
    P; dense solver only); problems without one get zeros, and with
    shared_matrices every P must equal the first's as well.  equilibrate as in
    ``batch_solve`` (dense solver only); `sing` is then probed on the scaled G.
    normalise as in ``batch_solve`` (dense solver only)."""
    p0 = problems[0]
    n, m, k = p0.n, p0.m, p0.k
    for p in problems:
        assert (p.n, p.m, p.k) == (n, m, k)
    if shared_matrices:
        for i, p in enumerate(problems):
            for name in ("A", "G", "P"):
                if getattr(p, name) is None and getattr(p0, name) is None:
                    continue
                if getattr(p, name) is None or getattr(p0, name) is None or \
                        not np.array_equal(getattr(p, name), getattr(p0, name)):
                    raise ValueError(f"shared_matrices=True: problem {i}'s {name} differs from problem 0's")
            if bool(p.sing) != bool(p0.sing):
                raise ValueError(f"shared_matrices=True: problem {i}'s sing differs from problem 0's")
    mats = [p0] if shared_matrices else problems
    c = np.concatenate([p.c for p in problems])
    A = np.concatenate([_colmajor(p.A, m, n) for p in mats]) if m else None
    b = np.concatenate([p.b for p in problems]) if m else None
    G = np.concatenate([_colmajor(p.G, k, n) for p in mats])
    h = np.concatenate([p.h for p in problems])
    sing = np.array([p.sing for p in mats], np.uint8)
    P = None
    if any(p.P is not None for p in problems):
        if solver == "sqr":
            raise ValueError("P: the rank-update solver takes linear objectives only")
        P = np.concatenate([_colmajor(p.P, n, n) if p.P is not None else np.zeros(n * n) for p in mats])
    if equilibrate and solver == "sqr":
        raise ValueError("equilibrate: the rank-update solver does not scale (SOCP_E_UNSUPPORTED)")
    if normalise and solver == "sqr":
        raise ValueError("normalise: the rank-update solver does not scale (SOCP_E_UNSUPPORTED)")
    if solver == "sqr":
        out = SqrHandle(p0.cones, n, m, k, A, G, sing, ctx=ctx, shared_matrices=shared_matrices,
                        batch=len(problems)).solve_socp(
            c, b, h, maxit=maxit, tol=tol, detect_infeasible=detect_infeasible)
    else:
        out = batch_solve(p0.cones, n, m, k, c, A, b, G, h, None if equilibrate else sing, maxit=maxit, tol=tol,
                          ctx=ctx, detect_infeasible=detect_infeasible, shared_matrices=shared_matrices, P=P,
                          equilibrate=equilibrate, normalise=normalise)
    states = [State(p, out["x"][i * n:(i + 1) * n], out["y"][i * m:(i + 1) * m],
                    out["z"][i * k:(i + 1) * k], out["s"][i * k:(i + 1) * k])
              for i, p in enumerate(problems)]
    return states, out["iters"], out["status"]
