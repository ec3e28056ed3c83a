"""A batch of cone programs as a differentiable torch operation.

``SocpFunction`` solves  minimise x'Px/2 + c'x  s.t.  Ax = b, Gx + s = h,
s in K  for every problem of a batch on the GPU (``socp_amd.batch_solve``),
centres the returned iterates (``socp_amd.batch_centre``) and, in backward,
forms dL/d(c, A, b, G, h, P) from dL/d(x, y, z, s) with ``socp_amd.batch_vjp``
at the centred point.  Why the centring: the adjoint of the KKT system is the
exact derivative only on the central path, and a solver's returned iterate is
off it by its own size.

Tensors are flat, float64, contiguous CUDA tensors in the library's layout
(include/socp.h): vectors stacked batch-major, matrices column-major per
problem and stacked batch-major -- so a batch's G is, as a tensor, ``(B, n, k)``
of columns: ``G.view(B, n, k)[p, j]`` is column j of problem p's k x n matrix
(``M.transpose(1, 2).contiguous().view(-1)`` from a ``(B, k, n)`` tensor of
matrices).  Gradients come back flat in the same layout.  With shared matrices
A, G and P are ONE matrix each, and so are their gradients: the sum over the
batch of the per-problem gradients, formed on the device in a fixed order
(``socp_batch_vjp_sum``), in the shape of the shared tensor.

Everything is stream-ordered on torch's current stream; nothing synchronises.
Importing this module needs torch but no GPU.
"""
from __future__ import annotations

import torch

import socp_amd as S

__all__ = ["SocpFunction", "SocpLayer"]


class _Config:
    """What a SocpFunction call needs beside its tensors."""

    def __init__(self, cones, n, m, k, centre_steps, shared_matrices, solve_options):
        self.cones, self.n, self.m, self.k = cones, int(n), int(m), int(k)
        self.centre_steps = int(centre_steps)
        self.shared_matrices = bool(shared_matrices)
        self.solve_options = dict(solve_options)


def _rows(v, B):
    return v.view(B, -1)


class SocpFunction(torch.autograd.Function):
    """``x, y, z, s, status, iters = SocpFunction.apply(cfg, c, A, b, G, h, P, sing)``.

    cfg: a ``SocpLayer``'s configuration.  A and b are None when m = 0; P and
    sing may be None.  x, y, z, s are the centred solution (a problem whose
    solve did not converge keeps the solver's iterate); status and iters are
    ``batch_solve``'s and carry no gradient.  A problem with a nonzero status,
    from the solve or from the centring, contributes exactly zero to every
    gradient.  With shared matrices the gradients of A, G and P are sums over the
    batch and come back in the shape of the one shared tensor."""

    @staticmethod
    def forward(ctx, cfg, c, A, b, G, h, P, sing):
        n, m, k = cfg.n, cfg.m, cfg.k
        opts = dict(cfg.solve_options)
        lib_ctx = opts.pop("ctx", None)
        out = S.batch_solve(cfg.cones, n, m, k, c, A, b, G, h, sing, P=P, shared_matrices=cfg.shared_matrices,
                            ctx=lib_ctx, **opts)
        B = out["status"].numel()
        x, z, s = out["x"], out["z"], out["s"]
        y = out["y"][:B * m]
        status, iters = out["status"], out["iters"]
        skip = status
        if cfg.centre_steps:
            kept = [v.clone() for v in (x, y, z, s)]
            cen = S.batch_centre(cfg.cones, n, m, k, c, A, b, G, h, sing, x, y if m else None, z, s,
                                 steps=cfg.centre_steps, P=P, ctx=lib_ctx, shared_matrices=cfg.shared_matrices,
                                 force_large=bool(opts.get("force_large", False)))
            ok = (status == 0).view(B, 1)
            x, y, z, s = [torch.where(ok, _rows(v, B), _rows(v0, B)).reshape(-1) if v.numel() else v
                          for v, v0 in zip((x, y, z, s), kept)]
            skip = torch.where(status != 0, status, cen["status"])
        ctx.cfg, ctx.lib_ctx, ctx.force_large = cfg, lib_ctx, bool(opts.get("force_large", False))
        ctx.save_for_backward(A, G, P, sing, x, y, z, s, skip)
        ctx.mark_non_differentiable(status, iters)
        ctx.set_materialize_grads(False)
        return x, y, z, s, status, iters

    @staticmethod
    def backward(ctx, gx, gy, gz, gs, _gstatus, _giters):
        cfg = ctx.cfg
        A, G, P, sing, x, y, z, s, skip = ctx.saved_tensors
        need = dict(zip(("c", "A", "b", "G", "h", "P"), ctx.needs_input_grad[1:7]))
        if cfg.m == 0:
            need["A"] = need["b"] = False
        want = ["d" + key for key, on in need.items() if on]
        cont = lambda g: None if g is None else g.contiguous().view(-1)  # noqa: E731
        r = S.batch_vjp(cfg.cones, cfg.n, cfg.m, cfg.k, A, G, sing, x, y if cfg.m else None, z, s, cont(gx),
                        cont(gy) if cfg.m else None, cont(gz), cont(gs), P=P, skip=skip, want=want, ctx=ctx.lib_ctx,
                        force_large=ctx.force_large, shared_matrices=cfg.shared_matrices)
        like = lambda key, t: None if key not in r else r[key].view(t.shape)  # noqa: E731
        return (None, r.get("dc"), like("dA", A), r.get("db"), like("dG", G), r.get("dh"), like("dP", P), None)


class SocpLayer(torch.nn.Module):
    """``SocpLayer(cones, n, m, k, *, centre_steps=4, shared_matrices=False, normalise=False, **solve_options)``

    cones: ``batch_solve``'s cone table.  centre_steps: the Newton centring
    steps after the solve (0: differentiate at the solver's iterate, which is
    wrong by the iterate's distance from the central path).  shared_matrices:
    one A, G (and P, sing) for the batch -- the parametric case; c, b and h get
    per-problem gradients, A, G and P the batch's sum.  normalise:
    ``batch_solve``'s (SOCP_F_NORMALISE), for the forward solve only -- the
    centring and the adjoint work on the caller's data, and the un-normalised
    iterate is what they receive.  solve_options go to ``batch_solve`` (maxit,
    tol, force_large, ctx, ...).

    ``layer(c, A, b, G, h, P=None, sing=None)`` returns
    ``(x, y, z, s, status, iters)``; see ``SocpFunction`` and the module
    docstring for the layout: G is a ``(B, n, k)`` tensor of columns."""

    def __init__(self, cones, n, m, k, *, centre_steps=4, shared_matrices=False, normalise=False, **solve_options):
        super().__init__()
        if normalise:
            solve_options["normalise"] = True
        self.cfg = _Config(cones, n, m, k, centre_steps, shared_matrices, solve_options)

    def forward(self, c, A, b, G, h, P=None, sing=None):
        return SocpFunction.apply(self.cfg, c, A, b, G, h, P, sing)
