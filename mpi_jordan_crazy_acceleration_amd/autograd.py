"""Differentiable solve, log-determinant and inverse from one block Gauss-Jordan inversion.

``gj.solve``, ``gj.inverse``, ``gj.slogdet`` and :class:`Factored` detach their inputs.  The entry
points here attach their results to the torch graph of A (and of B for a solve), and every backward
pass runs from the same resident inverse X = inv(A) -- no second inversion:

    X = solve(A, B)               Abar = -Y X^T,  Y = A^-T Gbar  (one transposed solve)    Bbar = Y
    X = solve(A, B, trans=True)   Abar = -X Y^T,  Y = A^-1 Gbar                            Bbar = Y
    (s, l) = slogdet(A)           Abar = lbar inv(A)^T                                     s: no gradient
    X = inverse(A)                Abar = -X^T Xbar X^T

Y is ``Factored.solve(Gbar, trans=not trans)``: refined in fp64 against A's rows, not a bare product.
Abar of a solve and of slogdet is written by ``Engine.grad_matrix`` (Device::grad_matrix, the HIP kernel
``csrc/kernels/grad_matrix.hip`` on a GPU) in one pass of fp64 arithmetic over the resident panel, a
product wider than 64 columns in pieces of 64 that accumulate.  Abar of the inverse is
``Engine.vjp_inverse``: two products on the engine's GEMM and one transposing pass, with Xbar converted
to the engine dtype -- an fp32 engine gives this one gradient in fp32 arithmetic.

The gradient is that of the exact map A, B -> result: refinement is treated as exact, and the pivot
choice is piecewise constant and does not enter.

Gradients come back in the dtype and on the device of the tensor they belong to.  On a CUDA handle
nothing goes through the host (but the scalar lbar of slogdet, which is the kernel's alpha).

Limits.  Single rank.  The backward passes are ``once_differentiable``: a double backward raises torch's
usual error.  :class:`DiffFactored` has no ``update``; if ``handle.update(...)`` was called between a
forward and its backward, the backward raises RuntimeError instead of returning the gradient of
another matrix.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .models.gauss_jordan import Factored, factor as _factor

_PIECE = 64  # Device::kMaxRhs


def _check_handle(ctx, what: str) -> Factored:
    h = ctx.handle
    if h.updates != ctx.updates:
        raise RuntimeError(f"{what}: the handle was updated (Factored.update) between the forward and the backward "
                           "pass; its inverse no longer belongs to the matrix of this graph")
    return h


def _f64(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float64).contiguous()


def _engine_grad_matrix(h: Factored, G: torch.Tensor, alpha: float = 0.0, W: torch.Tensor = None,
                        Z: torch.Tensor = None, sign: float = 1.0) -> torch.Tensor:
    """G = alpha inv(A)^T + sign W Z^T by Engine.grad_matrix, W and Z (n x k, fp64, any k) in pieces of 64
    columns with accumulate after the first"""
    on_dev = bool(h._cuda)
    if on_dev:
        torch.cuda.synchronize(G.device)  # the operands may have been written on torch's stream
    k = 0 if W is None else int(W.shape[1])
    if k == 0:
        h._eng.grad_matrix(float(alpha), G=G.data_ptr(), ldg=G.stride(0), device=on_dev)
        return G
    for c0 in range(0, k, _PIECE):
        w, z = W[:, c0:c0 + _PIECE], Z[:, c0:c0 + _PIECE]
        h._eng.grad_matrix(float(alpha) if c0 == 0 else 0.0, w.data_ptr(), w.stride(0), z.data_ptr(), z.stride(0),
                           int(w.shape[1]), float(sign), c0 > 0, G.data_ptr(), G.stride(0), on_dev)
    return G


def _handle_solve(h: Factored, b: torch.Tensor, trans: bool, max_refine: int, tol: float, precise: bool):
    """Factored.solve; on a CUDA handle always the block path, which never leaves the GPU"""
    if not h._cuda:
        return h.solve(b, trans=trans, max_refine=max_refine, tol=tol, precise=precise)
    dev = h._a64.device
    b64 = _f64(b, dev).reshape(h.n, -1)
    x64 = torch.empty_like(b64)
    torch.cuda.synchronize(dev)
    _, infos, _ = h._eng.solve_rhs_block(rows_f64=h._a64.data_ptr(), ld=h._a64.stride(0), b_dev=b64.data_ptr(),
                                         ldb=b64.stride(0), x_dev=x64.data_ptr(), ldx=x64.stride(0),
                                         ncols=b64.shape[1], max_refine=int(max_refine), tol=float(tol),
                                         trans=bool(trans), bounds=False, precise=bool(precise))
    h.infos = list(infos)
    return x64.reshape(b.shape).to(b.dtype)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, handle, trans, max_refine, tol, precise):
        X = _handle_solve(handle, B.detach(), trans, max_refine, tol, precise)
        ctx.handle, ctx.updates, ctx.trans = handle, handle.updates, bool(trans)
        ctx.a_like = (A.dtype, A.device)
        ctx.save_for_backward(X)
        return X

    @staticmethod
    @once_differentiable
    def backward(ctx, Gbar):
        h = _check_handle(ctx, "solve")
        (X,) = ctx.saved_tensors
        Y = _handle_solve(h, Gbar, not ctx.trans, -1, 1e-15, False)  # in Gbar's dtype, which is B's
        gA = None
        if ctx.needs_input_grad[0]:
            dtype, device = ctx.a_like
            x64, y64 = _f64(X, device).reshape(h.n, -1), _f64(Y, device).reshape(h.n, -1)
            G = torch.empty((h.n, h.n), dtype=torch.float64, device=device)
            W, Z = (x64, y64) if ctx.trans else (y64, x64)
            gA = _engine_grad_matrix(h, G, 0.0, W, Z, -1.0).to(dtype)
        return gA, (Y if ctx.needs_input_grad[1] else None), None, None, None, None, None


class _SlogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, handle):
        sign, logabs = handle.slogdet()
        ctx.handle, ctx.updates = handle, handle.updates
        ctx.a_like = (A.dtype, A.device)
        s = torch.tensor(sign, dtype=torch.float64, device=A.device)
        l = torch.tensor(logabs, dtype=torch.float64, device=A.device)
        ctx.mark_non_differentiable(s)
        return s, l

    @staticmethod
    @once_differentiable
    def backward(ctx, _gs, gl):
        h = _check_handle(ctx, "slogdet")
        dtype, device = ctx.a_like
        G = torch.empty((h.n, h.n), dtype=torch.float64, device=device)
        return _engine_grad_matrix(h, G, float(gl)).to(dtype), None


class _Inverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, handle):
        ctx.handle, ctx.updates = handle, handle.updates
        ctx.a_like = (A.dtype, A.device)
        return handle.inverse()

    @staticmethod
    @once_differentiable
    def backward(ctx, Xbar):
        h = _check_handle(ctx, "inverse")
        dtype, device = ctx.a_like
        g = _f64(Xbar, device)
        out = torch.empty((h.n, h.n), dtype=torch.float64, device=device)
        if h._cuda:
            torch.cuda.synchronize(device)
        h._eng.vjp_inverse(g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), bool(h._cuda))
        return out.to(dtype), None


class DiffFactored:
    """inv(A), computed once (:func:`factor`), with differentiable ``solve``, ``slogdet`` and ``inverse``.

    ``handle`` is the :class:`Factored` underneath (its ``infos``, ``cond`` and so on stay available);
    every result is attached to the graph of A, and of B for a solve, and every backward pass works from
    the handle's resident inverse by the formulas of this module's docstring.  An fp32 engine
    (``dtype="fp32"``) still gives the ``solve`` gradients to fp64 accuracy on a well-conditioned system (X
    and Y are refined against the fp64 rows); its ``slogdet`` and ``inverse`` gradients carry the fp32
    inverse's accuracy, and the ``inverse`` gradient is formed in fp32 arithmetic."""

    def __init__(self, A: torch.Tensor, block_size: int = 128, **kw):
        if not isinstance(A, torch.Tensor):
            raise TypeError("gj.autograd.factor takes a torch tensor; use gj.factor for numpy arrays")
        if A.dtype not in (torch.float32, torch.float64):
            raise TypeError("gj.autograd.factor: A must be float32 or float64")
        self.A = A
        self.handle: Factored = _factor(A, block_size=block_size, **kw)
        self.n = self.handle.n

    def solve(self, B: torch.Tensor, trans: bool = False, max_refine: int = -1, tol: float = 1e-15,
              precise: bool = False) -> torch.Tensor:
        """A X = B (``trans``: A^T X = B) for an n-vector or an n x k matrix B of any k, refined as
        ``Factored.solve`` does; differentiable in A and B."""
        if trans and precise:
            raise ValueError("precise is not available with trans")
        if not isinstance(B, torch.Tensor):
            raise TypeError("gj.autograd: B must be a torch tensor")
        if B.ndim not in (1, 2) or B.shape[0] != self.n:
            raise ValueError("B must be an n-vector or an n x k matrix")
        return _Solve.apply(self.A, B, self.handle, bool(trans), int(max_refine), float(tol), bool(precise))

    def slogdet(self):
        """(sign, log|det A|) as 0-dim fp64 tensors on A's device; ``sign`` is not differentiable."""
        return _SlogDet.apply(self.A, self.handle)

    def inverse(self) -> torch.Tensor:
        """inv(A) in A's dtype on A's device."""
        return _Inverse.apply(self.A, self.handle)


def factor(A: torch.Tensor, block_size: int = 128, **kw) -> DiffFactored:
    """Invert A once and return a :class:`DiffFactored`: a forward and a backward pass through any number
    of its solves, its log-determinant and its inverse cost that one inversion.  ``kw`` as in
    ``gj.factor`` (``dtype="fp32"``, ``equilibrate=True``, ...).  A singular A raises SingularMatrixError."""
    return DiffFactored(A, block_size=block_size, **kw)


def solve(A: torch.Tensor, B: torch.Tensor, block_size: int = 128, trans: bool = False, max_refine: int = -1,
          tol: float = 1e-15, precise: bool = False, **kw) -> torch.Tensor:
    """Differentiable ``gj.solve``: one inversion for the forward and the backward pass."""
    if trans and precise:
        raise ValueError("precise is not available with trans")
    return factor(A, block_size=block_size, **kw).solve(B, trans=trans, max_refine=max_refine, tol=tol,
                                                        precise=precise)


def inverse(A: torch.Tensor, block_size: int = 128, **kw) -> torch.Tensor:
    """Differentiable ``gj.inverse``."""
    return factor(A, block_size=block_size, **kw).inverse()


def slogdet(A: torch.Tensor, block_size: int = 128, **kw):
    """Differentiable (sign, log|det A|); a singular A raises SingularMatrixError."""
    return factor(A, block_size=block_size, **kw).slogdet()


__all__ = ["DiffFactored", "factor", "solve", "inverse", "slogdet"]
