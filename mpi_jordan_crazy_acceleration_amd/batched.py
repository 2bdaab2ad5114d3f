"""Inverse, refined solve and slogdet of a stack of small matrices: ``A`` of shape (..., n, n), n <= 1024.

One workgroup inverts one matrix (``Device::block_inverse``, the engine's candidate inverter), so a stack
of thousands of small systems is a handful of launches instead of an engine per matrix::

    F = gj.batched.factor(A)            # A: (..., n, n), numpy or torch, float32 / float64, any strides
    X = F.solve(B)                      # B: (..., n) or (..., n, k); refined in fp64, never a bare inv @ B
    Ainv = F.inverse()
    sign, logabsdet = F.slogdet()

A CUDA tensor stays on its GPU (no host round trip); numpy arrays and CPU tensors run the host
executor.  Results come back in A's dtype and container.  Every matrix is scaled by an exact power of
two to ||.||_inf in [1, 2) before it is inverted, so that the singularity rule is the engine's,
|pivot| < eps * ||A_b||_inf per matrix, whatever the scales in the stack, and the scaling is undone
exactly.  A matrix larger than 1024 is the big engine's: :func:`mpi_jordan_crazy_acceleration_amd.factor`.
A^T X = B for a stack is ``solve(A.transpose(-1, -2), B)``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._native import load_native
from .models.gauss_jordan import SingularMatrixError
from . import ops

MAX_ORDER = 1024
_TDT = {"fp64": torch.float64, "fp32": torch.float32}


def _as_tensor(A, what: str) -> torch.Tensor:
    if isinstance(A, torch.Tensor):
        t = A.detach()
    else:
        a = np.asarray(A)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        # (negative strides and read-only arrays are not torch's; the tensor is only read)
        t = torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else a.copy())
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be float32 or float64")
    return t


def _stack_of(A):
    """A (..., n, n) -> (fp64 contiguous (nb, n, n) on A's device, leading shape, n, A as a tensor)"""
    t = _as_tensor(A, "A")
    if t.ndim < 2 or t.shape[-1] != t.shape[-2]:
        raise ValueError("A must be (..., n, n)")
    n = int(t.shape[-1])
    if n < 1:
        raise ValueError("A must be (..., n, n) with n >= 1")
    if n > MAX_ORDER:
        raise ValueError(f"gj.batched handles n <= {MAX_ORDER}; for a larger matrix loop over gj.factor")
    lead = tuple(int(s) for s in t.shape[:-2])
    nb = int(np.prod(lead)) if lead else 1
    if nb < 1:
        raise ValueError("A must hold at least one matrix")
    return t.to(torch.float64).reshape(nb, n, n).contiguous(), lead, n, t


def _native_device(t: torch.Tensor):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)  # A may have been written on torch's stream
    return ops.device_for(t)


def _back(x: torch.Tensor, like, like_t: torch.Tensor):
    """x in the dtype and container of the input `like` (whose tensor form is like_t)"""
    x = x.to(like_t.dtype)
    return x if isinstance(like, torch.Tensor) else x.numpy()


class BatchFactored:
    """The inverses of a stack, kept for any number of solves (:func:`factor`).

    ``valid`` (bool) and ``exponents`` (int32) have A's leading shape; ``n``, ``nb``, ``dtype``;
    ``infos``: the last solve's ``converged`` / ``steps`` / ``residual`` / ``backward_error`` as arrays of
    shape (nb, k).  With ``check=False`` the inverse and every solution of an invalid (singular, NaN or
    Inf) matrix are NaN and the other matrices are unaffected."""

    def __init__(self, A, dtype: str = "fp64", eps: float = 1e-15, check: bool = True,
                 workspace_bytes: Optional[int] = None, _device=None):
        if dtype not in _TDT:
            raise ValueError("dtype must be 'fp64' or 'fp32'")
        a64, lead, n, t = _stack_of(A)
        self._like, self._like_t, self._lead = A, t, lead
        self.n, self.nb, self.dtype = n, int(a64.shape[0]), dtype
        self._cuda = a64.is_cuda
        self._tdev = a64.device
        dev = _device if _device is not None else _native_device(a64)
        self._bs = load_native().BatchSolver(dev, dtype, n, self.nb, float(eps), int(workspace_bytes or 0))
        self._bs.factor(a64.data_ptr(), n * n, n)
        self.chunk = int(self._bs.chunk)
        self.valid = np.asarray(self._bs.valid).astype(bool).reshape(lead)
        self.exponents = np.asarray(self._bs.exponents, dtype=np.int32).reshape(lead)
        self.infos = None
        if check and not self.valid.all():
            bad = np.flatnonzero(~self.valid.reshape(-1)).tolist()
            raise SingularMatrixError(f"singular or non-finite matrices in the stack at indices {bad}")

    def inverse(self):
        """inv(A) with A's shape, dtype and container (NaN for an invalid matrix)."""
        out = torch.empty((self.nb, self.n, self.n), dtype=_TDT[self.dtype], device=self._tdev)
        if self._cuda:
            torch.cuda.synchronize(self._tdev)  # the allocator may hand out a block torch's stream still uses
        self._bs.inverse(out.data_ptr(), self.n * self.n, self.n)
        return _back(out.reshape(self._lead + (self.n, self.n)), self._like, self._like_t)

    def solve(self, B, max_refine: int = -1, tol: float = 1e-15):
        """A X = B per matrix: B of shape (..., n) or (..., n, k), any k.  X = inv(A) B, then refined with the
        residual B - A X in fp64 against the kept fp64 copy of A, every (matrix, column) stopped by the rule
        of every other solve path (backward error <= tol, the budget, or a residual that stops shrinking)."""
        b = _as_tensor(B, "B")
        vec = b.ndim == len(self._lead) + 1
        if vec:
            b = b.unsqueeze(-1)
        if b.ndim != len(self._lead) + 2 or tuple(b.shape[:-2]) != self._lead or b.shape[-2] != self.n \
                or b.shape[-1] < 1:
            raise ValueError("B must be (..., n) or (..., n, k) with A's leading shape and k >= 1")
        k = int(b.shape[-1])
        b64 = b.to(device=self._tdev, dtype=torch.float64).reshape(self.nb, self.n, k).contiguous()
        xs = torch.empty((self.n, self.nb, k), dtype=torch.float64, device=self._tdev)
        if self._cuda:
            torch.cuda.synchronize(self._tdev)
        info = self._bs.solve(b64.data_ptr(), self.n * k, k, xs.data_ptr(), k, int(max_refine), float(tol))
        self.infos = {"converged": np.asarray(info["converged"]).astype(bool), "steps": np.asarray(info["steps"]),
                      "residual": np.asarray(info["residual"]), "backward_error": np.asarray(info["backward_error"])}
        x = xs.permute(1, 0, 2).reshape(self._lead + (self.n, k))
        if vec:
            x = x.squeeze(-1)
        return _back(x.contiguous(), self._like, self._like_t)

    def slogdet(self):
        """(sign, logabsdet) as fp64 numpy arrays of A's leading shape, numpy's convention; from an fp64 LU of
        the kept copy of A, not from the inverse."""
        sg, lg = self._bs.slogdet()
        return np.asarray(sg).reshape(self._lead), np.asarray(lg).reshape(self._lead)

    def rcond(self):
        """1 / (||A_b||_inf ||inv(A_b)||_inf) from the norms the factorisation already has (0 where invalid)."""
        an, inn = np.asarray(self._bs.norms), np.asarray(self._bs.inverse_norms)
        ok = self.valid.reshape(-1)
        out = np.zeros(self.nb)
        out[ok] = 1.0 / (an[ok] * inn[ok])
        return out.reshape(self._lead)


def factor(A, dtype: str = "fp64", eps: float = 1e-15, check: bool = True,
           workspace_bytes: Optional[int] = None) -> BatchFactored:
    """Invert every matrix of the stack A (..., n, n), 1 <= n <= 1024, once and keep the inverses.

    ``dtype``: the precision the inverses are computed and kept in.  ``eps``: a pivot below
    eps * ||A_b||_inf makes matrix b singular.  ``check``: raise SingularMatrixError (naming the indices)
    if any matrix is invalid; False: report them in ``valid`` and return NaN for them.
    ``workspace_bytes``: the stack is inverted in chunks whose working set (packed panel, transposed
    inverses, the inverter's scratch) stays under it; default 256 MiB."""
    return BatchFactored(A, dtype=dtype, eps=eps, check=check, workspace_bytes=workspace_bytes)


def inverse(A, dtype: str = "fp64", eps: float = 1e-15, check: bool = True, workspace_bytes: Optional[int] = None):
    """inv(A) for a stack A (..., n, n): see :func:`factor`."""
    return factor(A, dtype=dtype, eps=eps, check=check, workspace_bytes=workspace_bytes).inverse()


def solve(A, B, max_refine: int = -1, tol: float = 1e-15, dtype: str = "fp64", eps: float = 1e-15,
          check: bool = True, workspace_bytes: Optional[int] = None):
    """A X = B for a stack, refined in fp64: see :func:`factor` and :meth:`BatchFactored.solve`."""
    return factor(A, dtype=dtype, eps=eps, check=check, workspace_bytes=workspace_bytes).solve(B, max_refine, tol)


def slogdet(A):
    """(sign, logabsdet) of every matrix of the stack (fp64 numpy arrays of A's leading shape), by one
    ``Device::slogdet_batch`` launch on the fp64 copy of A; no inverse is computed."""
    a64, lead, _, _ = _stack_of(A)
    _native_device(a64)
    sg, lg = ops.slogdet_batch(a64)
    return sg.cpu().numpy().reshape(lead), lg.cpu().numpy().reshape(lead)
