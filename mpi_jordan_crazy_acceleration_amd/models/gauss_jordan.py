"""High-level single-process API of the block Gauss-Jordan inverter.

Mirrors the reference program's flow (``main.cpp:343-519``: build A, time ``Jordan``, print the
corners, recompute A, residual) but runs in-process: ``ranks`` host threads each drive one GPU
(RCCL between them when every rank has its own GPU) or one virtual host rank (``device="cpu"``).
For one process per GPU under ``torch.distributed`` use :class:`parallel.dist.DistributedGaussJordan`.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from .._native import load_native

STATUS = {0: "ok", 1: "singular matrix", 2: "not enough memory", 3: "cannot open", 4: "cannot read",
          5: "bad arguments", 6: "communication error", 7: "not enough memory for block",
          8: "verification failed"}


class SingularMatrixError(ArithmeticError):
    """Raised when every remaining candidate block is singular (reference: ``singular matrix``)."""


def _default_device() -> str:
    return "gpu" if load_native().device_count() > 0 else "cpu"


@dataclass
class GaussJordan:
    """Configuration of an in-process run (CLI-equivalent).

    block_size : reference ``m`` — the pivot block size (128 or 256 map best onto the MFMA tiles)
    ranks      : reference ``p`` — GPUs (device="gpu") or virtual host ranks (device="cpu")
    dtype      : "fp64" (reference) or "fp32" (CDNA4 fp32 MFMA path)
    """

    block_size: int = 128
    ranks: int = 1
    device: str = "auto"
    dtype: str = "fp64"
    comm: str = "auto"  # auto | rccl | loopback | async (stream-ordered virtual ranks)
    jitter_us: float = 0.0  # comm="async": random per-rank arrival delays (race screening)
    chunk_cols: int = 0
    depth: int = 0  # 0 = auto (engine.hpp)
    pivot: str = "block-min-inv-norm"  # or "partial" (block partial pivoting, SolveOptions::pivot)
    eps: float = 1e-15
    sync_debug: bool = False
    residual: str = "always"
    host_threads: int = 0
    race_check: bool = False  # happens-before schedule checker (RaceCheckDevice): report["races"]
    det: bool = False  # keep the pivot blocks for Engine::slogdet (SolveOptions::track_det)
    # Scale A's rows and columns by powers of two ahead of the sweep and undo the exponents on the inverse
    # (SolveOptions::equilibrate): exact, and both singularity tests then ignore the units of A's rows and
    # columns.  The exponents come from the engine's panel, so an fp32 engine scales what survived the
    # conversion to fp32.  Off: nothing changes.
    equilibrate: bool = False
    extra: dict = field(default_factory=dict)

    def _cfg(self, n: int) -> dict:
        dev = _default_device() if self.device == "auto" else self.device
        cfg = dict(n=int(n), m=int(self.block_size), ranks=int(self.ranks), device=dev,
                   dtype=self.dtype, comm=self.comm, chunk_cols=int(self.chunk_cols), depth=int(self.depth),
                   pivot=self.pivot,
                   eps=float(self.eps),
                   sync_debug=bool(self.sync_debug), residual=self.residual,
                   host_threads=int(self.host_threads), jitter_us=float(self.jitter_us),
                   race_check=bool(self.race_check))
        if self.det:
            cfg["det"] = True
        if self.equilibrate:
            cfg["equilibrate"] = True
        cfg.update(self.extra)
        return cfg

    def run(self, n: int, gen: str = "absdiff", seed: int = 0, file: Optional[str] = None,
            input: Optional[np.ndarray] = None, keep_inverse: bool = False, repeats: int = 1,
            rhs=None, keep_solution: bool = False, profile: bool = False, nrhs: int = 1,
            trans: bool = False, update=None, det: bool = False, bounds: bool = False,
            cond: bool = False, precise: bool = False) -> dict:
        """One CLI-equivalent run.  ``rhs``: None, "ones", "random", a file path, an n-vector or an
        n x k matrix — then x = inv(A) b is computed on the devices, refined in fp64, and
        ``axb_residual`` = ||A x - b||_inf reported.  ``nrhs`` > 1 (implied by a matrix): the block
        path, all columns per sweep (``axb_columns``: one info per column, ``x``: n x nrhs).
        ``trans``: A^T x = b from the same inverse (the block path at any width); ``axb_residual`` is
        then ||A^T x - b||_inf and the report holds ``trans`` = True.
        ``update`` = (U, V), n-vectors or n x k with k <= 64: after the inversion the inverse is
        updated to that of A + U V^T (Engine::update_inverse) and the ``rhs`` solve, the residual and
        ``keep_inverse`` all refer to A + U V^T; the report gains ``update`` = {k, min_pivot, cond1,
        seconds}.
        ``det``: the report gains ``slogdet`` = [sign, logabsdet] of the matrix the inverse belongs to
        (Engine::slogdet; after the update, if one is given) and ``slogdet_ranks``, every rank's pair
        (ranks x 2: the same bits in every row).
        ``bounds`` (with ``rhs``): every entry of ``axb_columns`` gains ``ferr`` and ``berr`` of its
        column (the forward error bound and the componentwise backward error of LAPACK's xGERFS); one
        right-hand side then takes the block path as one column.
        ``precise`` (with ``rhs``): extra-precise refinement (see :class:`Factored`); every entry of
        ``axb_columns`` gains ``dx_rel``, ``dx_ratio`` and ``err_est`` and the report holds ``precise`` =
        True; one right-hand side then takes the block path as one column.  Not with ``trans``
        (ValueError).
        ``cond``: the report gains ``cond`` = {"one", "inf"}, the condition numbers
        ||A||_p ||inv(A)||_p of the matrix the inverse belongs to (after the update, if one is given).
        With ``equilibrate`` the report gains ``equilibrate`` = {applied, row_exp_range, col_exp_range}.
        ``policy_ranks`` of every report: what each rank's engine chose (Engine.policy without the
        communicator's entries), one dict per rank."""
        if trans and precise:
            raise ValueError("precise is not available with trans")
        cfg = self._cfg(n)
        if det:
            cfg["det"] = True
        cfg.update(gen=gen, seed=int(seed), keep_inverse=keep_inverse, repeats=int(repeats),
                   keep_solution=bool(keep_solution), profile=bool(profile))
        if file is not None:
            cfg["file"] = str(file)
        if input is not None:
            cfg["input"] = np.ascontiguousarray(input, dtype=np.float64)
        if isinstance(rhs, str):
            cfg["rhs"] = rhs
        elif rhs is not None:
            r = np.asarray(rhs, dtype=np.float64)
            if r.ndim == 2 and r.shape[1] > 1:
                nrhs = r.shape[1]
            cfg["rhs_input"] = np.ascontiguousarray(r.reshape(-1))
        cfg["nrhs"] = int(nrhs)
        if trans:
            cfg["trans"] = True
        if bounds:
            cfg["bounds"] = True
        if precise:
            cfg["precise"] = True
        if cond:
            cfg["cond"] = True
        if update is not None:
            u, v = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
                    for t in update)
            u, v = u.reshape(u.shape[0], -1), v.reshape(v.shape[0], -1)
            if u.shape != v.shape or u.shape[0] != int(n) or not 1 <= u.shape[1] <= 64:
                raise ValueError("update=(U, V): n-vectors or n x k matrices of one shape, 1 <= k <= 64")
            cfg["update_u"] = np.ascontiguousarray(u)
            cfg["update_v"] = np.ascontiguousarray(v)
        rep = load_native().run_local(cfg)
        rep["status_name"] = STATUS.get(rep["status"], "error")
        return rep

    def inverse(self, A):
        is_torch = isinstance(A, torch.Tensor)
        if is_torch and A.is_cuda and self.ranks == 1 and self.device in ("auto", "gpu"):
            return self._inverse_resident(A)
        a = A.detach().to("cpu", torch.float64).numpy() if is_torch else np.asarray(A, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("A must be square")
        rep = self.run(a.shape[0], input=a, keep_inverse=True)
        if rep["status"] == 1:
            raise SingularMatrixError("singular matrix")
        if rep["status"] != 0:
            raise RuntimeError(rep["message"] or rep["status_name"])
        inv = rep["inverse"]
        if is_torch:
            return torch.from_numpy(inv).to(device=A.device, dtype=A.dtype)
        return inv


    def _engine_resident(self, A: torch.Tensor, track_det: bool = False):
        """The native engine, solved on a CUDA tensor's rows (copied device-to-device)."""
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("A must be square")
        C = load_native()
        tdt = torch.float64 if self.dtype == "fp64" else torch.float32
        a = A.detach().to(tdt).contiguous()
        n = a.shape[0]
        idx = a.device.index if a.device.index is not None else torch.cuda.current_device()
        eng = C.Engine(_hip_device(idx), C.self_comm(), n, int(self.block_size), self.dtype,
                       int(self.chunk_cols), float(self.eps), bool(self.sync_debug), int(self.depth),
                       pivot=self.pivot, track_det=bool(track_det or self.det),
                       equilibrate=bool(self.equilibrate))
        torch.cuda.synchronize(a.device)  # A may have been written on torch's stream
        eng.upload_rows_device(a.data_ptr(), a.stride(0))
        st = eng.solve()
        if st["status"] == 1:
            raise SingularMatrixError("singular matrix")
        if st["status"] != 0:
            raise RuntimeError(STATUS.get(st["status"], "error"))
        return eng, a

    def _inverse_resident(self, A: torch.Tensor) -> torch.Tensor:
        """Inverse of a CUDA tensor without host round trips: the rows are copied device-to-device
        into the engine's panel and the result straight back into a new tensor on A's device."""
        eng, a = self._engine_resident(A)
        out = torch.empty_like(a)
        eng.download_rows_device(out.data_ptr(), out.stride(0))
        return out.to(A.dtype)

    def factor(self, A) -> "Factored":
        """Invert A once and keep the engine: see :func:`factor`."""
        return Factored(self, A)

    def solve_resident(self, A: torch.Tensor, b, max_refine: int = -1, tol: float = 1e-15, trans: bool = False,
                       bounds: bool = False, precise: bool = False):
        """A x = b for a CUDA tensor A through the engine (Engine::solve_rhs_device): x = inv(A) b by
        the native GEMV, then iterative refinement with the residual b - A x in fp64 against A's
        rows (an fp32 inverse refines to fp64 accuracy on a well-conditioned system, as the CLI's
        --rhs path).  b: an n-vector, or an n x k matrix: then Engine::solve_rhs_block refines all
        columns together on the device (one pass over each matrix per sweep, B and X never leave the
        GPU).  ``trans``: A^T x = b from the same inverse, always by the block path (a vector is one
        column).  ``bounds``: every info gains ``ferr`` / ``berr`` (see :class:`Factored`), also by the
        block path.  ``precise``: extra-precise refinement (see :class:`Factored`), also by the block path;
        not with ``trans`` (ValueError).  Returns (x on A's device in A's dtype with b's shape, info per column)."""
        if trans and precise:
            raise ValueError("precise is not available with trans")
        eng, _ = self._engine_resident(A)
        a64 = A.detach().to(torch.float64).contiguous()
        return _solve_on_device(eng, a64, A.dtype, b, max_refine, tol, trans, bounds, precise)


def _solve_on_device(eng, a64: torch.Tensor, out_dtype, b, max_refine: int, tol: float, trans: bool,
                     bounds: bool = False, precise: bool = False):
    """solve_resident's solve against an engine that holds inv(A); a64 = A's rows in fp64 on the GPU,
    x is returned there in out_dtype"""
    if (trans or bounds or precise) and np.ndim(b) == 1:
        bt = b.detach() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float64))
        x, infos = _solve_on_device(eng, a64, out_dtype, bt.reshape(-1, 1), max_refine, tol, trans, bounds, precise)
        return x.reshape(-1), infos
    if not (trans or bounds or precise) and (np.ndim(b) != 2 or np.shape(b)[1] == 1):  # one right-hand side: the one-vector path
        torch.cuda.synchronize(a64.device)
        bt = b.detach().to("cpu", torch.float64) if isinstance(b, torch.Tensor) else \
            torch.as_tensor(np.asarray(b, dtype=np.float64))
        x, info = eng.solve_rhs_device(np.ascontiguousarray(bt.reshape(-1).numpy()), a64.data_ptr(),
                                       a64.stride(0), int(max_refine), float(tol))
        return torch.from_numpy(x.reshape(bt.shape)).to(device=a64.device, dtype=out_dtype), [info]
    b64 = (b.detach() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float64)))
    b64 = b64.to(device=a64.device, dtype=torch.float64).contiguous()
    if b64.shape[0] != a64.shape[0] or b64.shape[1] < 1:
        raise ValueError("b must have n rows and at least one column")
    x64 = torch.empty_like(b64)
    torch.cuda.synchronize(a64.device)
    _, infos, _ = eng.solve_rhs_block(rows_f64=a64.data_ptr(), ld=a64.stride(0), b_dev=b64.data_ptr(),
                                      ldb=b64.stride(0), x_dev=x64.data_ptr(), ldx=x64.stride(0),
                                      ncols=b64.shape[1], max_refine=int(max_refine), tol=float(tol),
                                      trans=bool(trans), bounds=bool(bounds), precise=bool(precise))
    return x64.to(out_dtype), list(infos)


class Factored:
    """inv(A), computed once and kept for any number of solves (:func:`factor`).

    ``solve(b, trans=False)``: A x = b, or A^T x = b with ``trans`` -- from the same inverse, no
    second inversion -- for an n-vector or an n x k matrix b, refined in fp64 against A's rows (which
    the object keeps in fp64); returns b's shape and type.  ``inverse()``: the inverse in A's type.
    ``n``, ``dtype`` ("fp64" | "fp32": the engine's arithmetic); ``infos``: the per-column refinement
    results of the last solve.  ``solve(b, bounds=True)``: every info also holds ``ferr``, a bound of
    ||x_true - x||_inf / ||x||_inf, and ``berr``, the componentwise backward error max_i |b - A x|_i /
    (|A| |x| + |b|)_i -- LAPACK's xGERFS pair, with the resident |inv(A)| in place of a norm estimate
    and fp64 arithmetic whatever the engine dtype; as there, ``ferr`` holds to first order in
    ||I - inv(A) A|| and is to be trusted when the column's ``converged`` is true.  x is the same with
    and without the option (a vector then takes the block path as one column).
    ``solve(b, precise=True)``: extra-precise refinement (LAPACK 3.2's xGERFSX).  The residual b - A x is
    accumulated in twice the working precision (Device::panel_rhs_dd: a double-double sum over the kept
    fp64 rows, rounded once) and every column is stopped by the size of its correction: converged when
    ||inv(A) r||_inf <= 2^-53 ||x||_inf, stopped when the correction no longer halves or ``max_refine``
    corrections were applied (10 by default in this mode, LAPACK's ithresh; ``tol`` is not used).  As long as kappa(A) u < 1 for the engine's u the
    forward error falls to about 2^-53, where the fp64 residual leaves kappa(A) 2^-53: this option
    changes x.  Every info gains ``dx_rel`` (the last correction's size relative to x), ``dx_ratio``
    (the worst contraction seen) and ``err_est`` = max(max(10, sqrt(n)) 2^-53, dx_rel / (1 - dx_ratio)),
    LAPACK's normwise forward error estimate (inf when the corrections did not contract).  With
    ``bounds`` too, ``ferr`` is computed from the doubled residual and stays a valid but pessimistic
    bound (|inv(A)| |r| cannot see the cancellation inv(A) r does): ``err_est`` is the sharp figure.  A
    vector takes the block path as one column; both engine dtypes are accepted (an fp32 engine corrects
    with its fp32 inverse); not with ``trans`` (ValueError).
    ``cond(p)`` / ``rcond(p)``, p in {1, inf}: ||A||_p ||inv(A)||_p of the handle's matrix from the
    resident inverse, and its reciprocal; cached until the next ``update``.
    A CUDA tensor A stays on its GPU (the resident engine); a numpy
    array or a CPU tensor runs one host rank.
    ``update(U, V)``: the handle becomes that of A + U V^T (rank k <= 64) by the matrix inversion
    lemma, one pass over the inverse instead of another inversion; ``updates`` counts the updates
    applied since the inversion and ``last_update`` holds the last one's result.
    ``slogdet()`` / ``det()``: the determinant of the matrix the handle stands for, from the pivot
    blocks the inversion already computed (no second factorisation); they follow every ``update``.
    ``equilibration``: what ``equilibrate=True`` did to the inversion's input (None without it); the
    inverse, the solves, the updates and the determinant all refer to A itself either way."""

    def __init__(self, gj: "GaussJordan", A):
        self._is_torch = isinstance(A, torch.Tensor)
        self._like = A if self._is_torch else None
        self.dtype = gj.dtype
        self.infos: list = []
        self.updates = 0
        self.last_update: Optional[dict] = None
        self._cond: Optional[dict] = None
        self._m = int(gj.block_size)
        self._a64_owned = False
        if self._is_torch and A.is_cuda:
            self._cuda = True
            self._eng, self._a = gj._engine_resident(A, track_det=True)
            self._a64 = A.detach().to(torch.float64).contiguous()
            self.n = int(A.shape[0])
            return
        self._cuda = False
        a = A.detach().to("cpu", torch.float64).numpy() if self._is_torch else np.asarray(A, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("A must be square")
        C = load_native()
        self.n = int(a.shape[0])
        self._a64 = np.ascontiguousarray(a)
        self._eng = C.Engine(C.host_device(int(gj.host_threads)), C.self_comm(), self.n, int(gj.block_size),
                             gj.dtype, int(gj.chunk_cols), float(gj.eps), bool(gj.sync_debug), int(gj.depth),
                             pivot=gj.pivot, track_det=True, equilibrate=bool(gj.equilibrate))
        self._eng.upload_local_rows(self._a64)
        st = self._eng.solve()
        if st["status"] == 1:
            raise SingularMatrixError("singular matrix")
        if st["status"] != 0:
            raise RuntimeError(STATUS.get(st["status"], "error"))

    @property
    def equilibration(self) -> Optional[dict]:
        """{"applied", "row_exp", "col_exp"} of the inversion (``equilibrate=True``): whether a scaling
        pass ran and the int32 row / column exponents (numpy arrays of n), with As = ldexp(A, row_exp[i]
        + col_exp[j]) the matrix the sweep inverted.  None when the option is off."""
        return self._eng.equil_exponents()

    def solve(self, b, trans: bool = False, max_refine: int = -1, tol: float = 1e-15, bounds: bool = False,
              precise: bool = False):
        if trans and precise:
            raise ValueError("precise is not available with trans")
        if self._cuda:
            out_dtype = b.dtype if isinstance(b, torch.Tensor) else self._like.dtype
            x, self.infos = _solve_on_device(self._eng, self._a64, out_dtype, b, max_refine, tol, trans, bounds,
                                             precise)
            return x
        b_torch = isinstance(b, torch.Tensor)
        bn = b.detach().to("cpu", torch.float64).numpy() if b_torch else np.asarray(b, dtype=np.float64)
        if bn.ndim not in (1, 2) or bn.shape[0] != self.n:
            raise ValueError("b must be an n-vector or an n x k matrix")
        if not (trans or bounds or precise) and (bn.ndim == 1 or bn.shape[1] == 1):  # the one-vector path, as gj.solve
            x, info = self._eng.solve_rhs_rows(np.ascontiguousarray(bn.reshape(-1)), self._a64, int(max_refine),
                                               float(tol))
            self.infos = [info]
        else:
            x, infos, _ = self._eng.solve_rhs_block(np.ascontiguousarray(bn.reshape(self.n, -1)), rows=self._a64,
                                                    max_refine=int(max_refine), tol=float(tol), trans=bool(trans),
                                                    bounds=bool(bounds), precise=bool(precise))
            self.infos = list(infos)
        x = x.reshape(bn.shape)
        return torch.from_numpy(x).to(device=b.device, dtype=b.dtype) if b_torch else x

    def update(self, U, V) -> dict:
        """A <- A + U V^T: U and V are n-vectors (k = 1, Sherman-Morrison) or n x k with k <= 64 (else
        ValueError; apply a larger update in pieces), numpy arrays or torch tensors.  The engine's
        inverse becomes inv(A + U V^T) = X - (X U) inv(I + V^T X U) (V^T X) (Engine::update_inverse) and
        the kept fp64 rows become A + U V^T, so ``solve`` and ``inverse`` go on unchanged.  Returns
        {k, min_pivot, cond1, seconds}: the smallest pivot (relative) and the 1-norm condition number
        of the k x k capacitance matrix I + V^T X U -- a near-singular update is accepted and shows
        there (and in the ``converged`` flags of later solves).  A singular one raises
        SingularMatrixError and leaves the handle as it was."""
        def as2d(M):
            if isinstance(M, torch.Tensor):
                t = M.detach().to(torch.float64)
                t = t if self._cuda else t.cpu()
            else:
                t = torch.as_tensor(np.asarray(M, dtype=np.float64))
            if t.ndim == 1:
                t = t.reshape(-1, 1)
            if t.ndim != 2 or t.shape[0] != self.n or t.shape[1] < 1:
                raise ValueError("U and V must be n-vectors or n x k matrices")
            return t

        u, v = as2d(U), as2d(V)
        if u.shape != v.shape:
            raise ValueError("U and V must have the same shape")
        k = int(u.shape[1])
        if k > 64:
            raise ValueError("update: at most 64 columns at a time; apply a larger update in pieces")
        if self._cuda:
            dev = self._a64.device
            u, v = u.to(dev).contiguous(), v.to(dev).contiguous()
            torch.cuda.synchronize(dev)
            info = self._eng.update_inverse(u_dev=u.data_ptr(), ldu=u.stride(0), v_dev=v.data_ptr(),
                                            ldv=v.stride(0), ncols=k)
        else:
            un, vn = np.ascontiguousarray(u.numpy()), np.ascontiguousarray(v.numpy())
            info = self._eng.update_inverse(un, vn)
        if info["status"] == 1:
            raise SingularMatrixError("singular update: I + V^T inv(A) U is singular")
        if info["status"] != 0:
            raise RuntimeError(STATUS.get(info["status"], "error"))
        # (the kept rows may be the caller's own array until the first update: never written in place)
        if self._cuda:  # A's fp64 rows stay on the GPU: A += U V^T by the same kernel
            from ..ops import rank_update
            if not self._a64_owned:
                self._a64 = self._a64.clone()
            rank_update(self._a64, u, v, self.n, self._m, sign=1.0, w_natural=True)
        else:
            self._a64 = self._a64 + un @ vn.T
        self._a64_owned = True
        self._cond = None
        res = {key: info[key] for key in ("k", "min_pivot", "cond1", "seconds")}
        self.updates += 1
        self.last_update = res
        return res

    def slogdet(self):
        """(sign, log|det|) of the handle's matrix as Python floats, numpy.linalg.slogdet's convention:
        det = sign * exp(logabsdet).  From the inverses of the pivot blocks that the inversion kept
        (Engine::slogdet), times det(I + V^T inv(A) U) of every ``update`` since (the determinant
        lemma), so it is valid after any number of updates."""
        d = self._eng.slogdet()
        if d["status"] != 0:
            raise RuntimeError(STATUS.get(d["status"], "error"))
        return float(d["sign"]), float(d["logabsdet"])

    def det(self) -> float:
        """sign * exp(logabsdet).  Overflows to +-inf (and underflows to 0) where the determinant leaves
        the fp64 range, as numpy.linalg.det does: prefer ``slogdet`` for anything large."""
        sign, logabs = self.slogdet()
        with np.errstate(over="ignore"):
            return float(sign * np.exp(logabs))

    def cond(self, p=np.inf) -> float:
        """||A||_p ||inv(A)||_p for p = 1 or inf (else ValueError): the condition number of the handle's
        matrix, with ||A|| from the kept fp64 rows and ||inv(A)|| from the resident inverse
        (Engine::cond: exact column sums and row sums, no estimate)."""
        if p not in (1, np.inf):
            raise ValueError("cond: p must be 1 or inf")
        if self._cond is None:
            if self._cuda:
                torch.cuda.synchronize(self._a64.device)
                self._cond = self._eng.cond(rows_f64=self._a64.data_ptr(), ld=self._a64.stride(0))
            else:
                self._cond = self._eng.cond(rows=self._a64)
        c = self._cond
        return float(c["a_norm1"] * c["inv_norm1"] if p == 1 else c["a_norminf"] * c["inv_norminf"])

    def rcond(self, p=np.inf) -> float:
        """1 / cond(p)"""
        return 1.0 / self.cond(p)

    def inverse(self):
        if self._cuda:
            out = torch.empty_like(self._a)
            self._eng.download_rows_device(out.data_ptr(), out.stride(0))
            return out.to(self._like.dtype)
        inv = self._eng.download_local_rows()
        return torch.from_numpy(inv).to(device=self._like.device, dtype=self._like.dtype) if self._is_torch else inv


_HIP_DEVICES: dict = {}


def _hip_device(idx: int):
    if idx not in _HIP_DEVICES:
        _HIP_DEVICES[idx] = load_native().hip_device(idx)
    return _HIP_DEVICES[idx]


def inverse(A, block_size: int = 128, **kw):
    """Inverse of a dense square matrix by block Gauss-Jordan (reference semantics, fixed pivot bug)."""
    return GaussJordan(block_size=block_size, residual="never", **kw).inverse(A)


def factor(A, block_size: int = 128, **kw) -> Factored:
    """Invert A once and return a :class:`Factored` handle: ``F.solve(b)``, ``F.solve(c, trans=True)``
    and ``F.inverse()`` all come from that one inversion (a forward plus an adjoint solve costs one
    inversion, not two)."""
    return GaussJordan(block_size=block_size, residual="never", **kw).factor(A)


def slogdet(A, block_size: int = 128, **kw):
    """(sign, log|det A|) as Python floats, by one block Gauss-Jordan inversion (:func:`factor`) -- the
    determinant comes from the pivot blocks, not from a second factorisation.  A singular matrix
    gives (0.0, -inf), numpy.linalg.slogdet's answer, instead of SingularMatrixError."""
    try:
        return factor(A, block_size=block_size, **kw).slogdet()
    except SingularMatrixError:
        return 0.0, float("-inf")


def cond(A, p=np.inf, block_size: int = 128, **kw) -> float:
    """||A||_p ||inv(A)||_p for p = 1 or inf (else ValueError) by one block Gauss-Jordan inversion
    (:func:`factor`, then ``Factored.cond``).  A singular matrix gives inf, numpy.linalg.cond's answer,
    instead of SingularMatrixError."""
    if p not in (1, np.inf):
        raise ValueError("cond: p must be 1 or inf")
    try:
        return factor(A, block_size=block_size, **kw).cond(p)
    except SingularMatrixError:
        return float("inf")


def det(A, block_size: int = 128, **kw) -> float:
    """det A = sign * exp(logabsdet) of :func:`slogdet`; +-inf on overflow, as numpy.linalg.det."""
    sign, logabs = slogdet(A, block_size=block_size, **kw)
    with np.errstate(over="ignore"):
        return float(sign * np.exp(logabs))


def solve(A, b, block_size: int = 128, trans: bool = False, bounds: bool = False, precise: bool = False, **kw):
    """Solve ``A x = b`` (``trans``: ``A^T x = b``, from the inverse of A itself) via the block
    Gauss-Jordan inverse.

    Every right-hand side runs the native path, x = inv(A) b on the devices next to the inverse's
    rows, refined in fp64 (never a bare ``inv @ b``): a vector through Engine::solve_rhs, a matrix
    of k columns through Engine::solve_rhs_block, which refines all columns per sweep with one pass
    over each matrix and gives every column the accuracy of the one-vector call.  A CUDA tensor A
    stays on its GPU (Engine::solve_rhs_device / solve_rhs_block_device); X keeps b's shape.
    ``bounds``: the solve also computes the error bounds of every column (the block path at any width);
    the return value is x alone -- use :func:`factor` and ``F.infos`` to read them.
    ``precise``: extra-precise refinement, the residual accumulated in twice the working precision (see
    :class:`Factored`): x itself is more accurate, to about 2^-53 as long as kappa(A) u < 1.  Not with
    ``trans`` (ValueError)."""
    if trans and precise:
        raise ValueError("precise is not available with trans")
    is_torch = isinstance(A, torch.Tensor)
    if is_torch and A.is_cuda:
        gj = GaussJordan(block_size=block_size, residual="never", **kw)
        x, _ = gj.solve_resident(A, b, trans=trans, bounds=bounds, precise=precise)
        return x
    bn = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    if bn.ndim in (1, 2):
        a = A.detach().to("cpu", torch.float64).numpy() if is_torch else np.asarray(A, dtype=np.float64)
        gj = GaussJordan(block_size=block_size, residual="never", **kw)
        rep = gj.run(a.shape[0], input=a, rhs=bn, keep_solution=True, trans=trans, bounds=bounds, precise=precise)
        if rep["status"] == 1:
            raise SingularMatrixError("singular matrix")
        if rep["status"] != 0:
            raise RuntimeError(rep["message"] or rep["status_name"])
        x = rep["x"].reshape(bn.shape)
        return torch.from_numpy(x).to(device=A.device, dtype=A.dtype) if is_torch else x
    raise ValueError("b must be an n-vector or an n x k matrix")


def run(n: int, m: int, ranks: int = 1, device: str = "auto", gen: str = "absdiff", seed: int = 0,
        file: Optional[str] = None, dtype: str = "fp64", residual: str = "always",
        input: Optional[np.ndarray] = None, **kw) -> dict:
    """The reference CLI flow in-process; returns the report dict (glob_time, residual, corners...).
    ``input``: an n x n matrix instead of the generator or a file."""
    return GaussJordan(block_size=m, ranks=ranks, device=device, dtype=dtype, residual=residual,
                       **kw).run(n, gen=gen, seed=seed, file=file, input=input)
