"""Kernel-level wrappers of the hand-written gfx950 kernels, on torch tensors.

These call straight into the native kernels (no PyTorch fallback): a CUDA(HIP) tensor runs the HIP
kernel, a CPU tensor runs the host reference executor — chosen by the tensor's device, never
silently.  Used by the per-kernel numerics tests and for profiling single kernels.
"""
from __future__ import annotations

import functools

import torch

from .._native import load_native

_DT = {torch.float64: "fp64", torch.float32: "fp32"}


@functools.lru_cache(maxsize=None)
def _hip(idx: int):
    return load_native().hip_device(idx)


@functools.lru_cache(maxsize=None)
def _host():
    return load_native().host_device(0)


def device_for(t: torch.Tensor):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)
        return _hip(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return _host()


def _p(t: torch.Tensor) -> int:
    return t.data_ptr()


def gemm(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, op: str = "acc", a_kmajor: bool = False,
         zero_cols=(0, 0), zero_rows=(), zero_row_height: int = 0, tneg: torch.Tensor = None,
         latency: bool = False, dense: bool = False, c_in: torch.Tensor = None, row_blocks=None,
         row_block_m: int = 0, skip_cols=(0, 0), owner=None, lat_wide: bool = False, lat_reg: bool = False,
         glds_build: int = 0, glds_tile: int = 0, c_nt: int = -1) -> torch.Tensor:
    """C += A@B (op="acc") or C = A@B (op="store").  With a_kmajor, ``A`` is given as A^T (K x M).

    Elimination extras (op="acc"): C enters as 0 in the columns ``zero_cols`` = (c0, c1) and in the
    row blocks [r, r + zero_row_height) for r in ``zero_rows`` (at most 8).  ``tneg`` (Nt x M view,
    Nt <= N, unit column stride): also receives -C^T of C's first Nt columns, the multiplier panel
    the engine's column / look-ahead updates write as they store C.  ``latency``: the small-tile
    launch the pivot chain uses.  ``dense``: the 5-workgroups-per-CU build of the fp64 LDS-DMA
    trailing update (the engine's choice under a CU reservation).  ``c_in`` (op="acc"): the
    accumulator's input array instead of C itself (C = c_in + A@B).  ``row_blocks`` with
    ``row_block_m``: only those row blocks of C / A^T take part (GemmExtra::rsel); M = C's rows is
    then the physical height and the product runs over len(row_blocks) * row_block_m rows.
    ``skip_cols`` = (s0, s1): those output columns are neither read nor written (GemmExtra::skip_c0
    / skip_c1; multiples of 128 on the GPU).  ``owner`` = (phys, p, k): the owner-predicated launch --
    nothing happens unless g = phys[0] (an int32 tensor on C's device; None: no predicate) is >= 0
    and g % p == k.  ``lat_wide`` / ``lat_reg`` / ``glds_build`` / ``glds_tile`` / ``c_nt``: the
    per-launch kernel choices of GemmExtra (which latency kernel, the fp64 LDS-DMA build and tile
    width, non-temporal C loads | stores); the host executor ignores them."""
    assert A.dtype == B.dtype == C.dtype and A.stride(-1) == 1 and B.stride(-1) == 1 and C.stride(-1) == 1
    M, N = C.shape
    K = A.shape[0] if a_kmajor else A.shape[1]
    tp, ldt, tcols = 0, 0, 0
    if tneg is not None:
        assert tneg.dtype == C.dtype and tneg.shape[1] == M and 0 < tneg.shape[0] <= N and tneg.stride(-1) == 1
        tp, ldt, tcols = _p(tneg), tneg.stride(0), tneg.shape[0]
    cp, ldci = 0, 0
    if c_in is not None:
        assert c_in.dtype == C.dtype and c_in.shape == C.shape and c_in.stride(-1) == 1
        cp, ldci = _p(c_in), c_in.stride(0)
    rb = [int(b) for b in (row_blocks or [])]
    Msel = len(rb) * int(row_block_m) if row_block_m else M
    device_for(C).gemm(_DT[C.dtype], op, a_kmajor, Msel, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(C),
                       C.stride(0), int(zero_cols[0]), int(zero_cols[1]), [int(r) for r in zero_rows],
                       int(zero_row_height), tp, ldt, bool(latency), tcols, bool(dense), cp, ldci, rb,
                       int(row_block_m), int(skip_cols[0]), int(skip_cols[1]), owner=_owner(owner, C),
                       lat_wide=bool(lat_wide), lat_reg=bool(lat_reg), glds_build=int(glds_build),
                       glds_tile=int(glds_tile), c_nt=int(c_nt))
    return C


def _owner(owner, C):
    if owner is None:
        return None
    phys, p, k = owner
    if phys is not None:
        assert phys.dtype == torch.int32 and phys.device == C.device and phys.numel() >= 1
    return (None if phys is None else _p(phys), int(p), int(k))


def gemm_batch(products) -> None:
    """Independent small products in one launch: each item is (op, At, B, C) with At = A^T (K x M),
    op "acc" (C += A@B) or "store" (C = A@B), optionally followed by a dict of per-product extras:
    ``lat_reg`` (bool) and ``owner`` = (phys, p, k) as in gemm().  All tensors share one dtype and
    device."""
    if not products:
        return
    C0 = products[0][3]
    descs = []
    for item in products:
        op, At, B, C = item[:4]
        extra = item[4] if len(item) > 4 else {}
        assert At.dtype == B.dtype == C.dtype == C0.dtype and At.stride(-1) == 1 and B.stride(-1) == 1
        assert C.stride(-1) == 1
        M, N = C.shape
        descs.append((op, M, N, At.shape[0], _p(At), At.stride(0), _p(B), B.stride(0), _p(C), C.stride(0),
                      bool(extra.get("lat_reg", False)), _owner(extra.get("owner"), C)))
    device_for(C0).gemm_batch(_DT[C0.dtype], descs)


def generate(X: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0, kind: str = "absdiff", seed: int = 0) -> torch.Tensor:
    device_for(X).generate(_DT[X.dtype], _p(X), n, m, p, k, kind, seed)
    return X


def extract_neg_t(X: torch.Tensor, col0: int, m: int) -> torch.Tensor:
    rows = X.shape[0]
    Lt = torch.empty((m, rows), dtype=X.dtype, device=X.device)
    device_for(X).extract_neg_t(_DT[X.dtype], _p(Lt), rows, _p(X), X.stride(0), rows, col0, m)
    return Lt


def block_inverse(Lt: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0, used: torch.Tensor = None,
                  thresh: float = 0.0, nlive: int = -1):
    """Batched candidate inversion over the K-major multiplier panel Lt (m x rows).

    nlive >= 0: launch one workgroup per unused candidate only (the engine's form; scores / valid
    of used blocks are then left untouched), -1: one per local block.  Returns (inv_t [nblk, m, m] with inv_t[b] = inv(W_b)^T, scores [nblk], valid [nblk])."""
    nblk = Lt.shape[1] // m
    dev = Lt.device
    inv_t = torch.zeros((max(nblk, 1), m, m), dtype=Lt.dtype, device=dev)
    scores = torch.zeros(max(nblk, 1), dtype=torch.float64, device=dev)
    valid = torch.zeros(max(nblk, 1), dtype=torch.int32, device=dev)
    Nr = (n + m - 1) // m
    if used is None:
        used = torch.zeros(Nr, dtype=torch.int32, device=dev)
    device_for(Lt).block_inverse(_DT[Lt.dtype], _p(Lt), Lt.stride(0), _p(inv_t), _p(scores), _p(valid), _p(used),
                                 n, m, p, k, thresh, nlive)
    return inv_t[:nblk], scores[:nblk], valid[:nblk]


def block_inverse_select(Lt: torch.Tensor, inv_t: torch.Tensor, scores: torch.Tensor, valid: torch.Tensor,
                         used: torch.Tensor, n: int, m: int, p: int, k: int, thresh: float, nlive: int, t: int,
                         pos: torch.Tensor, phys_at: torch.Tensor, seq: torch.Tensor, rec: torch.Tensor,
                         out: torch.Tensor, done: torch.Tensor):
    """block_inverse with the pivot selection run by the launch's last workgroup (the engine's fused
    step).  Every buffer is the caller's: ``done`` is the int32 counter that must be 0 between
    launches, ``rec`` / ``out`` are 32-byte records.  p > 1: the local argmin -> ``rec``; p == 1: the
    whole selection (``pos`` / ``phys_at`` / ``used`` / ``seq`` / ``out`` updated).  Returns
    (fused, mirror): fused False means nothing was enqueued (the kernel family cannot fuse the
    selection); mirror is the pinned host record (step, found, phys, owner, logical, score) at p == 1,
    else None."""
    return device_for(Lt).block_inverse_select(_DT[Lt.dtype], _p(Lt), Lt.stride(0), _p(inv_t), _p(scores),
                                               _p(valid), _p(used), n, m, p, k, float(thresh), int(nlive), int(t),
                                               _p(pos), _p(phys_at), _p(seq), _p(rec), _p(out), _p(done))


def permute_blocks(X: torch.Tensor, m: int, dst_blk: torch.Tensor, colsrc: torch.Tensor) -> torch.Tensor:
    rows, ncols = X.shape
    nblk, Nr = rows // m, ncols // m
    out = torch.empty_like(X)
    device_for(X).permute_blocks(_DT[X.dtype], _p(out), out.stride(0), _p(X), X.stride(0), nblk, m, Nr,
                                 _p(dst_blk), _p(colsrc))
    return out


def row_abs_max(X: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0) -> float:
    out = torch.zeros(1, dtype=torch.float64, device=X.device)
    device_for(X).row_abs_max(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _p(out))
    return float(out.item())


def row_abs_max_minus_i(X: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0) -> float:
    """max over this rank's real rows of sum_j |X[r][j] - delta(global row, j)|; NaN if a row holds one."""
    out = torch.zeros(1, dtype=torch.float64, device=X.device)
    device_for(X).row_abs_max_minus_i(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _p(out))
    return float(out.item())


def h_block(Ht: torch.Tensor, ldr: int = 0) -> torch.Tensor:
    """The m x m block kept transposed (ld m), written row-major: returns Ht^T (leading dimension ldr >= m)."""
    m = Ht.shape[0]
    assert Ht.shape == (m, m) and Ht.is_contiguous()
    R = torch.zeros((m, max(ldr, m)), dtype=Ht.dtype, device=Ht.device)
    device_for(Ht).h_block(_DT[Ht.dtype], _p(R), R.stride(0), _p(Ht), m)
    return R[:, :m]


def hash_rows(buf: torch.Tensor, ld_bytes: int, width_bytes: int, rows: int) -> int:
    """The 64-bit verification hash (GJ_VERIFY) of `rows` rows of `width_bytes` bytes, pitch `ld_bytes`."""
    dev = device_for(buf)
    parts = torch.zeros(dev.kHashParts, dtype=torch.int64, device=buf.device)
    dev.hash_rows(_p(buf), ld_bytes, width_bytes, rows, _p(parts))
    return sum(int(v) & 0xFFFFFFFFFFFFFFFF for v in parts.cpu().tolist()) & 0xFFFFFFFFFFFFFFFF


def residual(A_loc: torch.Tensor, Full: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0) -> float:
    out = torch.zeros(1, dtype=torch.float64, device=A_loc.device)
    device_for(A_loc).residual(_DT[A_loc.dtype], _p(A_loc), _p(Full), n, m, p, k, _p(out))
    return float(out.item())


def panel_rhs(P: torch.Tensor, V: torch.Tensor, Y: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
              C_in: torch.Tensor = None, sign: float = 1.0, active: torch.Tensor = None,
              colmax: torch.Tensor = None, ncols: int = None) -> torch.Tensor:
    """Y = C_in + sign * P @ V over the columns c < n (Device::panel_rhs): ``P`` this rank's rows of a
    panel (fp64 / fp32, rows x >= n), ``V`` the whole block in natural row order (fp64, >= n rows),
    ``C_in`` fp64 or None (0; may be Y itself), ``active`` int32[ncols] or None (columns with 0 are
    neither computed nor written), ``colmax`` float64[ncols] or None (max |Y| over the real rows of
    each active column, NaN kept).  All are views with unit column stride; ``ncols`` defaults to
    Y's width (1..64, else ValueError)."""
    assert V.dtype == Y.dtype == torch.float64 and P.stride(-1) == 1 and V.stride(-1) == 1 and Y.stride(-1) == 1
    ncols = Y.shape[1] if ncols is None else int(ncols)
    cp, ldc = 0, 0
    if C_in is not None:
        assert C_in.dtype == torch.float64 and C_in.stride(-1) == 1
        cp, ldc = _p(C_in), C_in.stride(0)
    if active is not None:
        assert active.dtype == torch.int32 and active.is_contiguous()
    if colmax is not None:
        assert colmax.dtype == torch.float64 and colmax.is_contiguous()
    device_for(Y).panel_rhs(_DT[P.dtype], _p(P), P.stride(0), n, m, p, k, _p(V), V.stride(0), ncols, cp, ldc, _p(Y),
                            Y.stride(0), float(sign), 0 if active is None else _p(active),
                            0 if colmax is None else _p(colmax))
    return Y


def panel_rhs_dd(P: torch.Tensor, V: torch.Tensor, Y: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                 C_in: torch.Tensor = None, active: torch.Tensor = None, colmax: torch.Tensor = None,
                 ncols: int = None, device=None) -> torch.Tensor:
    """Y = round(C_in - P @ V) over the columns c < n (Device::panel_rhs_dd): the residual in twice the
    working precision.  The whole sum, C_in included, is carried as an unevaluated pair of doubles (Dot2)
    and rounded once, so |Y - exact| <= u |exact| + 4 ((n + 2) u)^2 (|C_in| + |P| |V|) with u = 2^-53.
    Operands as in panel_rhs, but ``P`` is fp64 (anything else is an error) and there is no sign.
    ``device``: the native executor to run on instead of the one of Y's torch device (e.g.
    ``native.async_host_device()`` for CPU tensors)."""
    assert V.dtype == Y.dtype == torch.float64 and P.stride(-1) == 1 and V.stride(-1) == 1 and Y.stride(-1) == 1
    ncols = Y.shape[1] if ncols is None else int(ncols)
    cp, ldc = 0, 0
    if C_in is not None:
        assert C_in.dtype == torch.float64 and C_in.stride(-1) == 1
        cp, ldc = _p(C_in), C_in.stride(0)
    if active is not None:
        assert active.dtype == torch.int32 and active.is_contiguous()
    if colmax is not None:
        assert colmax.dtype == torch.float64 and colmax.is_contiguous()
    (device or device_for(Y)).panel_rhs_dd(_DT[P.dtype], _p(P), P.stride(0), n, m, p, k, _p(V), V.stride(0), ncols,
                                           cp, ldc, _p(Y), Y.stride(0), 0 if active is None else _p(active),
                                           0 if colmax is None else _p(colmax))
    return Y


def gather_rows_natural(dst: torch.Tensor, src: torch.Tensor, n: int, m: int, p: int, ncols: int = None) -> torch.Tensor:
    """dst[g] = the row of global index g < n out of ``src``, the rank-major rows an all-gather
    delivers (ceil(Nr / p) * m rows per rank); rows >= n of dst are not written (fp64 views)."""
    assert dst.dtype == src.dtype == torch.float64 and dst.stride(-1) == 1 and src.stride(-1) == 1
    ncols = dst.shape[1] if ncols is None else int(ncols)
    device_for(dst).gather_rows_natural(_p(dst), dst.stride(0), _p(src), src.stride(0), n, m, p, ncols)
    return dst


def copy_cols_masked(dst: torch.Tensor, src: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """dst[:, j] = src[:, j] for the columns with mask[j] != 0 (fp64 views, int32 mask)."""
    assert dst.dtype == src.dtype == torch.float64 and dst.stride(-1) == 1 and src.stride(-1) == 1
    assert mask.dtype == torch.int32 and mask.is_contiguous() and dst.shape == src.shape
    device_for(dst).copy_cols_masked(_p(dst), dst.stride(0), _p(src), src.stride(0), dst.shape[0], dst.shape[1],
                                     _p(mask))
    return dst


def panel_rhs_t(P: torch.Tensor, V: torch.Tensor, S: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                active: torch.Tensor = None, ncols: int = None) -> torch.Tensor:
    """S[c, j] = sum over this rank's real local rows r of P[r, c] * V[grow(r), j] for c < n
    (Device::panel_rhs_t): rank ``k``'s term of P_full^T V.  ``P`` this rank's rows of a panel (fp64 /
    fp32, rows x >= n), ``V`` the whole block in natural row order (fp64, >= n rows; only the rows
    this rank owns are read), ``S`` fp64 with >= n rows, ``active`` int32[ncols] or None (a column
    with 0 is not computed and gets +0.0).  Views with unit column stride; ``ncols`` defaults to S's
    width (1..64, else an error)."""
    assert V.dtype == S.dtype == torch.float64 and P.stride(-1) == 1 and V.stride(-1) == 1 and S.stride(-1) == 1
    ncols = S.shape[1] if ncols is None else int(ncols)
    if active is not None:
        assert active.dtype == torch.int32 and active.is_contiguous()
    device_for(S).panel_rhs_t(_DT[P.dtype], _p(P), P.stride(0), n, m, p, k, _p(V), V.stride(0), ncols, _p(S),
                              S.stride(0), 0 if active is None else _p(active))
    return S


def panel_abs_rhs(P: torch.Tensor, V: torch.Tensor, Y: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                  C_in: torch.Tensor = None, colmax: torch.Tensor = None, ncols: int = None,
                  device=None) -> torch.Tensor:
    """Y = |C_in| + |P| @ |V| over the columns c < n (Device::panel_abs_rhs), in fp64 whatever P's dtype
    is (an fp32 element is widened exactly, V is not rounded).  Operands as in panel_rhs: ``P`` this
    rank's rows of a panel (fp64 / fp32), ``V`` the whole block in natural row order (fp64), ``C_in``
    fp64 or None (0; may be Y itself), ``colmax`` float64[ncols] or None (max |Y| over the real rows,
    NaN kept).  Padded local rows of Y get |C_in| (or 0).  ``ncols`` defaults to Y's width (1..64, else
    an error).  ``device``: the native executor to run on instead of the one of Y's torch device (e.g.
    ``native.async_host_device()`` for CPU tensors)."""
    assert V.dtype == Y.dtype == torch.float64 and P.stride(-1) == 1 and V.stride(-1) == 1 and Y.stride(-1) == 1
    ncols = Y.shape[1] if ncols is None else int(ncols)
    cp, ldc = 0, 0
    if C_in is not None:
        assert C_in.dtype == torch.float64 and C_in.stride(-1) == 1
        cp, ldc = _p(C_in), C_in.stride(0)
    if colmax is not None:
        assert colmax.dtype == torch.float64 and colmax.is_contiguous()
    (device or device_for(Y)).panel_abs_rhs(_DT[P.dtype], _p(P), P.stride(0), n, m, p, k, _p(V), V.stride(0), ncols,
                                            cp, ldc, _p(Y), Y.stride(0), 0 if colmax is None else _p(colmax))
    return Y


def panel_abs_rhs_t(P: torch.Tensor, V: torch.Tensor, S: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                    ncols: int = None, device=None) -> torch.Tensor:
    """S[c, j] = sum over this rank's real local rows r of |P[r, c]| * |V[grow(r), j]| for c < n
    (Device::panel_abs_rhs_t): rank ``k``'s term of |P_full|^T |V|, in fp64 whatever P's dtype is.
    Operands as in panel_rhs_t; rows >= n of ``S`` are not written, rows of ``V`` owned by other ranks
    are not read.  ``ncols`` defaults to S's width (1..64, else an error); ``device`` as in panel_abs_rhs."""
    assert V.dtype == S.dtype == torch.float64 and P.stride(-1) == 1 and V.stride(-1) == 1 and S.stride(-1) == 1
    ncols = S.shape[1] if ncols is None else int(ncols)
    (device or device_for(S)).panel_abs_rhs_t(_DT[P.dtype], _p(P), P.stride(0), n, m, p, k, _p(V), V.stride(0), ncols,
                                              _p(S), S.stride(0))
    return S


def bound_terms(R: torch.Tensor, D: torch.Tensor, G: torch.Tensor, berr: torch.Tensor, nz_eps: float, safe1: float,
                safe2: float, rows: int = None, ncols: int = None, device=None) -> torch.Tensor:
    """The elementwise step of LAPACK's xGERFS (Device::bound_terms) over fp64 views: G = |R| + nz_eps * D,
    plus safe1 where D <= safe2; berr[j] = max_r |R| / D, with (|R| + safe1) / (D + safe1) where
    D <= safe2, NaN kept (written, +0.0 for no rows).  ``G`` may be ``R``.  ``rows`` / ``ncols`` default to
    G's shape (ncols 1..64, else an error); ``device`` as in panel_abs_rhs."""
    assert R.dtype == D.dtype == G.dtype == berr.dtype == torch.float64 and berr.is_contiguous()
    assert R.stride(-1) == 1 and D.stride(-1) == 1 and G.stride(-1) == 1
    rows = G.shape[0] if rows is None else int(rows)
    ncols = G.shape[1] if ncols is None else int(ncols)
    (device or device_for(G)).bound_terms(_p(R), R.stride(0), _p(D), D.stride(0), _p(G), G.stride(0), rows, ncols,
                                          float(nz_eps), float(safe1), float(safe2), _p(berr))
    return G


def rank_update(X: torch.Tensor, W: torch.Tensor, Z: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                sign: float = 1.0, w_natural: bool = False, ncols: int = None) -> torch.Tensor:
    """X[r, c] += sign * sum_j W[wrow(r), j] * Z[c, j] over this rank's real local rows r and the columns
    c < n, in place (Device::rank_update): the sum in fp64, added to the widened element and rounded
    once to X's dtype.  ``X`` this rank's rows of a panel (fp64 / fp32, rows x >= n), ``W`` fp64 in
    local row order (``w_natural`` False: wrow(r) = r, what panel_rhs writes) or n x ncols in natural
    order (True: wrow(r) = the global row of r), ``Z`` fp64, n x ncols in natural order, ``sign`` +1 or
    -1.  Padding rows, columns >= n and pitch gaps of X are neither read nor written.  Views with unit
    column stride; ``ncols`` defaults to Z's width (1..64, else an error)."""
    assert W.dtype == Z.dtype == torch.float64 and X.stride(-1) == 1 and W.stride(-1) == 1 and Z.stride(-1) == 1
    ncols = Z.shape[1] if ncols is None else int(ncols)
    device_for(X).rank_update(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _p(W), W.stride(0), bool(w_natural),
                              _p(Z), Z.stride(0), ncols, float(sign))
    return X


def grad_matrix(P: torch.Tensor, W: torch.Tensor, Z: torch.Tensor, G: torch.Tensor, n: int, alpha: float = 0.0,
                sign: float = 1.0, accumulate: bool = False, ncols: int = None, device=None) -> torch.Tensor:
    """G[i, j] = (G[i, j] if accumulate else 0) + alpha * P[j, i] + sign * sum_c W[i, c] * Z[j, c] for i, j < n
    (Device::grad_matrix), in fp64 whatever P's dtype is: the gradient matrix of a solve or of a
    log-determinant from a resident inverse ``P`` (fp64 / fp32, n x n, natural row order), which enters
    transposed.  ``W`` and ``Z`` fp64, n x ncols in natural order, ``G`` fp64, ``sign`` +1 or -1.  ``alpha``
    == 0: P is never read and may be None; ``ncols`` == 0: W and Z are never read and may be None.
    Nothing of G outside n x n is written.  Views with unit column stride; ``ncols`` defaults to Z's width
    (0 without Z; 0..64, else an error); ``device`` as in panel_abs_rhs."""
    assert G.dtype == torch.float64 and G.stride(-1) == 1
    assert P is None or P.stride(-1) == 1
    assert (W is None) == (Z is None)
    if Z is not None:
        assert W.dtype == Z.dtype == torch.float64 and W.stride(-1) == 1 and Z.stride(-1) == 1
    ncols = (Z.shape[1] if Z is not None else 0) if ncols is None else int(ncols)
    dt = _DT[P.dtype] if P is not None else "fp64"
    (device or device_for(G)).grad_matrix(dt, 0 if P is None else _p(P), 0 if P is None else P.stride(0), int(n),
                                          float(alpha), 0 if W is None else _p(W), 0 if W is None else W.stride(0),
                                          0 if Z is None else _p(Z), 0 if Z is None else Z.stride(0), ncols,
                                          float(sign), bool(accumulate), _p(G), G.stride(0))
    return G


def axpy_cols_masked(Y: torch.Tensor, S: torch.Tensor, C_in: torch.Tensor = None, sign: float = 1.0,
                     active: torch.Tensor = None, colmax: torch.Tensor = None, ncols: int = None) -> torch.Tensor:
    """Y[:, j] = C_in[:, j] + sign * S[:, j] for the columns with active[j] != 0 (Device::axpy_cols_masked;
    fp64 views, ``C_in`` None = 0 or Y itself, ``active`` int32 or None = all), ``colmax[j]`` = max |Y[:, j]|
    with NaN kept; an inactive column's Y and colmax stay untouched.  ``ncols`` defaults to Y's width
    (1..64, else an error)."""
    assert Y.dtype == S.dtype == torch.float64 and Y.stride(-1) == 1 and S.stride(-1) == 1
    ncols = Y.shape[1] if ncols is None else int(ncols)
    cp, ldc = 0, 0
    if C_in is not None:
        assert C_in.dtype == torch.float64 and C_in.stride(-1) == 1
        cp, ldc = _p(C_in), C_in.stride(0)
    if active is not None:
        assert active.dtype == torch.int32 and active.is_contiguous()
    if colmax is not None:
        assert colmax.dtype == torch.float64 and colmax.is_contiguous()
    device_for(Y).axpy_cols_masked(_p(Y), Y.stride(0), cp, ldc, _p(S), S.stride(0), float(sign), Y.shape[0], ncols,
                                   0 if active is None else _p(active), 0 if colmax is None else _p(colmax))
    return Y


def col_abs_sum(X: torch.Tensor, out: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0) -> torch.Tensor:
    """out[c] = sum over this rank's real local rows of |X[r, c]| for c < n (Device::col_abs_sum):
    rank ``k``'s term of the column sums, accumulated in fp64 with NaN kept.  ``X`` fp64 / fp32 with
    unit column stride, ``out`` fp64, contiguous, >= n entries."""
    assert out.dtype == torch.float64 and out.is_contiguous() and X.stride(-1) == 1
    device_for(out).col_abs_sum(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _p(out))
    return out


def _exp_ptr(e, n: int) -> int:
    if e is None:
        return 0
    assert e.dtype == torch.int32 and e.stride(-1) == 1 and e.numel() >= n
    return _p(e)


def abs_max_rows(X: torch.Tensor, out_nat: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0) -> torch.Tensor:
    """out_nat[grow(r)] = max_{c<n} |X[r, c]| for rank ``k``'s real local rows r (Device::abs_max_rows);
    the other entries of ``out_nat`` (fp64, natural row order, >= n entries) stay untouched.  A NaN or an
    Inf entry counts as +Inf.  ``X`` fp64 / fp32 with unit column stride; padding is never read."""
    assert out_nat.dtype == torch.float64 and out_nat.stride(-1) == 1 and X.stride(-1) == 1
    device_for(out_nat).abs_max_rows(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _p(out_nat))
    return out_nat


def abs_max_cols(X: torch.Tensor, out: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0,
                 rexp_nat: torch.Tensor = None) -> torch.Tensor:
    """out[c] = max over rank ``k``'s real local rows of ldexp(|X[r, c]|, rexp_nat[grow(r)]) for c < n
    (Device::abs_max_cols): the column maxima of the row-scaled panel, written (a rank without rows
    writes +0.0), a NaN or an Inf entry counting as +Inf.  ``rexp_nat`` int32 in natural row order or
    None (all 0); only this rank's rows' entries are read."""
    assert out.dtype == torch.float64 and out.stride(-1) == 1 and X.stride(-1) == 1
    device_for(out).abs_max_cols(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _exp_ptr(rexp_nat, n), _p(out))
    return out


def scale_pow2(X: torch.Tensor, n: int, m: int, p: int = 1, k: int = 0, rexp_nat: torch.Tensor = None,
               cexp: torch.Tensor = None) -> torch.Tensor:
    """X[r, c] = ldexp(X[r, c], rexp_nat[grow(r)] + cexp[c]) over rank ``k``'s real local rows and the
    columns c < n, in place (Device::scale_pow2): exact unless the result leaves the dtype's normal
    range (one rounding on underflow, +-Inf on overflow); NaN, +-Inf and +-0 are kept.  ``rexp_nat`` /
    ``cexp`` int32 (natural row order / columns) or None (all 0).  Nothing else of X is written."""
    assert X.stride(-1) == 1
    device_for(X).scale_pow2(_DT[X.dtype], _p(X), X.stride(0), n, m, p, k, _exp_ptr(rexp_nat, n), _exp_ptr(cexp, n))
    return X


def slogdet_batch(blocks: torch.Tensor, which: torch.Tensor = None, sign: torch.Tensor = None,
                  logabs: torch.Tensor = None):
    """(sign, logabs) of the determinants of an (nb, m, m) batch (Device::slogdet_batch): an LU with
    partial pivoting in fp64 whatever the dtype (fp32 is widened exactly), sign = -1 / 0 / +1 and
    logabs = log|det| as fp64 tensors on the blocks' device; an exactly zero pivot gives (0, -inf), a
    NaN or Inf entry (NaN, NaN).  ``blocks`` fp64 / fp32, CPU or CUDA, each block contiguous; it is
    only read.  ``which`` (int32, nb): blocks with which[b] == 0 are skipped and their entries of
    ``sign`` / ``logabs`` (given by the caller, else new tensors of zeros) keep what they held."""
    assert blocks.ndim == 3 and blocks.shape[1] == blocks.shape[2] and blocks.shape[1] >= 1
    assert blocks.stride(2) == 1 and blocks.stride(1) == blocks.shape[1]
    nb, m = int(blocks.shape[0]), int(blocks.shape[1])
    stride = blocks.stride(0) if nb > 1 else m * m
    if sign is None:
        sign = torch.zeros(nb, dtype=torch.float64, device=blocks.device)
    if logabs is None:
        logabs = torch.zeros(nb, dtype=torch.float64, device=blocks.device)
    assert sign.dtype == logabs.dtype == torch.float64 and sign.is_contiguous() and logabs.is_contiguous()
    assert sign.numel() >= nb and logabs.numel() >= nb
    if which is not None:
        assert which.dtype == torch.int32 and which.is_contiguous() and which.numel() >= nb
    device_for(blocks).slogdet_batch(_DT[blocks.dtype], _p(blocks), stride, m, nb,
                                     0 if which is None else _p(which), _p(sign), _p(logabs))
    return sign, logabs


def _stack(t: torch.Tensor, what: str):
    """(nb, stride, ld) of a 3-D view with unit column stride; a stack of one matrix has any stride"""
    assert t.ndim == 3 and t.stride(2) == 1, f"{what}: a 3-D view with unit column stride"
    return int(t.shape[0]), int(t.stride(0)), int(t.stride(1))


def batch_pack(A64: torch.Tensor, Lt: torch.Tensor, norm: torch.Tensor, exp: torch.Tensor, m: int = None):
    """The stack's way into block_inverse (Device::batch_pack).  ``A64`` (nb, n, n) fp64, any strides with
    unit column stride; ``Lt`` an (m, >= nb * m) view of fp64 / fp32, m = max(n, 16) by default; ``norm``
    float64[nb], ``exp`` int32[nb].  norm[b] = ||A_b||_inf (NaN kept), exp[b] the power of two that brings it
    into [1, 2), Lt[c, b * m + r] = -ldexp(A_b[r, c], exp[b]) in Lt's dtype, with -I below order m."""
    nb, sa, lda = _stack(A64, "A64")
    n = int(A64.shape[1])
    assert A64.dtype == torch.float64 and A64.shape[2] == n
    m = max(n, 16) if m is None else int(m)
    assert Lt.ndim == 2 and Lt.stride(1) == 1 and Lt.shape[0] >= m and Lt.shape[1] >= nb * m
    assert norm.dtype == torch.float64 and norm.is_contiguous() and norm.numel() >= nb
    assert exp.dtype == torch.int32 and exp.is_contiguous() and exp.numel() >= nb
    device_for(Lt).batch_pack(_DT[Lt.dtype], _p(A64), sa, lda, n, m, nb, _p(Lt), Lt.stride(0), _p(norm), _p(exp))
    return Lt


def batch_unpack(inv_t: torch.Tensor, exp: torch.Tensor, valid: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """block_inverse's output as inverses of the unscaled stack (Device::batch_unpack).  ``inv_t`` (nb, m, m)
    contiguous, inv_t[b] = inv(As_b)^T; ``X`` (nb, n, n) of the same dtype, n <= m, any strides with unit
    column stride: X[b, i, j] = ldexp(inv_t[b, j, i], exp[b]), NaN where valid[b] == 0."""
    nb, sx, ldx = _stack(X, "X")
    n, m = int(X.shape[1]), int(inv_t.shape[1])
    assert inv_t.is_contiguous() and inv_t.shape == (nb, m, m) and inv_t.dtype == X.dtype and X.shape[2] == n
    assert exp.dtype == valid.dtype == torch.int32 and exp.is_contiguous() and valid.is_contiguous()
    device_for(X).batch_unpack(_DT[X.dtype], _p(inv_t), n, m, nb, _p(exp), _p(valid), _p(X), sx, ldx)
    return X


def batch_rhs(M: torch.Tensor, V: torch.Tensor, Y: torch.Tensor, C_in: torch.Tensor = None, sign: float = 1.0,
              active: torch.Tensor = None, colmax: torch.Tensor = None, device=None) -> torch.Tensor:
    """Y[b] = C_in[b] + sign * M[b] @ V[b] for a stack (Device::batch_rhs), in fp64 whatever M's dtype is.
    ``M`` (nb, n, n) fp64 / fp32, ``V`` / ``Y`` / ``C_in`` (nb, n, k) fp64 with 1 <= k <= 64 (else an
    error), all 3-D views with unit column stride; ``C_in`` None (0) or Y itself; ``active`` int32 (nb, k)
    or None: a column with 0 is neither read nor written; ``colmax`` float64 (nb, k) or None: max |Y| per
    (matrix, column), NaN kept, untouched for an inactive column.  ``device`` as in panel_abs_rhs."""
    nb, sm, ldm = _stack(M, "M")
    n, k = int(M.shape[1]), int(Y.shape[2])
    assert V.dtype == Y.dtype == torch.float64 and M.shape[2] == n
    assert V.shape == (nb, n, k) and Y.shape == (nb, n, k)
    _, sv, ldv = _stack(V, "V")
    _, sy, ldy = _stack(Y, "Y")
    cp, sc, ldc = 0, 0, 0
    if C_in is not None:
        assert C_in.dtype == torch.float64 and C_in.shape == Y.shape
        _, sc, ldc = _stack(C_in, "C_in")
        cp = _p(C_in)
    if active is not None:
        assert active.dtype == torch.int32 and active.is_contiguous() and active.numel() == nb * k
    if colmax is not None:
        assert colmax.dtype == torch.float64 and colmax.is_contiguous() and colmax.numel() == nb * k
    (device or device_for(Y)).batch_rhs(_DT[M.dtype], _p(M), sm, ldm, n, nb, _p(V), sv, ldv, k, cp, sc, ldc, _p(Y), sy,
                                        ldy, float(sign), 0 if active is None else _p(active),
                                        0 if colmax is None else _p(colmax))
    return Y
