"""Device::grad_matrix (csrc/include/gj/device.hpp) against its contract, on the host executor and on
the GPU (csrc/kernels/grad_matrix.hip).

    G[i][j] = (accumulate ? G[i][j] : 0) + alpha * (double)P[j][i] + sign * sum_{c<k} W[i][c] * Z[j][c]
    for i < n and j < n

Embedding (the method of test_rank_update_ops.py).  P, W, Z and G are interior views of NaN-filled
parents with leading dimensions wider than the views, so NaN sits in every place the contract says is
never read or written: the rows and columns >= n of P, W, Z and G, the columns >= k of W and Z and
every pitch gap; without accumulate G's own n x n is NaN too (it is never read then).  After the call
every byte of the four parents outside G's n x n is compared bitwise with a copy taken before.  The
views of G (and of P with it) are placed 16-byte aligned or not, the two paths of the GPU kernel, and
the probe must say "vec" and "scalar" respectively.

Reference and bound.  The reference is the longdouble evaluation of the contract from the operands as
stored.  With u = 2^-53 and gamma(q) = q u / (1 - q u), in fp64 units for both dtypes (an fp32
element of P is widened exactly and nothing is rounded to fp32):
    |got - ref| <= gamma(k + 3) (|G_in| + |alpha| |P|^T + |W| |Z|^T)
Derived, not measured: k products summed in fp64 in some order (at most k roundings on any term), one
rounding for alpha * P, one for adding the sum to it, one for adding G.  Both executors compute in
that order (the sum; alpha * P; their sum; G + that), so no term sees more than k + 3 roundings.

Cases.  n in {1, 63, 64, 65, 130, 257} (a tile edge on each side; more than one tile, so that tile
(a, b) != (b, a); a ragged last tile), k in {0, 1, 3, 4, 5, 16, 17, 63, 64} (no product; every edge of
a K step of 4 and of the builds), alpha in {0, 1, -0.375}.  P is not symmetric and W != Z, so a missing
or doubled transposition cannot cancel.  The sign, accumulate, the alignment and the dtype rotate over
the cases so that every value of each meets every n and every k (test_rotation_covers checks exactly
that).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

LD = np.longdouble
NS = [1, 63, 64, 65, 130, 257]
KS = [0, 1, 3, 4, 5, 16, 17, 63, 64]
ALPHAS = [0.0, 1.0, -0.375]
DTS = ("fp64", "fp32")
U64 = LD(2) ** -53
_TD = {"fp64": torch.float64, "fp32": torch.float32}


def gamma(q):
    return q * U64 / (1 - q * U64)


@functools.lru_cache(maxsize=None)
def _operands(n, dt):
    """P (n x n, representable in dt, not symmetric), W and Z (n x 64, W != Z) and G_in (n x n); a case
    with k columns uses the first k.  Graded rows and columns: an absolute tolerance would hide some."""
    rng = np.random.default_rng([41, n])
    P = rng.uniform(-1, 1, (n, n)) * np.ldexp(1.0, (np.arange(n) * 7) % 13 - 6)[None, :]
    if dt == "fp32":
        P = P.astype(np.float32).astype(np.float64)
    W = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 9 - 4)[None, :]
    Z = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(n) * 3) % 11 - 5)[:, None]
    Gin = rng.uniform(-1, 1, (n, n)) * np.ldexp(1.0, (np.arange(n) * 5) % 7 - 3)[:, None]
    for a in (P, W, Z, Gin):
        a.setflags(write=False)
    return P, W, Z, Gin


@functools.lru_cache(maxsize=None)
def _reference(n, dt, k, alpha, sign, accumulate):
    """longdouble (G_in) + alpha P^T + sign W Z^T and (|G_in|) + |alpha| |P|^T + |W| |Z|^T"""
    P, W, Z, Gin = _operands(n, dt)
    Wk, Zk = W[:, :k].astype(LD), Z[:, :k].astype(LD)
    ref = LD(alpha) * P.T.astype(LD) + LD(sign) * (Wk @ Zk.T)
    mag = abs(LD(alpha)) * np.abs(P.T).astype(LD) + np.abs(Wk) @ np.abs(Zk).T
    if accumulate:
        ref = ref + Gin.astype(LD)
        mag = mag + np.abs(Gin).astype(LD)
    return ref, mag


def _embed(t, r0, c0, ld, device, extra_rows=3):
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), float("nan"), dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to(device)
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _run_case(device, n, k, alpha, sign, accumulate, aligned, dt, p_mode="view", wz_null=False, w_nan=None,
              z_nan=None, p_aligned=None):
    """returns G's n x n after the call (checked against the reference unless a NaN was planted).
    p_mode: "view" | "nan" (all NaN) | "null"; w_nan / z_nan = (row, column, row of the other factor
    whose entry in that column is set to 0)"""
    native = gj.load_native()
    P, W, Z, Gin = _operands(n, dt)
    es = 8 if dt == "fp64" else 4
    p_aligned = aligned if p_aligned is None else p_aligned
    Wk, Zk = W[:, :k].copy(), Z[:, :k].copy()
    if w_nan is not None:
        Wk[w_nan[0], w_nan[1]] = np.nan
        Zk[w_nan[2], w_nan[1]] = 0.0
    if z_nan is not None:
        Zk[z_nan[0], z_nan[1]] = np.nan
        Wk[z_nan[2], z_nan[1]] = 0.0
    # P: n x n inside a NaN parent
    if p_aligned:
        pc0, ldp = 16 // es * 2, -(-(n + 24) // 4) * 4
    else:
        pc0, ldp = 5, (n + 11) | 1
    Pval = np.full((n, n), np.nan) if p_mode == "nan" else P
    Ppar, Pv = _embed(torch.from_numpy(np.array(Pval)).to(_TD[dt]), 3, pc0, ldp, device)
    # G: n x n inside a NaN parent; its own values only when accumulating (never read otherwise)
    if aligned:
        gc0, ldg = 4, -(-(n + 10) // 2) * 2
    else:
        gc0, ldg = 3, (n + 9) | 1
    Gpar, Gv = _embed(torch.from_numpy(np.array(Gin) if accumulate else np.full((n, n), np.nan)), 2, gc0, ldg, device)
    assert (Gv.data_ptr() % 16 == 0 and (Gv.stride(0) * 8) % 16 == 0) == aligned
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * es) % 16 == 0) == p_aligned
    # W, Z: n x k inside NaN parents (k = 0: a NaN column that ncols = 0 must keep unread)
    Wpar, Wv = _embed(torch.from_numpy(Wk if k else np.full((n, 1), np.nan)), 2, 3, max(k, 1) + (8 if aligned else 7),
                      device)
    Zpar, Zv = _embed(torch.from_numpy(Zk if k else np.full((n, 1), np.nan)), 1, 2, max(k, 1) + (6 if aligned else 9),
                      device)
    parents = (("P", Ppar), ("W", Wpar), ("Z", Zpar), ("G", Gpar))
    before = {nm: _bits(t) for nm, t in parents}

    ops.grad_matrix(None if p_mode == "null" else Pv, None if wz_null else Wv, None if wz_null else Zv, Gv, n,
                    alpha=alpha, sign=sign, accumulate=accumulate, ncols=k)
    name = native.last_grad_matrix_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        tag = "nop" if alpha == 0 else ("f64" if dt == "fp64" or p_mode == "null" else "f32")
        vec = aligned and (alpha == 0 or p_aligned)
        assert name == f"gm{-(-k // 4) * 4}:{tag}:{'vec' if vec else 'scalar'}", name

    for nm, par in parents[:3]:
        assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    a, b = _bits(Gpar).clone(), before["G"].clone()
    a[2:2 + n, gc0:gc0 + n] = 0
    b[2:2 + n, gc0:gc0 + n] = 0
    assert torch.equal(a, b), "write outside G's n x n"
    got = Gv.cpu().numpy().astype(np.float64)
    if w_nan is not None or z_nan is not None:
        return got
    ref, mag = _reference(n, dt, k, float(alpha), float(sign), bool(accumulate))
    err = np.abs(got.astype(LD) - ref)
    bound = gamma(LD(k + 3)) * mag
    assert np.isfinite(got).all()
    print(f"n={n} k={k} alpha={alpha}: max err / bound = {float((err / np.maximum(bound, LD(1e-300))).max()):.3f}")
    assert (err <= bound).all(), (float((err / np.maximum(bound, LD(1e-300))).max()), n, k)
    if alpha == 0 and k == 0 and not accumulate:  # +0.0, bit for bit
        assert not got.view(np.int64).any()
    elif alpha != 0 or k:  # a no-op would pass a bound of this size only by accident: both terms must show
        base = Gin if accumulate else np.zeros((n, n))
        assert float(np.abs(got - base).max()) > 0
    return got


_FLAGS = list(itertools.product([1.0, -1.0], [False, True], [True, False], DTS))  # sign, accumulate, aligned, dtype
_CASES = [(n, k, al) for n in NS for k in KS for al in ALPHAS]


def _rot_index(case):
    ni, ki, ai = NS.index(case[0]), KS.index(case[1]), ALPHAS.index(case[2])
    return 3 * ni + 5 * ki + 7 * ai + ki // 3


def _rotation(i):
    return _FLAGS[i % 16]


def _id(c):
    return f"n{c[0]}-k{c[1]}-a{c[2]}"


def test_rotation_covers():
    """every value of the sign, accumulate, the alignment and the dtype meets every n and every k"""
    for f in range(2):
        for v in {c[f] for c in _CASES}:
            seen = {_rotation(_rot_index(c)) for c in _CASES if c[f] == v}
            for flag in range(4):
                assert len({s[flag] for s in seen}) == 2, (f, v, flag)
    # and both values of each meet a non-zero alpha with k > 0 (both terms at once)
    seen = {_rotation(_rot_index(c)) for c in _CASES if c[1] > 0 and c[2] != 0}
    assert len(seen) == 16


@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_grad_matrix_host(case):
    _run_case("cpu", *case, *_rotation(_rot_index(case)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_grad_matrix_gpu(case):
    _run_case("cuda", *case, *_rotation(_rot_index(case)))


# the flags the rotation gives a case once, in full for one ragged multi-tile shape
_FULL = [(130, k, al, *fl) for (k, al) in ((5, -0.375), (64, 1.0)) for fl in _FLAGS]
_full_id = lambda c: f"k{c[1]}-a{c[2]}-s{int(c[3])}-acc{int(c[4])}-al{int(c[5])}-{c[6]}"  # noqa: E731


@pytest.mark.parametrize("case", _FULL, ids=_full_id)
def test_grad_matrix_flags_host(case):
    _run_case("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _FULL, ids=_full_id)
def test_grad_matrix_flags_gpu(case):
    _run_case("cuda", *case)


def _alpha_zero(device):
    # alpha == 0: P is never read -- all NaN, or null -- and the result is finite and correct
    for dt, aligned, mode in (("fp64", True, "nan"), ("fp32", False, "nan"), ("fp64", True, "null"),
                              ("fp64", False, "null")):
        for k, acc in ((0, False), (17, True), (64, False)):
            _run_case(device, 130, k, 0.0, -1.0, acc, aligned, dt, p_mode=mode)


def test_alpha_zero_p_unread_host():
    _alpha_zero("cpu")


@pytest.mark.gpu
def test_alpha_zero_p_unread_gpu():
    _alpha_zero("cuda")


def _k_zero(device):
    # k == 0: W and Z are never read -- null
    for dt, aligned, acc in (("fp64", True, False), ("fp32", False, True), ("fp32", True, False)):
        _run_case(device, 65, 0, -0.375, 1.0, acc, aligned, dt, wz_null=True)
    _run_case(device, 65, 0, 0.0, 1.0, False, True, "fp64", p_mode="null", wz_null=True)


def test_k_zero_wz_null_host():
    _k_zero("cpu")


@pytest.mark.gpu
def test_k_zero_wz_null_gpu():
    _k_zero("cuda")


@pytest.mark.gpu
def test_mixed_alignment_gpu():
    # G aligned, P not: the element path (and correct); with alpha == 0 P's alignment does not count
    _run_case("cuda", 130, 17, 1.0, 1.0, False, True, "fp32", p_aligned=False)
    _run_case("cuda", 130, 17, 0.0, 1.0, False, True, "fp32", p_aligned=False)


def _nan_case(device):
    # a NaN of W[i][c] meets an exact zero of Z[j][c]: 0 * NaN = NaN, so the whole row i of G becomes NaN
    # and no other row does; a NaN of Z[j][c] likewise reaches exactly column j, also through a zero of W
    n = 130
    for dt, aligned, k, alpha in (("fp64", True, 5, 1.0), ("fp32", False, 17, 0.0)):
        got = _run_case(device, n, k, alpha, 1.0, True, aligned, dt, w_nan=(70, 2, 11))
        assert np.isnan(got[70]).all(), "a NaN of W did not reach its row (column 11: through a zero of Z)"
        assert np.isfinite(np.delete(got, 70, axis=0)).all()
        got = _run_case(device, n, k, alpha, -1.0, False, aligned, dt, z_nan=(99, 3, 5))
        assert np.isnan(got[:, 99]).all(), "a NaN of Z did not reach its column (row 5: through a zero of W)"
        assert np.isfinite(np.delete(got, 99, axis=1)).all()


def test_nan_through_zero_host():
    _nan_case("cpu")


@pytest.mark.gpu
def test_nan_through_zero_gpu():
    _nan_case("cuda")


def _bad_k(device):
    n = 64
    P = torch.zeros((n, n), dtype=torch.float64, device=device)
    G = torch.zeros((n, n), dtype=torch.float64, device=device)
    W = torch.ones((n, 80), dtype=torch.float64, device=device)
    Z = torch.ones((n, 80), dtype=torch.float64, device=device)
    for k in (65, -1):
        with pytest.raises(RuntimeError) as ei:
            ops.grad_matrix(P, W, Z, G, n, alpha=1.0, ncols=k)
        assert ei.value.status == 5  # Status::BadArgs
    with pytest.raises(RuntimeError) as ei:
        ops.grad_matrix(P, W, Z, G, -1, alpha=1.0, ncols=1)
    assert ei.value.status == 5
    assert float(G.abs().max()) == 0.0
    ops.grad_matrix(P, W, Z, G, n, alpha=1.0, ncols=64)
    assert float((G - 64.0).abs().max()) == 0.0


def test_bad_k_host():
    _bad_k("cpu")


@pytest.mark.gpu
def test_bad_k_gpu():
    _bad_k("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_grad_matrix_gpu_bit_identical(dt):
    for n, k, alpha, acc, aligned in ((257, 17, -0.375, True, False), (130, 64, 1.0, False, True)):
        a = _run_case("cuda", n, k, alpha, -1.0, acc, aligned, dt)
        b = _run_case("cuda", n, k, alpha, -1.0, acc, aligned, dt)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), "two launches differ"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_gpu_and_host_agree(dt):
    # within the sum of their bounds
    for n, k, alpha, acc, aligned in ((257, 63, -0.375, True, True), (65, 5, 1.0, False, False)):
        g = _run_case("cuda", n, k, alpha, 1.0, acc, aligned, dt)
        h = _run_case("cpu", n, k, alpha, 1.0, acc, aligned, dt)
        _, mag = _reference(n, dt, k, alpha, 1.0, acc)
        assert (np.abs(g.astype(LD) - h.astype(LD)) <= 2 * gamma(LD(k + 3)) * mag).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_huge_leading_dimension_refused_gpu(dt):
    # a leading dimension of G or of P whose 64-row tile 32-bit byte offsets cannot span is refused, not
    # computed wrongly (n = 1: the view is valid whatever its row stride)
    es = 8 if dt == "fp64" else 4
    G = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    P = torch.ones((1, 1), dtype=_TD[dt], device="cuda")
    W = torch.ones((1, 1), dtype=torch.float64, device="cuda")
    glim, plim = (2 ** 31 // 8 - 64) // 63, (2 ** 31 // es - 64) // 63
    with pytest.raises(RuntimeError):
        ops.grad_matrix(P, W, W, G.as_strided((1, 1), (glim + 1, 1)), 1, alpha=1.0)
    with pytest.raises(RuntimeError):
        ops.grad_matrix(P.as_strided((1, 1), (plim + 1, 1)), W, W, G, 1, alpha=1.0)
    assert float(G[0, 0]) == 0.0
    ops.grad_matrix(P.as_strided((1, 1), (plim, 1)), W, W, G.as_strided((1, 1), (glim, 1)), 1, alpha=1.0)
    assert float(G[0, 0]) == 2.0
