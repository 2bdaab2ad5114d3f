"""Device::rank_update (csrc/include/gj/device.hpp) against its contract, on the host executor and on
the GPU (csrc/kernels/rank_update.hip).

    X[r][c] = round_dt(X[r][c] + sign * sum_{j<k} W[wrow(r)][j] * Z[c][j])
    for this rank's local rows r with global row grow(r) < n, and the columns c < n

Embedding (the method of test_rhs_trans_ops.py).  X is an interior view of a NaN-filled parent with a
leading dimension wider than the view, and NaN sits in every place the contract says is never read or
written: X's local padding rows, its columns >= n and its pitch gap; W's rows of padded local rows
and W's pitch gap; with w_natural, W's rows that other ranks own and its rows >= n; Z's rows >= n and
Z's pitch gap.  After the call every byte of the three parents outside X's real rows x n columns is
compared bitwise with a copy taken before.  The views of X are placed 16-byte aligned or not, the
two load paths of the GPU kernel, and the probe must say "vec" and "scalar" respectively.

Reference and bound.  The reference is the longdouble evaluation of the contract from the operands as
stored.  With u64 = 2^-53, u32 = 2^-24 and gamma(q) = q u64 / (1 - q u64):
    fp64  |got - ref| <= gamma(k + 1) (|X_in| + |W| |Z|^T)
    fp32  |got - ref| <= gamma(k + 1) (|X_in| + |W| |Z|^T) + u32 |ref|
Derived, not measured: k products summed in fp64 in some order (at most k roundings on any term),
one more for the addition to the widened element; fp32 adds the single rounding of the result.

Cases.  k in {1, 3, 4, 5, 16, 17, 63, 64} (every edge of a K step of 4 and of the 16-wide builds);
(n, m) = (200, 16) (npad 208), (130, 64), (256, 128), each at p = 1 and as ranks 0 and 2 of p = 3
(the row map; a rank whose last block is ragged; a rank with no rows at all); both dtypes.
w_natural, the sign and the alignment rotate over the cases so that every value of each meets every
k, shape and dtype (test_rotation_covers checks exactly that).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

LD = np.longdouble
SHAPES = [(n, m, p, r) for (n, m) in ((200, 16), (130, 64), (256, 128)) for (p, r) in ((1, 0), (3, 0), (3, 2))]
KS = [1, 3, 4, 5, 16, 17, 63, 64]
DTS = ("fp64", "fp32")
U64, U32 = LD(2) ** -53, LD(2) ** -24
_TD = {"fp64": torch.float64, "fp32": torch.float32}


def gamma(q):
    return q * U64 / (1 - q * U64)


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """X (rows x n, representable in dt), W (n x 64, natural order) and Z (n x 64); a case with k
    columns uses the first k.  Graded rows and columns: an absolute tolerance would hide some."""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rng = np.random.default_rng([37, n, m, p, rank])
    X = rng.uniform(-1, 1, (L["rows"], n)) * np.ldexp(1.0, (np.arange(n) * 7) % 13 - 6)[None, :]
    if dt == "fp32":
        X = X.astype(np.float32).astype(np.float64)
    W = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 9 - 4)[None, :]
    Z = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(n) * 3) % 11 - 5)[:, None]
    for a in (X, W, Z):
        a.setflags(write=False)
    return X, W, Z


@functools.lru_cache(maxsize=None)
def _reference(shape, dt, k, sign):
    """longdouble X_in + sign W Z^T and |X_in| + |W| |Z|^T over the real rows x n columns"""
    L = _layout(*shape)
    X, W, Z = _operands(shape, dt)
    own = L["grow"][L["real"]]
    Wr, Zk = W[own, :k].astype(LD), Z[:, :k].astype(LD)
    Xr = X[L["real"]].astype(LD)
    ref = Xr + LD(sign) * (Wr @ Zk.T)
    mag = np.abs(Xr) + np.abs(Wr) @ np.abs(Zk).T
    return ref, mag


def _embed(t, r0, c0, ld, device, extra_rows=5):
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), float("nan"), dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to(device)
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _run_case(device, shape, k, dt, w_natural, sign, aligned, w_nan=None, z_zero=None):
    """returns the real rows x n columns of X after the call (checked against the reference unless a
    NaN was planted)"""
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad, real, grow = L["rows"], L["npad"], L["real"], L["grow"]
    R = int(real.sum())
    X, W, Z = _operands(shape, dt)
    es = 8 if dt == "fp64" else 4
    # X: the panel is rows x npad; the columns >= n and the local padding rows are NaN
    Xfull = np.full((rows, npad), np.nan)
    Xfull[:, :n] = X
    Xfull[~real, :] = np.nan
    if aligned:
        c0, ldx = 16 // es * 2, -(-(npad + 24) // 4) * 4
    else:
        c0, ldx = 5, (npad + 11) | 1
    Xpar, Xv = _embed(torch.from_numpy(Xfull).to(_TD[dt]), 3, c0, ldx, device)
    assert (Xv.data_ptr() % 16 == 0 and (Xv.stride(0) * es) % 16 == 0) == aligned or rows == 0
    # W: natural order (the rows this rank owns, NaN elsewhere) or local order (NaN in padded rows)
    own = grow[real]
    if w_natural:
        Wfull = np.full((npad, k), np.nan)
        Wfull[own] = W[own, :k]
    else:
        Wfull = np.full((rows, k), np.nan)
        Wfull[real] = W[own, :k]
    Zfull = np.full((npad, k), np.nan)
    Zfull[:n] = Z[:, :k]
    if w_nan is not None:  # (local real row index, column): NaN in W behind a zero of Z
        (Wfull[own[w_nan[0]]] if w_natural else Wfull[np.nonzero(real)[0][w_nan[0]]])[w_nan[1]] = np.nan
        Zfull[z_zero, w_nan[1]] = 0.0
    Wpar, Wv = _embed(torch.from_numpy(Wfull), 2, 3, k + (8 if aligned else 7), device)
    Zpar, Zv = _embed(torch.from_numpy(Zfull), 1, 2, k + (6 if aligned else 9), device)
    before = {nm: _bits(t) for nm, t in (("X", Xpar), ("W", Wpar), ("Z", Zpar))}

    ops.rank_update(Xv, Wv, Zv, n, m, p, rank, sign=sign, w_natural=w_natural, ncols=k)
    name = native.last_rank_update_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        exp = f"rku{-(-k // 4) * 4}:{'f64' if dt == 'fp64' else 'f32'}:{'vec' if aligned else 'scalar'}"
        assert name == exp or (rows == 0 and name.startswith(exp.rsplit(":", 1)[0])), (name, exp)

    # W and Z untouched; of X nothing but the real rows x n columns written (the real rows are a prefix)
    for nm, par in (("W", Wpar), ("Z", Zpar)):
        assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    a, b = _bits(Xpar).clone(), before["X"].clone()
    a[3:3 + R, c0:c0 + n] = 0
    b[3:3 + R, c0:c0 + n] = 0
    assert torch.equal(a, b), "write outside X's real rows x n columns"
    got = Xv[:R, :n].cpu().numpy().astype(np.float64)
    if w_nan is not None:
        return got
    ref, mag = _reference(shape, dt, k, float(sign))
    err = np.abs(got.astype(LD) - ref)
    bound = gamma(LD(k + 1)) * mag + (U32 * np.abs(ref) if dt == "fp32" else 0)
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (float((err / np.maximum(bound, LD(1e-300))).max()), k)
    if R:  # a no-op would pass a bound of this size only by accident: the update must show
        assert float(np.abs(got - X[real]).max()) > 0
    return got


_FLAGS = list(itertools.product([False, True], [1.0, -1.0], [True, False]))  # w_natural, sign, aligned
_CASES = [(s, k, dt) for s in SHAPES for k in KS for dt in DTS]


def _rot_index(case):
    return SHAPES.index(case[0]) + 3 * KS.index(case[1]) + 5 * DTS.index(case[2]) + KS.index(case[1]) // 4


def _rotation(i):
    return _FLAGS[i % 8]


def _id(c):
    s = c[0]
    return f"n{s[0]}m{s[1]}p{s[2]}r{s[3]}-k{c[1]}-{c[2]}"


def test_rotation_covers():
    """every value of w_natural, the sign and the alignment meets every k, shape and dtype"""
    for f in range(3):
        for v in {c[f] for c in _CASES}:
            seen = {_rotation(_rot_index(c)) for c in _CASES if c[f] == v}
            for flag in range(3):
                assert len({s[flag] for s in seen}) == 2, (f, v, flag)


@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_rank_update_host(case):
    _run_case("cpu", *case, *_rotation(_rot_index(case)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_rank_update_gpu(case):
    _run_case("cuda", *case, *_rotation(_rot_index(case)))


# the flags the rotation gives a case once, in full for one ragged multi-rank shape
_FULL = [((200, 16, 3, 0), k, dt, *fl) for k in (5, 64) for dt in DTS for fl in _FLAGS]


@pytest.mark.parametrize("case", _FULL, ids=lambda c: f"k{c[1]}-{c[2]}-nat{int(c[3])}-s{int(c[4])}-al{int(c[5])}")
def test_rank_update_flags_host(case):
    _run_case("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _FULL, ids=lambda c: f"k{c[1]}-{c[2]}-nat{int(c[3])}-s{int(c[4])}-al{int(c[5])}")
def test_rank_update_flags_gpu(case):
    _run_case("cuda", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_rank_update_gpu_bit_identical(dt):
    for shape, k, nat, aligned in (((200, 16, 3, 0), 17, True, False), ((256, 128, 1, 0), 64, False, True)):
        a = _run_case("cuda", shape, k, dt, nat, -1.0, aligned)
        b = _run_case("cuda", shape, k, dt, nat, -1.0, aligned)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), "two launches differ"


def _bad_k(device):
    n, m = 64, 16
    X = torch.zeros((n, n), dtype=torch.float64, device=device)
    W = torch.ones((n, 80), dtype=torch.float64, device=device)
    Z = torch.ones((n, 80), dtype=torch.float64, device=device)
    for k in (0, 65):
        with pytest.raises(RuntimeError):
            ops.rank_update(X, W, Z, n, m, ncols=k)
    assert float(X.abs().max()) == 0.0
    ops.rank_update(X, W, Z, n, m, ncols=64)
    assert float((X - 64.0).abs().max()) == 0.0


def test_bad_k_host():
    _bad_k("cpu")


@pytest.mark.gpu
def test_bad_k_gpu():
    _bad_k("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_huge_leading_dimension_refused_gpu(dt):
    # a leading dimension whose 64-row tile 32-bit byte offsets cannot span is refused, not computed
    # wrongly (one row, n = m = 1: the view is valid whatever its row stride)
    es = 8 if dt == "fp64" else 4
    X = torch.zeros((1, 1), dtype=_TD[dt], device="cuda")
    W = torch.ones((1, 1), dtype=torch.float64, device="cuda")
    limit = (2 ** 31 // es - 64) // 63
    with pytest.raises(RuntimeError):
        ops.rank_update(X.as_strided((1, 1), (limit + 1, 1)), W, W, 1, 1)
    assert float(X[0, 0]) == 0.0
    ops.rank_update(X.as_strided((1, 1), (limit, 1)), W, W, 1, 1)
    assert float(X[0, 0]) == 1.0


def _nan_case(device):
    # a NaN of W, in a row this rank owns, meets an exact zero of Z: 0 * NaN = NaN, so the whole row
    # of X becomes NaN and no other row does (the NaN everywhere else never shows: _run_case)
    shape = (200, 16, 3, 0)
    for dt, nat, k in (("fp64", False, 5), ("fp32", True, 17)):
        got = _run_case(device, shape, k, dt, nat, 1.0, dt == "fp64", w_nan=(7, 2), z_zero=11)
        assert np.isnan(got[7]).all(), "a NaN of W did not reach its row (column 11: through a zero of Z)"
        assert np.isfinite(np.delete(got, 7, axis=0)).all()


def test_nan_through_zero_host():
    _nan_case("cpu")


@pytest.mark.gpu
def test_nan_through_zero_gpu():
    _nan_case("cuda")
