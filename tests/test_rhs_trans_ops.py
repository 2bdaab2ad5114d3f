"""Device::panel_rhs_t, axpy_cols_masked and col_abs_sum (csrc/include/gj/device.hpp) against their
contract, on the host executor and on the GPU (csrc/kernels/panel_rhs_t.hip).

panel_rhs_t: S[c][j] = sum over this rank's real local rows r of P[r][c] V[grow(r)][j], c < n, j < k.

Embedding (the method of test_rhs_block_ops.py).  Every operand is an interior view of a NaN-filled
parent with a leading dimension wider than the view; what the contract says is never read holds NaN
as well: the padding columns of P (c >= n), P's local padding rows (global row >= n), the rows >= n
of V, the rows of V that other ranks own, and every pitch gap.  S, Y, out and colmax sit inside a
sentinel-filled parent; after the call every byte outside the writable set (S: the rows < n and
columns < k of the view) is compared with a copy taken before.  The views of P are placed 16-byte
aligned or not ("vec" / "scalar"), the two load paths of the GPU kernel.

Reference and bounds.  The reference is the longdouble product from the operands as stored (fp32:
V rounded to fp32 first, as the op does on load).  With R the rank's real rows, u = 2^-53 (fp64) or
2^-24 (fp32) and gamma(q) = q u / (1 - q u):
    panel_rhs_t       |got - ref| <= gamma(R + 1) (|P|^T |V|)
    col_abs_sum       |got - ref| <= gamma(R + 1) ref
    axpy_cols_masked  |got - ref| <= u (|C_in| + |S|)        (one rounding of an exact operand pair)
Derived, not measured: an element is R multiply-adds in some order (a chain per row slice on the
matrix cores, then the slices summed in fp64: never more than R roundings on any term); one more u
covers the longdouble reference's own error.

Cases.  (n, m, p, rank) = (300, 16, 1, 0), (1003, 59, 3, each rank), (1000, 59, 3, 1) (the ragged
last block on an odd npad) and (2048, 128, 1, 0); k in {1, 5, 16, 17, 40, 64}; both dtypes; on the GPU
the row split forced to 1, 2, 7 and automatic.  The active mask (null / some columns off) and the
alignment rotate over the cases so that every value of each meets every k, shape and split
(test_rotation_covers checks exactly that); axpy_cols_masked runs the full product of sign, C_in mode
(null / aliasing Y / separate) and mask with every k.  Every GPU case asserts
native.last_rhs_t_kernel().
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

LD = np.longdouble
SENT = -777.25
SHAPES = [(300, 16, 1, 0), (1003, 59, 3, 0), (1003, 59, 3, 1), (1003, 59, 3, 2), (1000, 59, 3, 1),
          (2048, 128, 1, 0)]
KS = [1, 5, 16, 17, 40, 64]
SPLITS = [1, 2, 7, 0]
CIN_MODES = ["null", "alias", "separate"]
_U = {"fp64": LD(2) ** -53, "fp32": LD(2) ** -24}
_TD = {"fp64": torch.float64, "fp32": torch.float32}


def gamma(q, u):
    return q * u / (1 - q * u)


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """P (rows x n), V (n x 64) and, in longdouble, P_real^T V_owned and |P_real|^T |V_owned| (computed
    once per shape and dtype with all 64 columns; a case with k columns uses the first k)."""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rng = np.random.default_rng([29, n, m, p, rank])
    P = rng.uniform(-1, 1, (L["rows"], n))
    # graded rows and columns: an absolute tolerance would hide whole columns
    P *= np.ldexp(1.0, (np.arange(n) * 7) % 21 - 10)[None, :]
    V = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 17 - 8)[None, :]
    if dt == "fp32":
        P = P.astype(np.float32).astype(np.float64)
    Vop = V.astype(np.float32).astype(np.float64) if dt == "fp32" else V
    real, grow = L["real"], L["grow"]
    Pr, Vr = P[real], Vop[grow[real]]
    prod = Pr.T.astype(LD) @ Vr.astype(LD)
    absprod = np.abs(Pr).T.astype(LD) @ np.abs(Vr).astype(LD)
    for x in (P, V, prod, absprod):
        x.setflags(write=False)
    return P, V, prod, absprod


def _embed(t, r0, c0, ld, fill, device, extra_rows=9):
    """t as an interior view of a `fill`-filled parent with leading dimension ld"""
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), fill, dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to(device)
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _outside_equal(par, before, r0, nr, c0, nc):
    a, b = _bits(par).clone(), before.clone()
    a[r0:r0 + nr, c0:c0 + nc] = 0
    b[r0:r0 + nr, c0:c0 + nc] = 0
    return torch.equal(a, b)


def _expected_name(dt, k, P, split, real):
    kw = 16 if k <= 16 else 32 if k <= 32 else 64
    vec = P.data_ptr() % 16 == 0 and (P.stride(0) * P.element_size()) % 16 == 0
    head = f"rhst{kw}:{'f64' if dt == 'fp64' else 'f32'}:{'vec' if vec else 'scalar'}:s"
    if split == 0:
        return head
    # a forced split runs whole steps of 4 rows and no empty slice
    chunk = max(-(-(-(-real // split)) // 4) * 4, 4)
    return head + str(max(-(-real // chunk), 1))


def _place_P(shape, dt, aligned, device):
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad = L["rows"], L["npad"]
    P = _operands(shape, dt)[0]
    es = 8 if dt == "fp64" else 4
    # the panel is rows x npad; columns >= n and local padding rows are NaN
    Pfull = np.full((rows, npad), np.nan)
    Pfull[:, :n] = P
    Pfull[~L["real"], :] = np.nan
    if aligned:
        c0, ldp = 16 // es * 2, -(-(npad + 24) // 4) * 4
    else:
        c0, ldp = 5, (npad + 11) | 1
    Ppar, Pv = _embed(torch.from_numpy(Pfull).to(_TD[dt]), 3, c0, ldp, float("nan"), device)
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * es) % 16 == 0) == aligned
    return Ppar, Pv


def _run_case(device, shape, k, dt, masked, aligned, split=0, twice=False, v_nan=None):
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    npad = L["npad"]
    R = int(L["real"].sum())
    _, V, prod, absprod = _operands(shape, dt)
    Ppar, Pv = _place_P(shape, dt, aligned, device)
    # V: the rows this rank owns; the rows of other ranks and the rows >= n are NaN
    Vfull = np.full((npad, k), np.nan)
    own = L["grow"][L["real"]]
    Vfull[own] = V[own, :k]
    if v_nan is not None:
        Vfull[v_nan] = np.nan
    Vpar, Vv = _embed(torch.from_numpy(Vfull), 2, 3, k + 7, float("nan"), device)
    # S: npad rows in view, of which the first n are writable
    Spar, Sv = _embed(torch.full((npad, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
    on = np.ones(k, dtype=bool)
    if masked:
        on[::3] = False  # column 0 off, also at k = 1
    active = torch.from_numpy(on.astype(np.int32)).to(device) if masked else None
    before = {nm: _bits(t) for nm, t in (("P", Ppar), ("V", Vpar), ("S", Spar))}

    def launch():
        if device != "cpu":
            native.set_rhs_t_split(split)
        try:
            ops.panel_rhs_t(Pv, Vv, Sv, n, m, p, rank, active=active, ncols=k)
        finally:
            if device != "cpu":
                native.set_rhs_t_split(0)

    launch()
    name = native.last_rhs_t_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        exp = _expected_name(dt, k, Pv, split, R)
        assert name == exp if split else (name.startswith(exp) and name[len(exp):].isdigit()), (name, exp)
    got = Sv.cpu().numpy().copy()
    if twice:
        s1 = _bits(Spar)
        launch()
        assert torch.equal(_bits(Spar), s1), "two runs differ"

    # inputs untouched; nothing but the rows < n, columns < k of S written
    for nm, par in (("P", Ppar), ("V", Vpar)):
        assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    assert _outside_equal(Spar, before["S"], 8, n, 5, k), "write outside S"
    # inactive columns: exactly +0.0
    assert (got[:n][:, ~on].view(np.int64) == 0).all()
    if v_nan is not None:
        return got[:n]
    ref = prod[:, :k]
    err = np.abs(got[:n].astype(LD) - ref)
    bound = gamma(LD(R + 1), _U[dt]) * absprod[:, :k]
    ok = err <= bound
    assert ok[:, on].all(), (float((err / np.maximum(absprod[:, :k], LD(1e-300)) / _U[dt])[:, on].max()), R + 1)
    assert np.isfinite(got[:n][:, on]).all()
    return got[:n]


def _rotation(i):
    """masked, aligned for rotation index i: the 4 combinations in turn"""
    return list(itertools.product([False, True], [True, False]))[i % 4]


_HOST_CASES = [(s, k, dt) for s in SHAPES for k in KS for dt in ("fp64", "fp32")]
_GPU_CASES = [(s, k, dt, sp) for s in SHAPES for k in KS for dt in ("fp64", "fp32") for sp in SPLITS]


def _rot_index(case):
    i = SHAPES.index(case[0]) + KS.index(case[1]) + 2 * ("fp64", "fp32").index(case[2])
    return i + (SPLITS.index(case[3]) if len(case) > 3 else 0)


def _id(c):
    s = c[0]
    tail = "" if len(c) < 4 else f"-split{c[3]}"
    return f"n{s[0]}m{s[1]}p{s[2]}r{s[3]}-k{c[1]}-{c[2]}{tail}"


def test_rotation_covers():
    """every value of the mask and the alignment meets every k, shape, dtype and split"""
    for cases, fields in ((_HOST_CASES, 3), (_GPU_CASES, 4)):
        for f in range(fields):
            for v in {c[f] for c in cases}:
                seen = {_rotation(_rot_index(c)) for c in cases if c[f] == v}
                assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {False, True}, (f, v)


@pytest.mark.parametrize("case", _HOST_CASES, ids=_id)
def test_panel_rhs_t_host(case):
    shape, k, dt = case
    masked, aligned = _rotation(_rot_index(case))
    _run_case("cpu", shape, k, dt, masked, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _GPU_CASES, ids=_id)
def test_panel_rhs_t_gpu(case):
    shape, k, dt, split = case
    masked, aligned = _rotation(_rot_index(case))
    _run_case("cuda", shape, k, dt, masked, aligned, split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_panel_rhs_t_gpu_bit_identical(dt, split):
    for shape, k, aligned in (((1003, 59, 3, 0), 17, False), ((2048, 128, 1, 0), 64, True)):
        _run_case("cuda", shape, k, dt, True, aligned, split=split, twice=True)


def _bad_k(device):
    n, m = 64, 16
    P = torch.zeros((n, n), dtype=torch.float64, device=device)
    V = torch.zeros((n, 80), dtype=torch.float64, device=device)
    S = torch.zeros((n, 80), dtype=torch.float64, device=device)
    for k in (0, 65):
        with pytest.raises(RuntimeError):
            ops.panel_rhs_t(P, V, S, n, m, ncols=k)
        with pytest.raises(RuntimeError):
            ops.axpy_cols_masked(S, V, ncols=k)
    assert float(S.abs().max()) == 0.0
    ops.panel_rhs_t(P, V, S, n, m, ncols=64)
    ops.axpy_cols_masked(S, V, ncols=64)


def test_bad_k_host():
    _bad_k("cpu")


@pytest.mark.gpu
def test_bad_k_gpu():
    _bad_k("cuda")


# ------------------------------------------------------------------ axpy_cols_masked
def _axpy_case(device, rows, k, sign, cin_mode, masked, s_nan=None):
    rng = np.random.default_rng([31, rows, k])
    S = rng.uniform(-1, 1, (rows, k)) * np.ldexp(1.0, (np.arange(k) * 5) % 17 - 8)[None, :]
    if s_nan is not None:
        S[s_nan] = np.nan
    cin = rng.uniform(-1, 1, (rows, k))
    Spar, Sv = _embed(torch.from_numpy(S), 2, 3, k + 7, float("nan"), device)
    if cin_mode == "alias":
        Ypar, Yv = _embed(torch.from_numpy(cin), 8, 5, k + 13, SENT, device)
        Cv, Cpar = Yv, None
    else:
        Ypar, Yv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
        Cpar, Cv = (None, None) if cin_mode == "null" else _embed(torch.from_numpy(cin), 1, 2, k + 3,
                                                                   float("nan"), device)
    on = np.ones(k, dtype=bool)
    if masked:
        on[::3] = False
    active = torch.from_numpy(on.astype(np.int32)).to(device) if masked else None
    cmpar = torch.full((k + 16,), SENT, dtype=torch.float64, device=device)
    cm = cmpar[8:8 + k]
    before = {nm: _bits(t) for nm, t in (("S", Spar), ("Y", Ypar), ("C", Cpar), ("cm", cmpar)) if t is not None}
    ops.axpy_cols_masked(Yv, Sv, C_in=Cv, sign=sign, active=active, colmax=cm, ncols=k)
    got, got_cm = Yv.cpu().numpy().copy(), cm.cpu().numpy().copy()
    for nm, par in (("S", Spar), ("C", Cpar)):
        if par is not None:
            assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    assert _outside_equal(Ypar, before["Y"], 8, rows, 5, k), "write outside Y"
    assert _outside_equal(cmpar.reshape(1, -1), before["cm"].reshape(1, -1), 0, 1, 8, k), "write outside colmax"
    cin0 = np.zeros((rows, k)) if cin_mode == "null" else cin
    y_untouched = cin if cin_mode == "alias" else np.full((rows, k), SENT)
    off = ~on
    # inactive columns: Y and colmax bitwise untouched
    assert np.array_equal(got[:, off].view(np.int64), y_untouched[:, off].view(np.int64))
    assert np.array_equal(got_cm[off], np.full(off.sum(), SENT))
    ref = cin0.astype(LD) + LD(sign) * S.astype(LD)
    finite = np.isfinite(S)
    err = np.abs(got.astype(LD) - ref)
    bound = _U["fp64"] * (np.abs(cin0).astype(LD) + np.abs(S).astype(LD))
    assert ((err <= bound) | ~finite)[:, on].all()
    assert np.isnan(got[:, on][~finite[:, on]]).all()
    for j in np.nonzero(on)[0]:
        col = np.abs(got[:, j])
        want = np.nan if np.isnan(col).any() else col.max()
        assert (np.isnan(want) and np.isnan(got_cm[j])) or got_cm[j] == want, (j, got_cm[j], want)
    return got, got_cm


_AXPY_CASES = [(rows, k, sign, cm, masked) for rows in (300, 1003, 2048) for k in KS for sign in (1.0, -1.0)
               for cm in CIN_MODES for masked in (False, True)]


def _axpy_id(c):
    return f"rows{c[0]}-k{c[1]}-{'plus' if c[2] > 0 else 'minus'}-{c[3]}-{'masked' if c[4] else 'all'}"


@pytest.mark.parametrize("case", _AXPY_CASES, ids=_axpy_id)
def test_axpy_cols_masked_host(case):
    _axpy_case("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _AXPY_CASES, ids=_axpy_id)
def test_axpy_cols_masked_gpu(case):
    _axpy_case("cuda", *case)


def _nan_case(device):
    # a NaN in a row of V this rank owns fills column 3 of S and reaches colmax[3] alone; the NaN in
    # the rows of V that other ranks own, in the rows >= n and in P's padding never shows (_run_case)
    shape = (1000, 59, 3, 1)  # the rank that owns the ragged last block
    n = shape[0]
    L = _layout(*shape)
    g = int(L["grow"][L["real"]][-1])  # its last real row
    for dt in ("fp64", "fp32"):
        S = _run_case(device, shape, 5, dt, False, dt == "fp64", v_nan=(g, 3))
        assert np.isnan(S[:, 3]).all() and np.isfinite(np.delete(S, 3, axis=1)).all()
        Sd = torch.from_numpy(S).to(device)
        Y = torch.zeros((n, 5), dtype=torch.float64, device=device)
        cm = torch.full((5,), SENT, dtype=torch.float64, device=device)
        ops.axpy_cols_masked(Y, Sd, colmax=cm)
        cmax = cm.cpu().numpy()
        assert np.isnan(cmax[3]) and np.isfinite(np.delete(cmax, 3)).all()
    # a single NaN element of S reaches its column's maximum
    _, cmax = _axpy_case(device, 1003, 17, -1.0, "separate", True, s_nan=(1002, 4))
    assert np.isnan(cmax[4]) and np.isfinite(np.delete(cmax, [0, 3, 4, 6, 9, 12, 15])).all()


def test_colmax_nan_host():
    _nan_case("cpu")


@pytest.mark.gpu
def test_colmax_nan_gpu():
    _nan_case("cuda")


# ------------------------------------------------------------------ col_abs_sum
def _col_abs_sum_case(device, shape, dt, aligned, x_nan=None):
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    R = int(L["real"].sum())
    P = _operands(shape, dt)[0]
    Ppar, Pv = _place_P(shape, dt, aligned, device)
    if x_nan is not None:
        Pv[x_nan[0], x_nan[1]] = float("nan")
    opar = torch.full((L["npad"] + 16,), SENT, dtype=torch.float64, device=device)
    out = opar[8:8 + L["npad"]]
    pb, ob = _bits(Ppar), _bits(opar)
    ops.col_abs_sum(Pv, out, n, m, p, rank)
    assert torch.equal(_bits(Ppar), pb), "X was written"
    assert _outside_equal(opar.reshape(1, -1), ob.reshape(1, -1), 0, 1, 8, n), "write outside out[:n]"
    got = out[:n].cpu().numpy()
    ref = np.abs(P[L["real"]]).astype(LD).sum(axis=0)
    ok = np.abs(got.astype(LD) - ref) <= gamma(LD(R + 1), _U["fp64"]) * ref
    if x_nan is not None:
        assert np.isnan(got[x_nan[1]])
        ok[x_nan[1]] = True
    assert ok.all() and np.isfinite(np.delete(got, [] if x_nan is None else x_nan[1])).all()


_SUM_CASES = [(s, dt, (SHAPES.index(s) + i) % 2 == 0) for s in SHAPES for i, dt in enumerate(("fp64", "fp32"))]


@pytest.mark.parametrize("shape,dt,aligned", _SUM_CASES + [(SHAPES[0], "fp64", False), (SHAPES[0], "fp32", True)])
def test_col_abs_sum_host(shape, dt, aligned):
    _col_abs_sum_case("cpu", shape, dt, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dt,aligned", _SUM_CASES + [(SHAPES[0], "fp64", False), (SHAPES[0], "fp32", True)])
def test_col_abs_sum_gpu(shape, dt, aligned):
    _col_abs_sum_case("cuda", shape, dt, aligned)


def _sum_nan(device):
    shape = (1000, 59, 3, 1)
    r = int(np.nonzero(_layout(*shape)["real"])[0][-1])
    for dt in ("fp64", "fp32"):
        _col_abs_sum_case(device, shape, dt, dt == "fp32", x_nan=(r, 998))


def test_col_abs_sum_nan_host():
    _sum_nan("cpu")


@pytest.mark.gpu
def test_col_abs_sum_nan_gpu():
    _sum_nan("cuda")
