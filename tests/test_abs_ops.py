"""Device::panel_abs_rhs, panel_abs_rhs_t and bound_terms (csrc/include/gj/device.hpp) against their
contract, on both host executors and on the GPU (csrc/kernels/panel_abs.hip).

    panel_abs_rhs    Y[r][j] = |C_in[r][j]| + sum_{c<n} |P[r][c]| |V[c][j]|  (real local rows; the padded
                     local rows get |C_in| or 0), colmax[j] = max |Y| over the real rows
    panel_abs_rhs_t  S[c][j] = sum over the real local rows r of |P[r][c]| |V[grow(r)][j]|, c < n
    bound_terms      G = |R| + nz_eps D (+ safe1 where D <= safe2), berr[j] = max_r |R| / D

Embedding (the method of test_rhs_trans_ops.py).  Every operand is an interior view of a NaN-filled
parent with a leading dimension wider than the view; what the contract says is never read holds NaN
as well: the padding columns of P (c >= n), P's local padding rows (global row >= n), the rows >= n
of V, for the transposed op the rows of V that other ranks own, and every pitch gap.  Outputs sit
inside a sentinel-filled parent; after the call every byte outside the writable set is compared with
a copy taken before.  The operands have mixed signs and graded columns.  The views of P are placed
16-byte aligned or not ("vec" / "scalar"), the two load paths of the GPU kernels.

Reference and bounds.  The reference is the longdouble product of the absolute values of the
operands as stored (an fp32 P is what it is; V is never rounded: the op works in fp64 for both
dtypes).  With u = 2^-53 for BOTH dtypes and gamma(q) = q u / (1 - q u):
    panel_abs_rhs    |got - ref| <= gamma(n + 2) ref
    panel_abs_rhs_t  |got - ref| <= gamma(R + 2) ref      (R = the rank's real rows)
    bound_terms      |G - ref| <= 2 u ref, |berr - ref| <= 2 u ref
Derived, not measured: every term is non-negative, an element is n (R) multiply-adds in some order
(a chain per slice on the matrix cores, then the slices summed: never more than n roundings on any
term), one more for |C_in| +, one for the longdouble reference's own error.  G is one fused
multiply-add and at most one more addition; a ratio is at most one rounded sum and one division.

Cases.  (n, m, p, rank) = (300, 16, 1, 0), (1003, 59, 3, each rank), (1000, 59, 3, 1) (the ragged
last block on an odd npad); k in {1, 16, 17, 64}; both dtypes; on the GPU the split forced to 1, 2, 7
and automatic.  The alignment and the C_in mode (null / aliasing Y / separate) rotate over the cases
so that every value of each meets every k, shape, dtype and split (test_rotation_covers checks
exactly that).  Every GPU case asserts native.last_abs_kernel().
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
U = LD(2) ** -53
SHAPES = [(300, 16, 1, 0), (1003, 59, 3, 0), (1003, 59, 3, 1), (1003, 59, 3, 2), (1000, 59, 3, 1)]
KS = [1, 16, 17, 64]
SPLITS = [1, 2, 7, 0]
CIN_MODES = ["null", "alias", "separate"]
EXECUTORS = ["host", "async"]
_TD = {"fp64": torch.float64, "fp32": torch.float32}


def gamma(q):
    return q * U / (1 - q * U)


@functools.lru_cache(maxsize=None)
def _executor(name):
    """None: the executor of the tensors' device (host executor / HIP); "async": the asynchronous host executor"""
    return gj.load_native().async_host_device(2) if name == "async" else None


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """P (rows x n), V (n x 64), C (rows x 64) and, in longdouble, |P_real| |V| and |P_real|^T |V_owned|
    (computed once per shape and dtype with all 64 columns; a case with k columns uses the first k)."""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rng = np.random.default_rng([37, n, m, p, rank])
    P = rng.uniform(-1, 1, (L["rows"], n))
    # graded columns: an absolute tolerance would hide whole columns
    P *= np.ldexp(1.0, (np.arange(n) * 7) % 21 - 10)[None, :]
    V = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 17 - 8)[None, :]
    C = rng.uniform(-1, 1, (L["rows"], 64)) * np.ldexp(1.0, (np.arange(64) * 3) % 11 - 5)[None, :]
    if dt == "fp32":
        P = P.astype(np.float32).astype(np.float64)
    real, grow = L["real"], L["grow"]
    aP, aV = np.abs(P).astype(LD), np.abs(V).astype(LD)
    plain = aP[real] @ aV
    trans = aP[real].T @ aV[grow[real]]
    for x in (P, V, C, plain, trans):
        x.setflags(write=False)
    return P, V, C, plain, trans


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


def _place_P(shape, dt, aligned, device, zero_col=None, zero_row=None):
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad = L["rows"], L["npad"]
    es = 8 if dt == "fp64" else 4
    # the panel is rows x npad; columns >= n and local padding rows are NaN
    Pfull = np.full((rows, npad), np.nan)
    Pfull[:, :n] = _operands(shape, dt)[0]
    if zero_col is not None:
        Pfull[:, zero_col] = 0.0
    if zero_row is not None:
        Pfull[zero_row, :n] = 0.0
    Pfull[~L["real"], :] = np.nan
    if aligned:
        c0, ldp = 16 // es * 2, -(-(npad + 24) // 4) * 4
    else:
        c0, ldp = 5, (npad + 11) | 1
    Ppar, Pv = _embed(torch.from_numpy(Pfull).to(_TD[dt]), 3, c0, ldp, float("nan"), device)
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * es) % 16 == 0) == aligned
    return Ppar, Pv


def _expected_name(trans, dt, k, P, split, n, real):
    kw = 16 if k <= 16 else 32 if k <= 32 else 64
    vec = P.data_ptr() % 16 == 0 and (P.stride(0) * P.element_size()) % 16 == 0
    head = f"{'abst' if trans else 'abs'}{kw}:{'f64' if dt == 'fp64' else 'f32'}:{'vec' if vec else 'scalar'}:s"
    if split == 0:
        return head
    if trans:  # a forced split runs whole steps of 4 rows and no empty slice
        chunk = max(-(-(-(-real // split)) // 4) * 4, 4)
        return head + str(max(-(-real // chunk), 1))
    chunk = -(-(-(-n // split)) // 16) * 16  # slices of whole 16 columns, no empty slice
    return head + str(max(-(-n // chunk), 1))


def _check_name(native, device, trans, dt, k, Pv, split, n, R):
    name = native.last_abs_kernel()
    if device == "cpu":
        assert name == "host"
        return
    exp = _expected_name(trans, dt, k, Pv, split, n, R)
    assert name == exp if split else (name.startswith(exp) and name[len(exp):].isdigit()), (name, exp)


def _run_plain(device, shape, k, dt, aligned, cin_mode, split=0, twice=False, executor=None, v_scale=0,
               v_nan=None, zero_col=None):
    """Y = |C_in| + |P| |V| on one case; returns (Y over the local rows, colmax)"""
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad, real = L["rows"], L["npad"], L["real"]
    _, V, C, plain, _ = _operands(shape, dt)
    Ppar, Pv = _place_P(shape, dt, aligned, device, zero_col=zero_col)
    Vfull = np.full((npad, k), np.nan)
    Vfull[:n] = np.ldexp(V[:, :k], v_scale)
    if v_nan is not None:
        Vfull[v_nan] = np.nan
    Vpar, Vv = _embed(torch.from_numpy(Vfull), 2, 3, k + 7, float("nan"), device)
    cin = np.ldexp(C[:, :k], v_scale)
    if cin_mode == "alias":
        Ypar, Yv = _embed(torch.from_numpy(cin.copy()), 8, 5, k + 13, SENT, device)
        Cv, Cpar = Yv, None
    else:
        Ypar, Yv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
        Cpar, Cv = (None, None) if cin_mode == "null" else _embed(torch.from_numpy(cin.copy()), 1, 2, k + 3,
                                                                   float("nan"), device)
    cmpar = torch.full((k + 16,), SENT, dtype=torch.float64, device=device)
    cm = cmpar[8:8 + k]
    before = {nm: _bits(t) for nm, t in (("P", Ppar), ("V", Vpar), ("Y", Ypar), ("C", Cpar), ("cm", cmpar))
              if t is not None}

    def launch():
        if device != "cpu":
            native.set_rhs_splitk(split)
        try:
            ops.panel_abs_rhs(Pv, Vv, Yv, n, m, p, rank, C_in=Cv, colmax=cm, ncols=k, device=_executor(executor))
        finally:
            if device != "cpu":
                native.set_rhs_splitk(0)

    launch()
    _check_name(native, device, False, dt, k, Pv, split, n, int(real.sum()))
    got, got_cm = Yv.cpu().numpy().copy(), cm.cpu().numpy().copy()
    if twice and cin_mode != "alias":
        y1, c1 = _bits(Ypar), _bits(cmpar)
        launch()
        assert torch.equal(_bits(Ypar), y1) and torch.equal(_bits(cmpar), c1), "two runs differ"

    for nm, par in (("P", Ppar), ("V", Vpar), ("C", Cpar)):
        if par is not None:
            assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    assert _outside_equal(Ypar, before["Y"], 8, rows, 5, k), "write outside Y"
    assert _outside_equal(cmpar.reshape(1, -1), before["cm"].reshape(1, -1), 0, 1, 8, k), "write outside colmax"
    acin = np.zeros((rows, k)) if cin_mode == "null" else np.abs(cin)
    # the padded local rows: |C_in| (or 0), exactly
    assert np.array_equal(got[~real].view(np.int64), acin[~real].view(np.int64))
    for j in range(k):
        col = got[real, j]
        want = np.nan if np.isnan(col).any() else (col.max() if col.size else 0.0)
        assert (np.isnan(want) and np.isnan(got_cm[j])) or got_cm[j] == want, (j, got_cm[j], want)
    if v_nan is not None:
        return got, got_cm
    ref = acin[real].astype(LD) + np.ldexp(plain[:, :k], v_scale)
    err = np.abs(got[real].astype(LD) - ref)
    assert (err <= gamma(LD(n + 2)) * ref).all(), (float((err / np.maximum(ref, LD(10) ** -4000) / U).max()), n + 2)
    assert np.isfinite(got).all()
    return got, got_cm


def _run_trans(device, shape, k, dt, aligned, split=0, twice=False, executor=None, v_scale=0, v_nan=None,
               zero_row=None):
    """S = |P|^T |V_loc| on one case; returns S[:n]"""
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    npad = L["npad"]
    R = int(L["real"].sum())
    _, V, _, _, trans = _operands(shape, dt)
    Ppar, Pv = _place_P(shape, dt, aligned, device, zero_row=zero_row)
    # V: the rows this rank owns; the rows of other ranks and the rows >= n are NaN
    Vfull = np.full((npad, k), np.nan)
    own = L["grow"][L["real"]]
    Vfull[own] = np.ldexp(V[own, :k], v_scale)
    if v_nan is not None:
        Vfull[v_nan] = np.nan
    Vpar, Vv = _embed(torch.from_numpy(Vfull), 2, 3, k + 7, float("nan"), device)
    # S: npad rows in view, of which the first n are writable
    Spar, Sv = _embed(torch.full((npad, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
    before = {nm: _bits(t) for nm, t in (("P", Ppar), ("V", Vpar), ("S", Spar))}

    def launch():
        if device != "cpu":
            native.set_rhs_t_split(split)
        try:
            ops.panel_abs_rhs_t(Pv, Vv, Sv, n, m, p, rank, ncols=k, device=_executor(executor))
        finally:
            if device != "cpu":
                native.set_rhs_t_split(0)

    launch()
    _check_name(native, device, True, dt, k, Pv, split, n, R)
    got = Sv.cpu().numpy().copy()
    if twice:
        s1 = _bits(Spar)
        launch()
        assert torch.equal(_bits(Spar), s1), "two runs differ"
    for nm, par in (("P", Ppar), ("V", Vpar)):
        assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    assert _outside_equal(Spar, before["S"], 8, n, 5, k), "write outside S"
    if v_nan is not None:
        return got[:n]
    ref = np.ldexp(trans[:, :k], v_scale)
    err = np.abs(got[:n].astype(LD) - ref)
    assert (err <= gamma(LD(R + 2)) * ref).all(), (float((err / np.maximum(ref, LD(10) ** -4000) / U).max()), R + 2)
    assert np.isfinite(got[:n]).all()
    return got[:n]


_ROT = list(itertools.product([True, False], CIN_MODES))


def _rotation(i):
    """aligned, C_in mode for rotation index i: the 6 combinations in turn"""
    return _ROT[i % 6]


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
    """every alignment and every C_in mode meets every k, shape, dtype and split"""
    for cases, fields in ((_HOST_CASES, 3), (_GPU_CASES, 4)):
        for f in range(fields):
            for v in {c[f] for c in cases}:
                seen = {_rotation(_rot_index(c)) for c in cases if c[f] == v}
                assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == set(CIN_MODES), (f, v)


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("case", _HOST_CASES, ids=_id)
def test_panel_abs_rhs_host(case, executor):
    shape, k, dt = case
    aligned, cin = _rotation(_rot_index(case))
    _run_plain("cpu", shape, k, dt, aligned, cin, executor=executor)


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("case", _HOST_CASES, ids=_id)
def test_panel_abs_rhs_t_host(case, executor):
    shape, k, dt = case
    aligned, _ = _rotation(_rot_index(case))
    _run_trans("cpu", shape, k, dt, aligned, executor=executor)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _GPU_CASES, ids=_id)
def test_panel_abs_rhs_gpu(case):
    shape, k, dt, split = case
    aligned, cin = _rotation(_rot_index(case))
    _run_plain("cuda", shape, k, dt, aligned, cin, split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _GPU_CASES, ids=_id)
def test_panel_abs_rhs_t_gpu(case):
    shape, k, dt, split = case
    aligned, _ = _rotation(_rot_index(case))
    _run_trans("cuda", shape, k, dt, aligned, split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_gpu_bit_identical(dt, split):
    for shape, k, aligned in (((1003, 59, 3, 0), 17, False), ((1000, 59, 3, 1), 64, True)):
        _run_plain("cuda", shape, k, dt, aligned, "separate", split=split, twice=True)
        _run_trans("cuda", shape, k, dt, aligned, split=split, twice=True)


# ------------------------------------------------------------------ fp64 arithmetic on fp32 storage
def _tiny_v(device, executor=None):
    """V = 2^-160 (...) is below fp32's smallest subnormal: any fp32 rounding of V or fp32
    accumulation gives 0; the fp64 product is non-zero and as accurate as ever."""
    for shape, k, aligned in (((300, 16, 1, 0), 5, True), ((1000, 59, 3, 1), 17, False)):
        Y, cm = _run_plain(device, shape, k, "fp32", aligned, "separate", executor=executor, v_scale=-160)
        real = _layout(*shape)["real"]
        assert (Y[real] > 0).all() and (cm > 0).all()
        S = _run_trans(device, shape, k, "fp32", aligned, executor=executor, v_scale=-160)
        assert (S > 0).all()


@pytest.mark.parametrize("executor", EXECUTORS)
def test_fp32_storage_fp64_arithmetic_host(executor):
    _tiny_v("cpu", executor)


@pytest.mark.gpu
def test_fp32_storage_fp64_arithmetic_gpu():
    _tiny_v("cuda")


# ------------------------------------------------------------------ NaN through a zero factor
def _nan_through_zero(device, executor=None):
    shape = (1000, 59, 3, 1)  # the rank that owns the ragged last block
    L = _layout(*shape)
    real = L["real"]
    for dt in ("fp64", "fp32"):
        # column 7 of P is all zeros, V[7][3] is NaN: 0 * NaN is a term of every Y[r][3]
        Y, cm = _run_plain(device, shape, 5, dt, dt == "fp64", "null", executor=executor, v_nan=(7, 3), zero_col=7)
        assert np.isnan(Y[real, 3]).all() and np.isfinite(np.delete(Y, 3, axis=1)).all()
        assert np.isnan(cm[3]) and np.isfinite(np.delete(cm, 3)).all()
        # the rank's last real row of P is all zeros, V at its global row is NaN in column 3
        r = int(np.nonzero(real)[0][-1])
        S = _run_trans(device, shape, 5, dt, dt == "fp32", executor=executor, v_nan=(int(L["grow"][r]), 3), zero_row=r)
        assert np.isnan(S[:, 3]).all() and np.isfinite(np.delete(S, 3, axis=1)).all()


@pytest.mark.parametrize("executor", EXECUTORS)
def test_nan_through_zero_host(executor):
    _nan_through_zero("cpu", executor)


@pytest.mark.gpu
def test_nan_through_zero_gpu():
    _nan_through_zero("cuda")


# ------------------------------------------------------------------ arguments
def _bad_k(device, executor=None):
    n, m = 64, 16
    ex = _executor(executor)
    P = torch.zeros((n, n), dtype=torch.float64, device=device)
    V = torch.zeros((n, 80), dtype=torch.float64, device=device)
    S = torch.zeros((n, 80), dtype=torch.float64, device=device)
    be = torch.zeros(80, dtype=torch.float64, device=device)
    for k in (0, 65):
        with pytest.raises(RuntimeError):
            ops.panel_abs_rhs(P, V, S, n, m, ncols=k, device=ex)
        with pytest.raises(RuntimeError):
            ops.panel_abs_rhs_t(P, V, S, n, m, ncols=k, device=ex)
        with pytest.raises(RuntimeError):
            ops.bound_terms(V, V, S, be, 1e-16, 1e-300, 1e-290, ncols=k, device=ex)
    assert float(S.abs().max()) == 0.0
    ops.panel_abs_rhs(P, V, S, n, m, ncols=64, device=ex)
    ops.panel_abs_rhs_t(P, V, S, n, m, ncols=64, device=ex)


@pytest.mark.parametrize("executor", EXECUTORS)
def test_bad_k_host(executor):
    _bad_k("cpu", executor)


@pytest.mark.gpu
def test_bad_k_gpu():
    _bad_k("cuda")


@pytest.mark.gpu
def test_leading_dimension_gpu():
    """a leading dimension whose tile rows leave 32-bit byte offsets is refused before anything runs (the
    view is never dereferenced: n = 0 columns would be read, but the check comes first)"""
    x = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    big = torch.as_strided(x, (1, 4), (1 << 29, 1))
    Y = torch.zeros((16, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.panel_abs_rhs(big, Y, Y, 4, 16, ncols=4)
    with pytest.raises(RuntimeError):
        ops.panel_abs_rhs_t(big, Y, Y, 4, 16, ncols=4)
    assert float(Y.abs().max()) == 0.0


# ------------------------------------------------------------------ bound_terms
def _bound_case(device, rows, k, alias, executor=None):
    n = 1003
    nz, safe1 = (n + 1) * 2.0 ** -53, (n + 1) * np.finfo(np.float64).tiny
    safe2 = safe1 / 2.0 ** -53
    rng = np.random.default_rng([41, rows, k])
    R = rng.uniform(-1, 1, (rows, k)) * np.ldexp(1.0, (np.arange(k) * 5) % 17 - 30)[None, :]
    D = rng.uniform(0.5, 1, (rows, k)) * np.ldexp(1.0, (np.arange(k) * 3) % 13 - 6)[None, :]
    if rows:
        # safe2 rows: D = 0 with R = 0 (ratio 1), D = 0 with R != 0 (a huge ratio), D tiny and R tiny
        D[rows // 2, :] = 0.0
        R[rows // 2, ::2] = 0.0
        if rows > 3:
            D[3, :] = safe2 / 4
            R[3, :] = rng.uniform(-1, 1, k) * safe2
    Rpar, Rv = _embed(torch.from_numpy(R.copy()), 2, 3, k + 7, SENT if alias else float("nan"), device)
    Dpar, Dv = _embed(torch.from_numpy(D), 1, 2, k + 3, float("nan"), device)
    if alias:
        Gpar, Gv = Rpar, Rv
    else:
        Gpar, Gv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
    bepar = torch.full((k + 16,), SENT, dtype=torch.float64, device=device)
    be = bepar[8:8 + k]
    before = {nm: _bits(t) for nm, t in (("R", Rpar), ("D", Dpar), ("G", Gpar), ("be", bepar))}
    ops.bound_terms(Rv, Dv, Gv, be, nz, safe1, safe2, rows=rows, ncols=k, device=_executor(executor))
    G, berr = Gv.cpu().numpy().copy(), be.cpu().numpy().copy()
    assert torch.equal(_bits(Dpar), before["D"]), "D was written"
    if not alias:
        assert torch.equal(_bits(Rpar), before["R"]), "R was written"
    assert _outside_equal(Gpar, before["G"], 2 if alias else 8, rows, 3 if alias else 5, k), "write outside G"
    assert _outside_equal(bepar.reshape(1, -1), before["be"].reshape(1, -1), 0, 1, 8, k), "write outside berr"
    if rows == 0:
        assert (berr.view(np.int64) == 0).all()  # +0.0
        return
    aR, Dl, tiny = np.abs(R).astype(LD), D.astype(LD), D <= safe2
    assert tiny.any()
    gref = aR + LD(nz) * Dl + np.where(tiny, LD(safe1), LD(0))
    assert (np.abs(G.astype(LD) - gref) <= 2 * U * gref).all()
    ratio = np.where(tiny, (aR + LD(safe1)) / (Dl + LD(safe1)), aR / np.where(tiny, LD(1), Dl))
    bref = ratio.max(axis=0)
    assert (np.abs(berr.astype(LD) - bref) <= 2 * U * bref).all(), (berr, bref)
    if rows <= 3:  # the D = 0, R = 0 row is the largest ratio of its column: exactly 1
        assert (berr[::2] == 1.0).all()


_BOUND_CASES = [(rows, k, (i + j) % 2 == 0) for i, rows in enumerate((0, 1, 3, 300, 1003)) for j, k in enumerate(KS)]


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("rows,k,alias", _BOUND_CASES)
def test_bound_terms_host(rows, k, alias, executor):
    _bound_case("cpu", rows, k, alias, executor)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k,alias", _BOUND_CASES)
def test_bound_terms_gpu(rows, k, alias):
    _bound_case("cuda", rows, k, alias)


def _bound_nan(device, executor=None):
    rows, k = 70, 5
    R = torch.full((rows, k), 1e-17, dtype=torch.float64)
    D = torch.ones((rows, k), dtype=torch.float64)
    R[69, 3] = float("nan")
    D[0, 1] = float("nan")
    R, D = R.to(device), D.to(device)
    G = torch.zeros((rows, k), dtype=torch.float64, device=device)
    be = torch.zeros(k, dtype=torch.float64, device=device)
    ops.bound_terms(R, D, G, be, 1e-13, 1e-305, 1e-289, device=_executor(executor))
    b, g = be.cpu().numpy(), G.cpu().numpy()
    assert np.isnan(b[[1, 3]]).all() and (b[[0, 2, 4]] == 1e-17).all()
    assert np.isnan(g[69, 3]) and np.isnan(g[0, 1]) and np.isnan(g).sum() == 2


@pytest.mark.parametrize("executor", EXECUTORS)
def test_bound_terms_nan_host(executor):
    _bound_nan("cpu", executor)


@pytest.mark.gpu
def test_bound_terms_nan_gpu():
    _bound_nan("cuda")
