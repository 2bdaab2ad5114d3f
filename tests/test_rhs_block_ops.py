"""Device::panel_rhs, gather_rows_natural and copy_cols_masked (csrc/include/gj/device.hpp) against
their contract, on the host executor and on the GPU (csrc/kernels/panel_rhs.hip).

panel_rhs: Y = C_in + sign * P V over the columns c < n, for this rank's rows of a panel.

Embedding.  Every operand is an interior view of a NaN-filled parent with a leading dimension wider
than the view; what the contract says is never read holds NaN as well: the padding columns of P
(c >= n), P's local padding rows (global row >= n), the rows >= n of V and every pitch gap.  Y, colmax
and the destination of gather_rows_natural sit inside a sentinel-filled parent.  A finite result
proves nothing of that was read; after the call every byte outside the writable set is compared
with a copy taken before.  The views are placed 16-byte aligned or not ("vec" / "scalar"), the
two load paths of the GPU kernel; an odd npad with ld = npad is the unaligned case of the engine.

Reference and bound.  The reference is the longdouble product over c < n from the operands as
stored (fp32: V rounded to fp32 first, as the op does on load).  Componentwise
    |got - ref| <= gamma(n + 2) (|C_in| + |P| |V|),   gamma(q) = q u / (1 - q u),
u = 2^-53 (fp64) or 2^-24 (fp32).  Derived, not measured: the product of an element is n multiply-adds
in some order (a chain per K-slice on the matrix cores, one rounding per term, then the slices
summed in fp64: never more than n roundings on any term), which gives gamma(n) |P| |V|; adding it
to C_in is one more rounding of the sum, and the last u covers the longdouble reference's own
error (n 2^-64 S).  The fp32 path widens the product and adds in fp64, far inside the fp32 u.

Cases.  (n, m, p, rank) = (300, 16, 1, 0), (1003, 59, 3, each rank: an odd npad, a rank with
fewer blocks), (2048, 128, 1, 0), and (1000, 59, 3, 1): 1003 = 17 * 59 has no short block, so the
ragged last block on an odd npad at p > 1 is this one's; k in {1, 5, 16, 17, 40, 64}; both dtypes; on
the GPU the K-split forced to 1, 2, 7 and auto.  sign, the C_in mode (null / aliasing Y /
separate), the active mask (null / some columns off) and the alignment rotate over the cases so
that every value of each meets every k, shape and split.  Every GPU case asserts
native.last_rhs_kernel().
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
SHAPES = [(300, 16, 1, 0), (1003, 59, 3, 0), (1003, 59, 3, 1), (1003, 59, 3, 2), (2048, 128, 1, 0),
          (1000, 59, 3, 1)]
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
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n, max_nblk=(Nr + p - 1) // p)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """P (rows x n), V (n x 64), C_in (rows x 64) and, in longdouble, P V and |P| |V| (computed once
    per shape and dtype with all 64 columns; a case with k columns uses the first k)."""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rng = np.random.default_rng([23, n, m, p, rank])
    P = rng.uniform(-1, 1, (L["rows"], n))
    # graded rows and columns: an absolute tolerance would hide whole rows
    P *= np.ldexp(1.0, (np.arange(L["rows"]) * 7) % 21 - 10)[:, None]
    V = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 17 - 8)[None, :]
    Cin = rng.uniform(-1, 1, (L["rows"], 64))
    if dt == "fp32":
        P = P.astype(np.float32).astype(np.float64)
    Vop = V.astype(np.float32).astype(np.float64) if dt == "fp32" else V
    prod = P.astype(LD) @ Vop.astype(LD)
    absprod = np.abs(P).astype(LD) @ np.abs(Vop).astype(LD)
    for x in (P, V, Cin, prod, absprod):
        x.setflags(write=False)
    return P, V, Cin, prod, absprod


def _embed(t, r0, c0, ld, fill, device, extra_rows=9):
    """t as an interior view of a `fill`-filled parent with leading dimension ld"""
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), fill, dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to(device)
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _expected_name(dt, k, P, split, n):
    kw = 16 if k <= 16 else 32 if k <= 32 else 64
    vec = P.data_ptr() % 16 == 0 and (P.stride(0) * P.element_size()) % 16 == 0
    head = f"rhs{kw}:{'f64' if dt == 'fp64' else 'f32'}:{'vec' if vec else 'scalar'}:s"
    return head if split == 0 else head + str(split)


def _run_case(device, shape, k, dt, sign, cin_mode, masked, aligned, split=0, cin_nan=None, twice=False):
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad = L["rows"], L["npad"]
    P, V, Cin, prod, absprod = _operands(shape, dt)
    es = 8 if dt == "fp64" else 4
    # P: the panel is rows x npad; columns >= n and local padding rows are NaN
    Pfull = np.full((rows, npad), np.nan)
    Pfull[:, :n] = P
    Pfull[~L["real"], :] = np.nan
    if aligned:
        c0, ldp = 16 // es * 2, -(-(npad + 24) // 4) * 4
    else:
        c0, ldp = 5, (npad + 11) | 1
    Ppar, Pv = _embed(torch.from_numpy(Pfull).to(_TD[dt]), 3, c0, ldp, float("nan"), device)
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * es) % 16 == 0) == aligned or rows == 0
    # V: n real rows, then NaN rows up to npad and beyond
    Vpar, Vv = _embed(torch.from_numpy(V[:, :k].copy()), 2, 3, k + 7, float("nan"), device,
                      extra_rows=npad - n + 9)
    cin = Cin[:, :k].copy()
    if cin_nan is not None:
        cin[cin_nan] = np.nan
    if cin_mode == "alias":
        Ypar, Yv = _embed(torch.from_numpy(cin), 8, 5, k + 13, SENT, device)
        Cv, Cpar = Yv, None
    else:
        Ypar, Yv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
        Cpar, Cv = (None, None) if cin_mode == "null" else _embed(torch.from_numpy(cin), 1, 2, k + 3,
                                                                   float("nan"), device)
    on = np.ones(k, dtype=bool)
    if masked:
        on[::3] = False  # column 0 off, also at k = 1
    active = torch.from_numpy(on.astype(np.int32)).to(device) if masked else None
    cmpar = torch.full((k + 16,), SENT, dtype=torch.float64, device=device)
    cm = cmpar[8:8 + k]
    before = {name: _bits(t) for name, t in (("P", Ppar), ("V", Vpar), ("Y", Ypar), ("C", Cpar), ("cm", cmpar))
              if t is not None}

    def launch():
        if device != "cpu":
            native.set_rhs_splitk(split)
        try:
            ops.panel_rhs(Pv, Vv, Yv, n, m, p, rank, C_in=Cv, sign=sign, active=active, colmax=cm, ncols=k)
        finally:
            if device != "cpu":
                native.set_rhs_splitk(0)

    launch()
    name = native.last_rhs_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        exp = _expected_name(dt, k, Pv, split, n)
        assert name == exp if split else (name.startswith(exp) and name[len(exp):].isdigit()), (name, exp)
    got = Yv.cpu().numpy().copy()
    got_cm = cm.cpu().numpy().copy()
    if twice and cin_mode != "alias":
        y1, c1 = _bits(Ypar), _bits(cmpar)
        launch()
        assert torch.equal(_bits(Ypar), y1) and torch.equal(_bits(cmpar), c1), "two runs differ"

    # inputs untouched, nothing outside the Y view and the colmax view written
    for nm, par in (("P", Ppar), ("V", Vpar), ("C", Cpar)):
        if par is not None:
            assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    yb = _bits(Ypar).clone()
    ybefore = before["Y"].clone()
    yb[8:8 + rows, 5:5 + k] = 0
    ybefore[8:8 + rows, 5:5 + k] = 0
    assert torch.equal(yb, ybefore), "write outside Y"
    cb, cbefore = _bits(cmpar).clone(), before["cm"].clone()
    cb[8:8 + k] = 0
    cbefore[8:8 + k] = 0
    assert torch.equal(cb, cbefore), "write outside colmax"

    cin0 = np.zeros((rows, k)) if cin_mode == "null" else cin
    y_untouched = cin if cin_mode == "alias" else np.full((rows, k), SENT)
    real = L["real"]
    # inactive columns: Y and colmax bitwise untouched
    off = ~on
    assert np.array_equal(got[:, off].view(np.int64), y_untouched[:, off].view(np.int64))
    assert np.array_equal(got_cm[off], np.full(off.sum(), SENT))
    # padded local rows: Y = C_in (or 0), exactly
    assert np.array_equal(got[~real][:, on].view(np.int64), cin0[~real][:, on].view(np.int64))
    # real rows: the bound
    ref = cin0[real].astype(LD) + LD(sign) * prod[real, :k]
    S = np.abs(cin0[real]).astype(LD) + absprod[real, :k]
    err = np.abs(got[real].astype(LD) - ref)
    bound = gamma(LD(n + 2), _U[dt]) * S
    finite = np.isfinite(ref.astype(np.float64))
    ok = (err <= bound) | ~finite
    assert ok[:, on].all(), (float((err / np.maximum(S, LD(1e-300)) / _U[dt])[:, on][finite[:, on]].max()), n + 2)
    assert np.isnan(got[real][~finite]).all()
    assert np.isfinite(got[real][:, on][finite[:, on]]).all()
    # colmax: the maximum over the real rows of what was written, NaN kept
    for j in np.nonzero(on)[0]:
        col = np.abs(got[real, j])
        want = np.nan if np.isnan(col).any() else (col.max() if col.size else 0.0)
        assert (np.isnan(want) and np.isnan(got_cm[j])) or got_cm[j] == want, (j, got_cm[j], want)
    return got, got_cm


def _rotation(i):
    """sign, C_in mode, masked, aligned for case number i: the 24 combinations in turn"""
    combos = list(itertools.product([1.0, -1.0], CIN_MODES, [False, True], [True, False]))
    return combos[i % len(combos)]


_HOST_CASES = [(s, k, dt) for s in SHAPES for k in KS for dt in ("fp64", "fp32")]
_GPU_CASES = [(s, k, dt, sp) for s in SHAPES for k in KS for dt in ("fp64", "fp32") for sp in SPLITS]


def _id(c):
    s = c[0]
    tail = "" if len(c) < 4 else f"-split{c[3]}"
    return f"n{s[0]}m{s[1]}p{s[2]}r{s[3]}-k{c[1]}-{c[2]}{tail}"


@pytest.mark.parametrize("case", _HOST_CASES, ids=_id)
def test_panel_rhs_host(case):
    shape, k, dt = case
    sign, cin_mode, masked, aligned = _rotation(7 * _HOST_CASES.index(case))
    _run_case("cpu", shape, k, dt, sign, cin_mode, masked, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _GPU_CASES, ids=_id)
def test_panel_rhs_gpu(case):
    shape, k, dt, split = case
    # 5 is coprime to 24: consecutive cases (the four splits of one shape / k / dtype) take different
    # combinations, and over the list every combination meets every split
    sign, cin_mode, masked, aligned = _rotation(5 * _GPU_CASES.index(case))
    _run_case("cuda", shape, k, dt, sign, cin_mode, masked, aligned, split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_panel_rhs_gpu_bit_identical(dt, split):
    for shape, k, aligned in (((1003, 59, 3, 0), 17, False), ((2048, 128, 1, 0), 64, True)):
        _run_case("cuda", shape, k, dt, -1.0, "separate", True, aligned, split=split, twice=True)


def _nan_case(device):
    # a NaN in a real row of Y (through C_in) gives colmax = NaN for that column alone; the NaN that
    # fills P's padding columns and rows, V's rows >= n and every pitch gap never shows (_run_case)
    shape = (1000, 59, 3, 1)  # the rank that owns the ragged last block
    L = _layout(*shape)
    r = int(np.nonzero(L["real"])[0][-1])
    for dt in ("fp64", "fp32"):
        _, cmax = _run_case(device, shape, 5, dt, 1.0, "separate", False, False, cin_nan=(r, 3))
        assert np.isnan(cmax[3]) and np.isfinite(np.delete(cmax, 3)).all()
        # a NaN of C_in in a padded local row reaches Y there (Y = C_in) but not the maximum
        pad = int(np.nonzero(~L["real"])[0][0])
        got, cmax = _run_case(device, shape, 5, dt, 1.0, "alias", False, True, cin_nan=(pad, 2))
        assert np.isnan(got[pad, 2]) and np.isfinite(cmax).all()


def test_colmax_nan_host():
    _nan_case("cpu")


@pytest.mark.gpu
def test_colmax_nan_gpu():
    _nan_case("cuda")


def _bad_k(device):
    n, m = 64, 16
    P = torch.zeros((n, n), dtype=torch.float64, device=device)
    V = torch.zeros((n, 80), dtype=torch.float64, device=device)
    Y = torch.zeros((n, 80), dtype=torch.float64, device=device)
    for k in (0, 65):
        with pytest.raises(RuntimeError):
            ops.panel_rhs(P, V, Y, n, m, ncols=k)
    assert float(Y.abs().max()) == 0.0
    ops.panel_rhs(P, V, Y, n, m, ncols=64)


def test_bad_k_host():
    _bad_k("cpu")


@pytest.mark.gpu
def test_bad_k_gpu():
    _bad_k("cuda")


# ------------------------------------------------------------------ reorder and copy
def _gather_case(device, n, m, p, k):
    L0 = _layout(n, m, p, 0)
    per = L0["max_nblk"] * m
    rng = np.random.default_rng([5, n, m, p, k])
    src = rng.standard_normal((p * per, k))
    want = np.full((L0["npad"] + 3, k), SENT)
    for q in range(p):
        Lq = _layout(n, m, p, q)
        g = Lq["grow"][Lq["real"]]
        want[g] = src[q * per + np.nonzero(Lq["real"])[0]]
    spar, sv = _embed(torch.from_numpy(src), 2, 3, k + 5, float("nan"), device)
    dpar, dv = _embed(torch.full((L0["npad"] + 3, k), SENT, dtype=torch.float64), 4, 6, k + 9, SENT, device)
    before = _bits(dpar).clone()
    ops.gather_rows_natural(dv, sv, n, m, p, ncols=k)
    assert np.array_equal(dv.cpu().numpy().view(np.int64), want.view(np.int64))  # rows >= n keep the sentinel
    after = _bits(dpar).clone()
    after[4:4 + dv.shape[0], 6:6 + k] = 0
    before[4:4 + dv.shape[0], 6:6 + k] = 0
    assert torch.equal(after, before)


def _copy_case(device, rows, k):
    rng = np.random.default_rng([9, rows, k])
    src = rng.standard_normal((rows, k))
    mask = (np.arange(k) % 3 != 1).astype(np.int32)
    spar, sv = _embed(torch.from_numpy(src), 2, 3, k + 5, float("nan"), device)
    dpar, dv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 4, 6, k + 9, SENT, device)
    before = _bits(dpar).clone()
    ops.copy_cols_masked(dv, sv, torch.from_numpy(mask).to(device))
    want = np.where(mask[None, :] != 0, src, SENT)
    assert np.array_equal(dv.cpu().numpy().view(np.int64), want.view(np.int64))
    after = _bits(dpar).clone()
    after[4:4 + rows, 6:6 + k] = 0
    before[4:4 + rows, 6:6 + k] = 0
    assert torch.equal(after, before)


_REORDER = [(300, 16, 1, 5), (1003, 59, 3, 17), (1003, 59, 3, 64), (2048, 128, 1, 1), (50, 16, 5, 3)]


@pytest.mark.parametrize("n,m,p,k", _REORDER)
def test_gather_rows_natural_host(n, m, p, k):
    _gather_case("cpu", n, m, p, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,p,k", _REORDER)
def test_gather_rows_natural_gpu(n, m, p, k):
    _gather_case("cuda", n, m, p, k)


@pytest.mark.parametrize("rows,k", [(1, 1), (354, 17), (2048, 64)])
def test_copy_cols_masked_host(rows, k):
    _copy_case("cpu", rows, k)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k", [(1, 1), (354, 17), (2048, 64)])
def test_copy_cols_masked_gpu(rows, k):
    _copy_case("cuda", rows, k)
