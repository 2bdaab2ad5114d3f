"""Device::panel_rhs_dd (csrc/include/gj/device.hpp) against its contract, on the host executors and
on the GPU (csrc/kernels/panel_rhs_dd.hip).

panel_rhs_dd: Y = round_fp64(C_in - P V) over the columns c < n for this rank's rows of an fp64
panel, the whole sum, C_in included, carried as an unevaluated pair of doubles (Dot2) and rounded once.

Embedding, as in test_rhs_block_ops.py.  Every operand is an interior view of a NaN-filled parent with
a leading dimension wider than the view; what the contract says is never read holds NaN as well: the
padding columns of P (c >= n), P's local padding rows (global row >= n), the rows >= n of V and every
pitch gap.  Y and colmax sit inside a sentinel-filled parent; after the call every byte outside the
writable set is compared with a copy taken before.  The views are placed 16-byte aligned or not
("vec" / "scalar"), the two load paths of the GPU kernel.

Reference.  Exact rational arithmetic: fractions.Fraction from the operands as stored.  P and V are
drawn on a grid (an integer below 2^53 times a power of two per row / column, full 53-bit mantissas
for the large entries), so that the exact products can be summed by integer matrix products of 18-bit
pieces (every partial sum < 2^46: exact in int64) and put together as Python integers; the Fraction of
element (r, j) is Fraction(C_in) - Fraction(sum, 2^106) * 2^(row exponent + column exponent).  All 64
columns of a shape are computed once and cached.

Bound, componentwise, with S = |C_in| + |P| |V| and u = 2^-53:
    |got - ref| <= u |ref| + 4 ((n + 2) u)^2 S.
Derived, not measured: Dot2's theorem (Ogita, Rump, Oishi 2005) gives u |ref| + gamma(n)^2 S for n
terms; C_in and the fixed-order sum of the K lanes and K-slices add at most two levels; the factor 4
covers double-double additions of relative error 2 u^2.  S is taken from an fp64 product shrunk by
(1 - 1e-12), a lower bound of the exact S, so the test asks no less than the bound above.

Operands with heavy cancellation, so that the bound discriminates: C_in = fl(P V) + rho with |rho|
about 1e-10 S.  A result accumulated in fp64 then misses the bound by about ten orders, and the test
asserts that ops.panel_rhs (sign -1) does miss it on the same case.

Cases.  (n, m, p, rank) = (300, 16, 1, 0), (1003, 59, 3, each rank), (1000, 59, 3, 1); k in {1, 16,
17, 40, 64}; the C_in mode (null / aliasing Y / separate), the active mask (null / some columns off)
and the alignment rotate over the cases; on the GPU the K-split forced to 1, 2, 7 and auto, with
native.last_rhs_dd_kernel() asserted.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

SENT = -777.25
SHAPES = [(300, 16, 1, 0), (1003, 59, 3, 0), (1003, 59, 3, 1), (1003, 59, 3, 2), (1000, 59, 3, 1)]
KS = [1, 16, 17, 40, 64]
SPLITS = [1, 2, 7, 0]
CIN_MODES = ["null", "alias", "separate"]
U = Fraction(1, 2 ** 53)


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n)


def _exact_products(Pi, Vi):
    """sum_c Pi[r, c] * Vi[c, j] for int64 arrays of magnitude < 2^54, exactly, as Python integers"""
    def pieces(X):
        s, a = np.sign(X), np.abs(X)
        return [s * ((a >> (18 * q)) & 0x3FFFF) for q in range(3)]
    out = np.zeros((Pi.shape[0], Vi.shape[1]), dtype=object)
    for qa, pa in enumerate(pieces(Pi)):
        for qb, vb in enumerate(pieces(Vi)):
            out += (pa @ vb).astype(object) * (1 << (18 * (qa + qb)))  # n 2^36 < 2^46: exact in int64
    return out


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """P (rows x n), V (n x 64), C_in (rows x 64, the cancelling one) and, exactly, P V as integers with
    their exponents; the fp64 lower bound of |P| |V|.  Once per shape, all 64 columns."""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows = L["rows"]
    rng = np.random.default_rng([29, n, m, p, rank])
    Pi = rng.integers(-2 ** 53, 2 ** 53, (rows, n), dtype=np.int64)
    Vi = rng.integers(-2 ** 53, 2 ** 53, (n, 64), dtype=np.int64)
    Pi[:, ::7] = 0  # zeros of P: the terms a NaN of V must pass through
    # graded rows and columns: an absolute tolerance would hide whole rows
    pe = (np.arange(rows) * 7) % 21 - 10 - 53
    ve = (np.arange(64) * 5) % 17 - 8 - 53
    P = np.ldexp(Pi.astype(np.float64), pe[:, None])  # exact: |Pi| <= 2^53
    V = np.ldexp(Vi.astype(np.float64), ve[None, :])
    prod = _exact_products(Pi, Vi)  # P V = prod * 2^(pe + ve)
    S = (np.abs(P) @ np.abs(V)) * (1 - 1e-12)
    rho = 1e-10 * S * rng.choice([-1.0, 1.0], S.shape) * rng.uniform(0.5, 1.0, S.shape)
    Cin = P @ V + rho
    for x in (P, V, Cin, S):
        x.setflags(write=False)
    return P, V, Cin, prod, pe, ve, S


def _frac_product(prod, pe, ve, r, j):
    e = int(pe[r]) + int(ve[j])
    return Fraction(int(prod[r, j])) * (Fraction(2) ** e)


def _embed(t, r0, c0, ld, fill, device, extra_rows=9):
    """t as an interior view of a `fill`-filled parent with leading dimension ld"""
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), fill, dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to(device)
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _expected_name(k, P, split):
    kw = 16 if k <= 16 else 32 if k <= 32 else 64
    vec = P.data_ptr() % 16 == 0 and (P.stride(0) * 8) % 16 == 0
    head = f"rhsdd{kw}:f64:{'vec' if vec else 'scalar'}:s"
    return head if split == 0 else head + str(split)


def _misses(got, ref_of, S, cin0, real_rows, cols, n):
    """the elements (local row, column) outside the bound, and the largest error in units of the bound"""
    c2 = 4 * (Fraction(n + 2) * U) ** 2
    bad, worst = [], Fraction(0)
    for r in real_rows:
        for j in cols:
            ref = ref_of(r, j)
            err = abs(Fraction(float(got[r, j])) - ref)
            bound = U * abs(ref) + c2 * (Fraction(float(abs(cin0[r, j]))) + Fraction(float(S[r, j])))
            if err > bound:
                bad.append((r, j))
            if bound > 0:
                worst = max(worst, err / bound)
    return bad, float(worst)


def _run_case(device, shape, k, cin_mode, masked, aligned, split=0, twice=False, executor=None, check_plain=False):
    native = gj.load_native()
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad = L["rows"], L["npad"]
    P, V, Cin, prod, pe, ve, S = _operands(shape)
    # P: the panel is rows x npad; columns >= n and local padding rows are NaN
    Pfull = np.full((rows, npad), np.nan)
    Pfull[:, :n] = P
    Pfull[~L["real"], :] = np.nan
    if aligned:
        c0, ldp = 4, -(-(npad + 24) // 4) * 4
    else:
        c0, ldp = 5, (npad + 11) | 1
    Ppar, Pv = _embed(torch.from_numpy(Pfull), 3, c0, ldp, float("nan"), device)
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * 8) % 16 == 0) == aligned or rows == 0
    # V: n real rows, then NaN rows up to npad and beyond
    Vpar, Vv = _embed(torch.from_numpy(V[:, :k].copy()), 2, 3, k + 7, float("nan"), device, extra_rows=npad - n + 9)
    cin = Cin[:, :k].copy()
    if cin_mode == "alias":
        Ypar, Yv = _embed(torch.from_numpy(cin), 8, 5, k + 13, SENT, device)
        Cv, Cpar = Yv, None
    else:
        Ypar, Yv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT, device)
        Cpar, Cv = (None, None) if cin_mode == "null" else _embed(torch.from_numpy(cin), 1, 2, k + 3, float("nan"),
                                                                   device)
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
            ops.panel_rhs_dd(Pv, Vv, Yv, n, m, p, rank, C_in=Cv, active=active, colmax=cm, ncols=k, device=executor)
        finally:
            if device != "cpu":
                native.set_rhs_splitk(0)

    launch()
    name = native.last_rhs_dd_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        exp = _expected_name(k, Pv, split)
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
    yb, ybefore = _bits(Ypar).clone(), before["Y"].clone()
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
    # real rows: the bound, in exact arithmetic
    assert np.isfinite(got[real][:, on]).all()
    real_rows, cols = np.nonzero(real)[0], np.nonzero(on)[0]

    def ref_of(r, j):
        return Fraction(float(cin0[r, j])) - _frac_product(prod, pe, ve, r, j)

    bad, worst = _misses(got, ref_of, S, cin0, real_rows, cols, n)
    assert not bad, (len(bad), bad[:3], worst)
    # colmax: the maximum over the real rows of what was written
    for j in cols:
        col = np.abs(got[real, j])
        want = col.max() if col.size else 0.0
        assert got_cm[j] == want, (j, got_cm[j], want)
    if check_plain and cin_mode != "null":
        # the honesty check: the fp64-accumulated residual of the same case is far outside the bound
        Y2 = torch.full((rows, k), SENT, dtype=torch.float64, device=device)
        ops.panel_rhs(Pv, Vv, Y2, n, m, p, rank, C_in=(Cv if cin_mode == "separate" else torch.from_numpy(cin).to(device)),
                      sign=-1.0, ncols=k)
        bad2, worst2 = _misses(Y2.cpu().numpy(), ref_of, S, cin0, real_rows[:40], cols, n)
        assert len(bad2) > 0.9 * len(real_rows[:40]) * len(cols) and worst2 > 1e6, (len(bad2), worst2)
    return got, got_cm


def _rotation(i):
    """C_in mode, masked, aligned for case number i: the 12 combinations in turn"""
    combos = list(itertools.product(CIN_MODES, [False, True], [True, False]))
    return combos[i % len(combos)]


_HOST_CASES = [(s, k) for s in SHAPES for k in KS]
_GPU_CASES = [(s, k, sp) for s in SHAPES for k in KS for sp in SPLITS]


def _id(c):
    s = c[0]
    tail = "" if len(c) < 3 else f"-split{c[2]}"
    return f"n{s[0]}m{s[1]}p{s[2]}r{s[3]}-k{c[1]}{tail}"


@pytest.mark.parametrize("case", _HOST_CASES, ids=_id)
def test_panel_rhs_dd_host(case):
    shape, k = case
    cin_mode, masked, aligned = _rotation(7 * _HOST_CASES.index(case))
    _run_case("cpu", shape, k, cin_mode, masked, aligned)


@pytest.mark.parametrize("k", [1, 17, 64])
def test_panel_rhs_dd_async_host(k):
    native = gj.load_native()
    _run_case("cpu", (1000, 59, 3, 1), k, "separate", k == 17, False, executor=native.async_host_device())


@pytest.mark.gpu
@pytest.mark.parametrize("case", _GPU_CASES, ids=_id)
def test_panel_rhs_dd_gpu(case):
    shape, k, split = case
    # 5 is coprime to 12: the four splits of one shape and k take different combinations, and over the
    # list every combination meets every split
    cin_mode, masked, aligned = _rotation(5 * _GPU_CASES.index(case))
    _run_case("cuda", shape, k, cin_mode, masked, aligned, split=split)


def test_fp64_accumulation_misses_the_bound_host():
    _run_case("cpu", (300, 16, 1, 0), 17, "separate", False, True, check_plain=True)


@pytest.mark.gpu
def test_fp64_accumulation_misses_the_bound_gpu():
    _run_case("cuda", (1003, 59, 3, 1), 40, "separate", False, True, check_plain=True)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
def test_panel_rhs_dd_gpu_bit_identical(split):
    for shape, k, aligned in (((1003, 59, 3, 0), 17, False), ((1000, 59, 3, 1), 64, True), ((300, 16, 1, 0), 16, True)):
        _run_case("cuda", shape, k, "separate", True, aligned, split=split, twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 40, 64])
def test_gpu_and_host_agree_within_the_bound(k):
    # both are inside the bound around the exact value (_run_case), hence within twice the bound of each
    # other; they need not agree to the bit
    shape = (1003, 59, 3, 2)
    g, _ = _run_case("cuda", shape, k, "separate", False, True)
    h, _ = _run_case("cpu", shape, k, "separate", False, True)
    P, V, Cin, prod, pe, ve, S = _operands(shape)
    real = _layout(*shape)["real"]
    c2 = float(4 * (Fraction(shape[0] + 2) * U) ** 2)
    bound = 2.0 ** -53 * np.maximum(np.abs(g), np.abs(h)) + c2 * (np.abs(Cin[:, :k]) + S[:, :k])
    assert (np.abs(g - h)[real] <= 2 * bound[real]).all()


def _nan_case(device):
    # a NaN of V reaches every element of its column of Y, also through the zeros of P (every 7th
    # column of P is 0, row 7 of V meets only those); the other columns stay finite
    n, m, p, rank = shape = (300, 16, 1, 0)
    P, V, Cin, *_ = _operands(shape)
    k = 5
    assert not P[:, 7].any()
    Vn = V[:, :k].copy()
    Vn[7, 3] = np.nan
    Pv = torch.from_numpy(P.copy()).to(device)
    Y = torch.zeros((P.shape[0], k), dtype=torch.float64, device=device)
    cm = torch.zeros(k, dtype=torch.float64, device=device)
    ops.panel_rhs_dd(Pv, torch.from_numpy(Vn).to(device), Y, n, m, p, rank, colmax=cm)
    y, c = Y.cpu().numpy(), cm.cpu().numpy()
    real = _layout(*shape)["real"]
    assert np.isnan(y[real, 3]).all() and np.isfinite(np.delete(y, 3, axis=1)).all()
    assert np.isnan(c[3]) and np.isfinite(np.delete(c, 3)).all()


def test_nan_through_zero_host():
    _nan_case("cpu")


@pytest.mark.gpu
def test_nan_through_zero_gpu():
    _nan_case("cuda")


def _bad_args(device):
    n, m = 64, 16
    V = torch.zeros((n, 80), dtype=torch.float64, device=device)
    Y = torch.zeros((n, 80), dtype=torch.float64, device=device)
    P = torch.zeros((n, n), dtype=torch.float64, device=device)
    for k in (0, 65):
        with pytest.raises(RuntimeError):
            ops.panel_rhs_dd(P, V, Y, n, m, ncols=k)
    with pytest.raises(RuntimeError):  # the panel is fp64
        ops.panel_rhs_dd(P.to(torch.float32), V, Y, n, m, ncols=4)
    assert float(Y.abs().max()) == 0.0
    ops.panel_rhs_dd(P, V, Y, n, m, ncols=64)


def test_bad_args_host():
    _bad_args("cpu")


@pytest.mark.gpu
def test_bad_args_gpu():
    _bad_args("cuda")
