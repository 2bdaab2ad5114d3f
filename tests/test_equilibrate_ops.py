"""Device::abs_max_rows, abs_max_cols and scale_pow2 (csrc/include/gj/device.hpp) against their
contract, on the host executor and on the GPU (csrc/kernels/equilibrate.hip).

    abs_max_rows  out_nat[grow(r)] = max_{c<n} |X[r][c]|                      this rank's real rows
    abs_max_cols  out[c] = max_r ldexp(|X[r][c]|, rexp_nat[grow(r)])          c < n, written (+0.0 without rows)
    scale_pow2    X[r][c] = round_dt(ldexp(X[r][c], rexp_nat[grow(r)] + cexp[c]))  in place

Embedding (the method of test_rank_update_ops.py).  X is an interior view of a NaN-filled parent with
a leading dimension wider than the view; NaN sits in X's local padding rows, in its columns >= n and
in the pitch gap.  The exponent vectors are int32, which has no NaN: the entries the contract says are
never read (other ranks' rows, rows >= n, everything around the vectors) hold a poison exponent that
would turn every value it touched into 0 or Inf.  Every output sits inside a longer buffer of
sentinels.  After each call every byte outside the written region is compared with a copy taken
before.  The views of X are placed 16-byte aligned or not, the two load paths of the GPU kernels, and
the probe must say "vec" and "scalar" respectively.

Reference.  Magnitudes, maxima and scaling by a power of two are exact, so the expected values come
from np.abs / np.ldexp (one correct rounding where a result is subnormal; the conversion to fp32 is
numpy's round-to-nearest-even) and every comparison is bitwise.

Cases.  (n, m) in {(1, 8), (15, 8), (64, 16), (65, 16), (130, 128), (300, 128)} -- one element, less
than one 16-byte access, whole and ragged 64-column strips, more than one strip, several row groups --
each at p = 1 and as ranks 0 and 2 of p = 3, plus n = 10, m = 8 as rank 2 of 3 (a rank without rows);
both dtypes; both alignments.  Data are random values times 2^(random exponent), the exponents within
+-80 for fp64 and +-30 for fp32 (so that no fp32 result leaves the normal range by accident).
"""
import functools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

SHAPES = [(n, m, p, r) for (n, m) in ((1, 8), (15, 8), (64, 16), (65, 16), (130, 128), (300, 128))
          for (p, r) in ((1, 0), (3, 0), (3, 2))] + [(10, 8, 3, 2)]
DTS = ("fp64", "fp32")
_TD = {"fp64": torch.float64, "fp32": torch.float32}
_ND = {"fp64": np.float64, "fp32": np.float32}
ERANGE = {"fp64": 80, "fp32": 30}
POISON = 50000  # an exponent that takes any finite value to 0 or Inf
SENT = -7.0     # no maximum is negative


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(Nr=Nr, npad=Nr * m, nblk=nblk, rows=rows, grow=grow, real=grow < n)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """X (real rows x n, representable in dt), rexp (n, natural order) and cexp (n)"""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    E = ERANGE[dt]
    rng = np.random.default_rng([41, n, m, p, rank])
    R = int(L["real"].sum())
    X = np.ldexp(rng.uniform(-1, 1, (R, n)), rng.integers(-E, E + 1, (R, n)))
    X = X.astype(_ND[dt]).astype(np.float64)
    rexp = rng.integers(-E, E + 1, n).astype(np.int32)
    cexp = rng.integers(-E, E + 1, n).astype(np.int32)
    for a in (X, rexp, cexp):
        a.setflags(write=False)
    return X, rexp, cexp


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _np_bits(a):
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


class _Case:
    """the embedded operands of one shape / dtype / alignment on a device"""

    def __init__(self, device, shape, dt, aligned, X=None, rexp=None, cexp=None):
        n, m, p, rank = shape
        self.shape, self.dt, self.device, self.aligned = shape, dt, device, aligned
        self.L = L = _layout(n, m, p, rank)
        rows, npad, real = L["rows"], L["npad"], L["real"]
        self.R = int(real.sum())
        self.own = L["grow"][real]
        X0, rexp0, cexp0 = _operands(shape, dt)
        self.X = X0 if X is None else X
        rexp = rexp0 if rexp is None else rexp
        cexp = cexp0 if cexp is None else cexp
        self.rexp, self.cexp = rexp, cexp
        es = 8 if dt == "fp64" else 4
        Xfull = np.full((rows, npad), np.nan)
        Xfull[real, :n] = self.X
        if aligned:
            self.c0, ldx = 16 // es * 2, -(-(npad + 24) // 4) * 4
        else:
            self.c0, ldx = 5, (npad + 11) | 1
        self.r0 = 3
        par = torch.full((rows + self.r0 + 5, ldx), float("nan"), dtype=_TD[dt])
        par[self.r0:self.r0 + rows, self.c0:self.c0 + npad] = torch.from_numpy(Xfull).to(_TD[dt])
        self.Xpar = par.to(device)
        self.Xv = self.Xpar[self.r0:self.r0 + rows, self.c0:self.c0 + npad]
        if rows:
            assert (self.Xv.data_ptr() % 16 == 0 and (self.Xv.stride(0) * es) % 16 == 0) == aligned
        # exponents: poison wherever the contract says "never read"
        rfull = np.full(npad + 9, POISON, np.int32)
        rfull[4 + self.own] = rexp[self.own]
        self.rpar = torch.from_numpy(rfull).to(device)
        self.rv = self.rpar[4:4 + npad]
        cfull = np.full(n + 9, POISON, np.int32)
        cfull[3:3 + n] = cexp
        self.cpar = torch.from_numpy(cfull).to(device)
        self.cv = self.cpar[3:3 + n]
        self.before = {k: _bits(t) for k, t in (("X", self.Xpar), ("r", self.rpar), ("c", self.cpar))}

    def probe(self, op):
        name = gj.load_native().last_equil_kernel()
        if self.device == "cpu":
            assert name == "host"
            return
        exp = f"eq:{op}:{'f64' if self.dt == 'fp64' else 'f32'}:{'vec' if self.aligned else 'scalar'}"
        assert name == exp or (self.L["rows"] == 0 and name.startswith(exp.rsplit(":", 1)[0])), (name, exp)

    def unchanged(self, *names):
        for k, t in (("X", self.Xpar), ("r", self.rpar), ("c", self.cpar)):
            if k in names:
                assert torch.equal(_bits(t), self.before[k]), f"{k} was written"

    # magnitudes with NaN and Inf counted as +Inf
    def mags(self):
        a = np.abs(self.X)
        return np.where(np.isfinite(a), a, np.inf)

    def row_max(self):
        n, npad = self.shape[0], self.L["npad"]
        out = torch.full((npad + 8,), SENT, dtype=torch.float64, device=self.device)
        ops.abs_max_rows(self.Xv, out[3:], n, *self.shape[1:])
        self.probe("rmax")
        self.unchanged("X", "r", "c")
        want = np.full(npad + 8, SENT)
        if self.R:
            want[3 + self.own] = self.mags().max(axis=1)
        got = out.cpu().numpy()
        assert np.array_equal(_np_bits(got), _np_bits(want)), "abs_max_rows"
        return got[3:3 + n]

    def col_max(self, with_rexp=True):
        n = self.shape[0]
        out = torch.full((n + 8,), SENT, dtype=torch.float64, device=self.device)
        ops.abs_max_cols(self.Xv, out[3:3 + n], n, *self.shape[1:], rexp_nat=self.rv if with_rexp else None)
        self.probe("cmax")
        self.unchanged("X", "r", "c")
        want = np.full(n + 8, SENT)
        want[3:3 + n] = 0.0
        if self.R:
            e = self.rexp[self.own][:, None] if with_rexp else 0
            with np.errstate(over="ignore"):
                want[3:3 + n] = np.ldexp(self.mags(), e).max(axis=0)
        got = out.cpu().numpy()
        assert np.array_equal(_np_bits(got), _np_bits(want)), "abs_max_cols"
        return got[3:3 + n]

    def scale(self, with_rexp=True, with_cexp=True):
        n = self.shape[0]
        ops.scale_pow2(self.Xv, n, *self.shape[1:], rexp_nat=self.rv if with_rexp else None,
                       cexp=self.cv if with_cexp else None)
        self.probe("scale")
        self.unchanged("r", "c")
        a, b = _bits(self.Xpar).clone(), self.before["X"].clone()
        sl = (slice(self.r0, self.r0 + self.R), slice(self.c0, self.c0 + n))
        a[sl] = 0
        b[sl] = 0
        assert torch.equal(a, b), "write outside X's real rows x n columns"
        e = (self.rexp[self.own][:, None] if with_rexp else 0) + (self.cexp[None, :] if with_cexp else 0)
        with np.errstate(over="ignore", under="ignore"):
            want = np.ldexp(self.X, e).astype(_ND[self.dt])
        got = self.Xv[:self.R, :n].cpu().numpy()
        return got, want


def _same(got, want):
    """bitwise, except that any NaN matches any NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_np_bits(np.where(nan, 0, got)), _np_bits(np.where(nan, 0, want)))


def _run_case(device, shape, dt, aligned):
    c = _Case(device, shape, dt, aligned)
    c.row_max()
    c.col_max(True)
    c.col_max(False)
    got, want = c.scale()
    _same(got, want)
    if c.R:
        assert np.isfinite(got).all() and (got != c.X.astype(_ND[dt])).any()


_CASES = [(s, dt, al) for s in SHAPES for dt in DTS for al in (True, False)]


def _id(c):
    s = c[0]
    return f"n{s[0]}m{s[1]}p{s[2]}r{s[3]}-{c[1]}-{'al' if c[2] else 'mis'}"


@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_equilibrate_ops_host(case):
    _run_case("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_equilibrate_ops_gpu(case):
    _run_case("cuda", *case)


def _one_sided(device):
    # only row exponents, only column exponents, neither (the identity, bit for bit)
    for dt in DTS:
        for wr, wc in ((True, False), (False, True), (False, False)):
            c = _Case(device, (65, 16, 3, 0), dt, dt == "fp64")
            _same(*c.scale(wr, wc))


def test_one_sided_host():
    _one_sided("cpu")


@pytest.mark.gpu
def test_one_sided_gpu():
    _one_sided("cuda")


def _nonfinite(device):
    # a NaN and an Inf inside the real region give +Inf in exactly their row and column
    shape = (130, 128, 3, 0)
    for dt in DTS:
        X = _operands(shape, dt)[0].copy()
        (r1, c1), (r2, c2) = (5, 129), (77, 0)
        X[r1, c1] = np.nan
        X[r2, c2] = -np.inf
        c = _Case(device, shape, dt, dt == "fp32", X=X)
        rm = c.row_max()  # (compared bitwise with the +Inf-keyed reference inside)
        inf_rows = set(np.nonzero(np.isinf(rm))[0])
        assert inf_rows == {int(c.own[r1]), int(c.own[r2])} and not np.isnan(rm).any()
        for with_rexp in (True, False):
            cm = c.col_max(with_rexp)
            assert set(np.nonzero(np.isinf(cm))[0]) == {c1, c2} and not np.isnan(cm).any()


def test_nonfinite_host():
    _nonfinite("cpu")


@pytest.mark.gpu
def test_nonfinite_gpu():
    _nonfinite("cuda")


def _special_values(device):
    # scale_pow2 keeps NaN, +-Inf and +-0 with its sign; an underflow rounds once (gradually), an
    # overflow gives +-Inf.  Row 1 is scaled down and row 2 up, so that their elements can be normal
    # numbers whose results are not.
    shape = (15, 8, 1, 0)
    for dt in DTS:
        X = _operands(shape, dt)[0].copy()
        rexp = _operands(shape, dt)[1].copy()
        rexp[1], rexp[2] = (-60, 60) if dt == "fp64" else (-40, 40)
        cexp = (np.arange(15) % 5 - 2).astype(np.int32)
        lo, hi = (-1074, 1024) if dt == "fp64" else (-149, 128)
        X[0, :5] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
        # row 1: results in the subnormal range (a full mantissa, so the rounding shows) and past it
        # row 2: results that overflow, of both signs
        for j in range(15):
            e = int(rexp[1]) + int(cexp[j])
            X[1, j] = np.ldexp(-1.2345678901234567 if j % 2 else 1.7654321098765432, (lo + 3 + j % 11) - e)
            e = int(rexp[2]) + int(cexp[j])
            X[2, j] = np.ldexp(-1.5 if j % 2 else 1.5, hi - 1 + (j % 3) - e)
        X = X.astype(_ND[dt]).astype(np.float64)
        assert np.isfinite(X[1:3]).all() and (X[1:3] != 0).all()
        c = _Case(device, shape, dt, dt == "fp64", X=X, rexp=rexp, cexp=cexp)
        got, want = c.scale()
        _same(got, want)
        assert np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[0, 2] == -np.inf
        assert got[0, 3] == 0 and not np.signbit(got[0, 3]) and got[0, 4] == 0 and np.signbit(got[0, 4])
        tiny_n = np.finfo(_ND[dt]).tiny
        sub = (np.abs(got[1]) < tiny_n) & (got[1] != 0)
        assert sub.sum() >= 5, "no subnormal result in the case"
        assert np.isinf(got[2]).sum() >= 5 and np.isfinite(got[2]).sum() >= 1
        assert (np.sign(got[2]) == np.sign(X[2])).all()


def test_special_values_host():
    _special_values("cpu")


@pytest.mark.gpu
def test_special_values_gpu():
    _special_values("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [2, 3, 7, 1000])
def test_forced_row_split_gpu(split):
    # the column maxima with the rows split over workgroups: the same bits as the reference whatever
    # the split (1000 > the rows of every case: one row per slice at the most)
    native = gj.load_native()
    native.set_equil_col_split(split)
    try:
        for shape, dt, al in (((300, 128, 1, 0), "fp64", True), ((65, 16, 3, 0), "fp32", False),
                              ((130, 128, 3, 2), "fp64", False), ((10, 8, 3, 2), "fp32", True)):
            c = _Case("cuda", shape, dt, al)
            c.col_max(True)
            c.col_max(False)
    finally:
        native.set_equil_col_split(0)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_gpu_bit_identical_and_cache_policy(dt):
    # two launches give the same bits, and so does the plain cache policy of scale_pow2
    native = gj.load_native()
    shape = (300, 128, 1, 0)
    a, _ = _Case("cuda", shape, dt, True).scale()
    b, _ = _Case("cuda", shape, dt, True).scale()
    native.set_equil_nt(False)
    try:
        c, want = _Case("cuda", shape, dt, True).scale()
    finally:
        native.set_equil_nt(True)
    assert np.array_equal(_np_bits(a), _np_bits(b)) and np.array_equal(_np_bits(a), _np_bits(c))
    _same(a, want)


def _huge_leading_dimension(device):
    # rows are addressed with 64-bit offsets: a leading dimension beyond 2^31 bytes is accepted and
    # computed right (one row, n = m = 1: the view is valid whatever its row stride)
    for dt in DTS:
        X = torch.full((1, 1), -3.0, dtype=_TD[dt], device=device)
        Xv = X.as_strided((1, 1), (2 ** 31 + 5, 1))
        e = torch.tensor([3], dtype=torch.int32, device=device)
        out = torch.zeros(1, dtype=torch.float64, device=device)
        assert float(ops.abs_max_rows(Xv, out, 1, 1)[0]) == 3.0
        assert float(ops.abs_max_cols(Xv, out, 1, 1, rexp_nat=e)[0]) == 24.0
        ops.scale_pow2(Xv, 1, 1, rexp_nat=e, cexp=e)
        assert float(X[0, 0]) == -192.0


def test_huge_leading_dimension_host():
    _huge_leading_dimension("cpu")


@pytest.mark.gpu
def test_huge_leading_dimension_gpu():
    _huge_leading_dimension("cuda")
