"""Device::batch_pack, batch_unpack and batch_rhs (csrc/include/gj/device.hpp) against their contract, on
the host executor and on the GPU (csrc/kernels/batch.hip).

Embedding.  Every operand is an interior view of a NaN-filled parent: a stack is a 3-D strided view
whose matrices are separated by NaN rows and whose rows are wider than the view, so that a finite
result proves no pitch gap was read.  Every output sits inside a sentinel-filled parent; after the call
every byte outside the writable set is compared with a copy taken before.

pack / unpack are exact: compared bit for bit against numpy (np.ldexp, negation, astype), NaN positions
compared as positions.  The norm is a sum in the op's own order: compared within n roundings, and the
exponent must be the rule applied to the norm the op returned.

batch_rhs.  Reference: the longdouble product from the operands as stored.  Componentwise
    |got - ref| <= gamma(n + 2) (|C_in| + |M| |V|),   gamma(q) = q u / (1 - q u),  u = 2^-53
for both dtypes (an fp32 element of M is widened exactly and the arithmetic is fp64): n multiply-adds
in some order give gamma(n) |M| |V|, adding C_in is one more rounding, and the last u covers the
reference's own error -- the derivation of tests/test_rhs_block_ops.py.
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
U64 = LD(2) ** -53
_TD = {"fp64": torch.float64, "fp32": torch.float32}
_ND = {"fp64": np.float64, "fp32": np.float32}
PACK_NS = [1, 5, 15, 16, 17, 64, 65, 130]
RHS_NS = [1, 3, 16, 17, 64, 65, 130]
RHS_KS = [1, 16, 17, 64]
NBS = [1, 3, 70]


def gamma(q, u=U64):
    return q * u / (1 - q * u)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _embed3(x, r0, c0, gap, ld, fill, device):
    """x (nb, rows, cols) as a strided interior view of a `fill`-filled 2-D parent: matrix b starts at row
    r0 + b * (rows + gap), column c0"""
    nb, rows, cols = x.shape
    rs = rows + gap
    parent = torch.full((r0 + nb * rs + 3, ld), fill, dtype=x.dtype)
    for b in range(nb):
        parent[r0 + b * rs:r0 + b * rs + rows, c0:c0 + cols] = x[b]
    parent = parent.to(device)
    view = parent.as_strided((nb, rows, cols), (rs * ld, ld, 1), r0 * ld + c0)
    mask = torch.zeros(parent.shape, dtype=torch.bool)
    for b in range(nb):
        mask[r0 + b * rs:r0 + b * rs + rows, c0:c0 + cols] = True
    return parent, view, mask


def _embed1(x, off, fill, device):
    parent = torch.full((x.numel() + 2 * off,), fill, dtype=x.dtype)
    parent[off:off + x.numel()] = x.reshape(-1)
    parent = parent.to(device)
    return parent, parent[off:off + x.numel()]


def _outside_unchanged(parent, before, mask, what):
    now = _bits(parent).clone()
    was = before.clone()
    now[mask] = 0
    was[mask] = 0
    assert torch.equal(now, was), f"{what}: written outside its view"


def _rule(norm):
    """equil_exponent: ldexp(norm, e) in [1, 2); 0 for a norm that is 0 or not finite"""
    e = np.zeros(norm.shape, dtype=np.int32)
    ok = np.isfinite(norm) & (norm > 0)
    e[ok] = 1 - np.frexp(norm[ok])[1]
    return e


def _same_bits_or_nan(got, ref, what):
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN positions differ"
    ib = np.int64 if got.dtype == np.float64 else np.int32
    assert np.array_equal(got.view(ib)[~gn], ref.view(ib)[~rn]), f"{what}: bits differ"


# ------------------------------------------------------------------ pack
@functools.lru_cache(maxsize=None)
def _pack_stack(n, nb):
    rng = np.random.default_rng([41, n, nb])
    A = rng.uniform(-1, 1, (nb, n, n))
    A *= np.ldexp(1.0, (np.arange(nb) * 37) % 200 - 100)[:, None, None]  # every matrix at its own scale
    if n >= 5:
        A[0, 0, 1], A[0, 1, 0] = -0.0, 0.0
        A[0, 2, 2] = np.ldexp(np.abs(A[0]).sum(axis=1).max(), -140)  # scaled: an fp32 subnormal
        A[0, 3, 3], A[0, 4, 0] = 5e-324, -3e-310                      # fp64 subnormals
        if nb >= 3:
            A[1, n - 1, 2] = np.nan
            A[2, 0, n - 1], A[2, 1, 1] = np.inf, -np.inf
        if nb > 6:
            A[5] = 0.0                          # all zero: exp = 0
            A[6] *= np.ldexp(1.0, -960)         # the whole matrix near the bottom of fp64's range
    A.setflags(write=False)
    return A


def _run_pack(device, n, nb, dt):
    native = gj.load_native()
    m = max(n, 16)
    A = _pack_stack(n, nb)
    Apar, Av, _ = _embed3(torch.from_numpy(A.copy()), 2, 3, 2, n + 6, float("nan"), device)
    ldl = nb * m + 7
    Ltpar = torch.full((m + 4, ldl), SENT, dtype=_TD[dt], device=device)
    Lt = Ltpar[2:2 + m, 3:3 + nb * m]
    ltmask = torch.zeros(Ltpar.shape, dtype=torch.bool)
    ltmask[2:2 + m, 3:3 + nb * m] = True
    npar, norm = _embed1(torch.full((nb,), SENT, dtype=torch.float64), 5, SENT, device)
    epar, exp = _embed1(torch.full((nb,), -77, dtype=torch.int32), 5, -77, device)
    before = {"A": _bits(Apar), "Lt": _bits(Ltpar), "n": _bits(npar), "e": _bits(epar)}
    ops.batch_pack(Av, Lt, norm, exp, m=m)
    name = native.last_batch_kernel()
    assert name == ("host" if device == "cpu" else f"bpack:{'f64' if dt == 'fp64' else 'f32'}"), name
    assert torch.equal(_bits(Apar), before["A"]), "A was written"
    _outside_unchanged(Ltpar, before["Lt"], ltmask, "Lt")
    om = torch.zeros(nb + 10, dtype=torch.bool)
    om[5:5 + nb] = True
    _outside_unchanged(npar, before["n"], om, "norm")
    _outside_unchanged(epar, before["e"], om, "exp")

    got_norm, got_exp = norm.cpu().numpy(), exp.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        ref_norm = np.abs(A).sum(axis=2).max(axis=1)
    assert np.array_equal(np.isnan(got_norm), np.isnan(ref_norm)), "norm: a NaN was lost or made"
    fin = np.isfinite(ref_norm)
    assert np.array_equal(got_norm[~fin & ~np.isnan(ref_norm)], ref_norm[~fin & ~np.isnan(ref_norm)])
    assert np.all(np.abs(got_norm[fin] - ref_norm[fin]) <= float(gamma(n)) * ref_norm[fin])
    assert np.array_equal(got_exp, _rule(got_norm)), "exp is not the rule of the op's own norm"
    if n >= 5 and nb > 6:
        assert got_norm[5] == 0.0 and got_exp[5] == 0

    ref = np.zeros((m, nb * m))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for b in range(nb):
            blk = np.zeros((m, m))
            blk[:n, :n] = -np.ldexp(A[b], int(got_exp[b]))
            blk[np.arange(n, m), np.arange(n, m)] = -1.0  # the identity corner, negated like the rest
            ref[:, b * m:(b + 1) * m] = blk.T                # Lt[c, b m + r] = blk[r, c]
        ref = ref.astype(_ND[dt])
    _same_bits_or_nan(Lt.cpu().contiguous().numpy(), ref, "Lt")


PACK_CASES = [(n, nb, dt) for n in PACK_NS for nb in NBS for dt in ("fp64", "fp32")]


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "n%d-nb%d-%s" % c)
def test_batch_pack_host(case):
    _run_pack("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "n%d-nb%d-%s" % c)
def test_batch_pack_gpu(case):
    _run_pack("cuda", *case)


# ------------------------------------------------------------------ unpack
def _run_unpack(device, n, nb, dt):
    native = gj.load_native()
    m = max(n, 16)
    rng = np.random.default_rng([43, n, nb])
    inv = rng.uniform(-1, 1, (nb, m, m)) * np.ldexp(1.0, (np.arange(nb) * 5) % 21 - 10)[:, None, None]
    inv = inv.astype(_ND[dt])
    if n >= 5:
        inv[0, 1, 0], inv[0, 0, 1], inv[0, 2, 2] = -0.0, 0.0, np.inf
    inv[:, n:, :] = np.nan  # outside the leading n x n: never read
    inv[:, :, n:] = np.nan
    exp = ((np.arange(nb) * 13) % 81 - 40).astype(np.int32)
    if nb >= 3:
        exp[2] = -200 if dt == "fp32" else -1100  # an underflow: rounded once, as numpy does
    valid = np.ones(nb, dtype=np.int32)
    valid[1::4] = 0  # (nb = 1: every block valid)
    inv_t = torch.from_numpy(inv).to(device)
    e_t, v_t = torch.from_numpy(exp).to(device), torch.from_numpy(valid).to(device)
    Xpar, Xv, xmask = _embed3(torch.full((nb, n, n), SENT, dtype=_TD[dt]), 3, 2, 3, n + 5, SENT, device)
    before = _bits(Xpar)
    ib = _bits(inv_t)
    ops.batch_unpack(inv_t, e_t, v_t, Xv)
    name = native.last_batch_kernel()
    assert name == ("host" if device == "cpu" else f"bunpack:{'f64' if dt == 'fp64' else 'f32'}"), name
    assert torch.equal(_bits(inv_t), ib), "inv_t was written"
    _outside_unchanged(Xpar, before, xmask, "X")
    got = Xv.cpu().contiguous().numpy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ref = np.ldexp(inv[:, :n, :n].astype(np.float64), exp[:, None, None]).astype(_ND[dt]).transpose(0, 2, 1).copy()
    ref[valid == 0] = np.nan
    _same_bits_or_nan(got, ref, "X")
    assert np.isnan(got[valid == 0]).all(), "an invalid block must give NaN"


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "n%d-nb%d-%s" % c)
def test_batch_unpack_host(case):
    _run_unpack("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "n%d-nb%d-%s" % c)
def test_batch_unpack_gpu(case):
    _run_unpack("cuda", *case)


# ------------------------------------------------------------------ batch_rhs
@functools.lru_cache(maxsize=None)
def _rhs_operands(n, nb, dt, tiny):
    """M (nb, n, n), V and C_in (nb, n, 64), and in longdouble M V and |M| |V| (once per shape and dtype with
    all 64 columns; a case with k columns uses the first k)"""
    rng = np.random.default_rng([47, n, nb])
    M = rng.uniform(-1, 1, (nb, n, n))
    M *= np.ldexp(1.0, (np.arange(n) * 7) % 21 - 10)[None, :, None]  # graded rows
    V = rng.uniform(-1, 1, (nb, n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 17 - 8)[None, None, :]
    C = rng.uniform(-1, 1, (nb, n, 64))
    if dt == "fp32":
        M = M.astype(np.float32).astype(np.float64)
    if tiny:  # below anything fp32 arithmetic could hold
        V = V * np.ldexp(1.0, -160)
        C = C * np.ldexp(1.0, -160)
    prod = np.matmul(M.astype(LD), V.astype(LD))
    absprod = np.matmul(np.abs(M).astype(LD), np.abs(V).astype(LD))
    for x in (M, V, C, prod, absprod):
        x.setflags(write=False)
    return M, V, C, prod, absprod


def _run_rhs(device, n, nb, k, dt, sign, cin_mode, masked, aligned, tiny=False, nan_v=False, twice=False):
    native = gj.load_native()
    M, V, C, prod, absprod = _rhs_operands(n, nb, dt, tiny)
    M, V = M.copy(), V[:, :, :k].copy()
    es = 8 if dt == "fp64" else 4
    if nan_v:  # column c of M_0 is zero, row c of V_0 is NaN in column 0: every Y_0[:, 0] is NaN
        c = n // 2
        M[0, :, c] = 0.0
        V[0, c, 0] = np.nan
    if aligned:
        c0, ldm, r0, gap = 16 // es * 2, -(-(n + 24) // 4) * 4, 4, 4 - n % 4 if n % 4 else 4
    else:
        c0, ldm, r0, gap = 5, (n + 11) | 1, 3, 2
    Mpar, Mv, _ = _embed3(torch.from_numpy(M).to(_TD[dt]), r0, c0, gap, ldm, float("nan"), device)
    vec = Mv.data_ptr() % 16 == 0 and (Mv.stride(1) * es) % 16 == 0 and (Mv.stride(0) * es) % 16 == 0
    assert vec == aligned, "the embedding must give the alignment the case asks for"
    Vpar, Vv, _ = _embed3(torch.from_numpy(V), 2, 3, 1, k + 7, float("nan"), device)
    cin = C[:, :, :k].copy()
    if cin_mode == "alias":
        Ypar, Yv, ymask = _embed3(torch.from_numpy(cin), 5, 4, 2, k + 9, SENT, device)
        Cpar, Cv = None, Yv
    else:
        Ypar, Yv, ymask = _embed3(torch.full((nb, n, k), SENT, dtype=torch.float64), 5, 4, 2, k + 9, SENT, device)
        Cpar, Cv = None, None
        if cin_mode == "separate":
            Cpar, Cv, _ = _embed3(torch.from_numpy(cin), 1, 2, 3, k + 3, float("nan"), device)
    on = np.ones((nb, k), dtype=bool)
    if masked:
        on.reshape(-1)[::3] = False  # (matrix 0, column 0) off, also at nb = k = 1
        if nan_v:
            on[0, 0] = True
    active = torch.from_numpy(on.astype(np.int32)).to(device) if masked else None
    cmpar, cm = _embed1(torch.full((nb * k,), SENT, dtype=torch.float64), 6, SENT, device)
    before = {nm: _bits(t) for nm, t in (("M", Mpar), ("V", Vpar), ("Y", Ypar), ("C", Cpar), ("cm", cmpar))
              if t is not None}
    y_in = Yv.cpu().numpy().copy()

    def launch():
        ops.batch_rhs(Mv, Vv, Yv, C_in=Cv, sign=sign, active=active, colmax=cm)

    launch()
    name = native.last_batch_kernel()
    if device == "cpu":
        assert name == "host"
    else:
        kw = 16 if k <= 16 else 32 if k <= 32 else 64
        assert name == f"brhs{kw}:{'f64' if dt == 'fp64' else 'f32'}:{'vec' if aligned else 'scalar'}", name
    got = Yv.cpu().numpy().copy()
    got_cm = cm.cpu().numpy().copy().reshape(nb, k)
    if twice and cin_mode != "alias":
        y1, c1 = _bits(Ypar), _bits(cmpar)
        launch()
        assert torch.equal(_bits(Ypar), y1) and torch.equal(_bits(cmpar), c1), "two launches differ"

    for nm, par in (("M", Mpar), ("V", Vpar), ("C", Cpar)):
        if par is not None:
            assert torch.equal(_bits(par), before[nm]), f"{nm} was written"
    _outside_unchanged(Ypar, before["Y"], ymask, "Y")
    cmm = torch.zeros(nb * k + 12, dtype=torch.bool)
    cmm[6:6 + nb * k] = True
    _outside_unchanged(cmpar, before["cm"], cmm, "colmax")

    # inactive (matrix, column) pairs: bitwise untouched, and so are their colmax entries
    off = ~on
    offm = np.broadcast_to(off[:, None, :], got.shape)
    assert np.array_equal(got.view(np.int64)[offm], y_in.view(np.int64)[offm]), "an inactive column was written"
    assert np.all(got_cm[off] == SENT), "the colmax of an inactive column was written"

    cterm = 0 if cin_mode == "null" else cin.astype(LD)
    prod, absprod = prod[:, :, :k], absprod[:, :, :k]
    if nan_v:  # matrix 0 was edited: its reference again (its NaN column is checked on its own)
        prod, absprod = prod.copy(), absprod.copy()
        with np.errstate(invalid="ignore"):
            prod[0] = M[0].astype(LD) @ V[0].astype(LD)
            absprod[0] = np.abs(M[0]).astype(LD) @ np.abs(V[0]).astype(LD)
    ref = cterm + LD(sign) * prod
    bound = gamma(n + 2) * (np.abs(cterm) + absprod)
    onm = np.broadcast_to(on[:, None, :], got.shape).copy()
    if nan_v:
        assert np.isnan(got[0, :, 0]).all(), "a NaN of V must reach Y through a zero of M"
        assert np.isnan(got_cm[0, 0]), "colmax must keep the NaN"
        onm[0, :, 0] = False
    assert np.isfinite(got[onm]).all(), "a pitch gap or a masked operand was read"
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err[onm] <= bound[onm]), float((err[onm] / np.maximum(bound[onm], LD(1e-4000))).max())
    if tiny:
        assert np.all(got[onm] != 0.0) and np.abs(got[onm]).max() < 1e-40
    # colmax = the maximum of |Y| as the op wrote it, exactly
    want_cm = np.abs(got).max(axis=1)
    chk = on.copy()
    if nan_v:
        chk[0, 0] = False
    assert np.array_equal(got_cm[chk], want_cm[chk]), "colmax is not max |Y|"


def _rhs_cases():
    out = []
    combos = itertools.product(RHS_NS, RHS_KS, NBS, ("fp64", "fp32"))
    for i, (n, k, nb, dt) in enumerate(combos):
        sign = 1.0 if (i // 7) % 2 == 0 else -1.0
        cin = ("null", "alias", "separate")[(i // 2) % 3]
        masked = (i // 3) % 2 == 1
        aligned = (i // 5) % 2 == 0
        out.append((n, nb, k, dt, sign, cin, masked, aligned))
    return out


RHS_CASES = _rhs_cases()
_rid = lambda c: "n%d-nb%d-k%d-%s-s%+d-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "mask" if c[6] else "all",  # noqa: E731
                                                    "vec" if c[7] else "scalar")
# both alignments, both signs and the three C_in modes meet both dtypes
assert {(c[3], c[7]) for c in RHS_CASES} == set(itertools.product(("fp64", "fp32"), (True, False)))
assert {(c[3], c[5]) for c in RHS_CASES} == set(itertools.product(("fp64", "fp32"), ("null", "alias", "separate")))
assert {(c[3], c[4]) for c in RHS_CASES} == set(itertools.product(("fp64", "fp32"), (1.0, -1.0)))
FLAG_CASES = [  # (n, nb, k, dt, sign, cin, masked, aligned, tiny, nan_v, twice)
    (65, 3, 17, "fp32", 1.0, "separate", False, True, True, False, False),    # V at 2^-160 under fp32 storage
    (17, 3, 16, "fp32", -1.0, "null", True, False, True, False, False),
    (64, 3, 17, "fp64", 1.0, "separate", True, True, False, True, False),     # NaN of V through a zero of M
    (17, 1, 1, "fp32", -1.0, "null", False, False, False, True, False),
    (130, 70, 64, "fp64", -1.0, "separate", True, True, False, False, True),  # two launches, the same bits
    (65, 3, 17, "fp32", 1.0, "null", False, False, False, False, True),
]


@pytest.mark.parametrize("case", RHS_CASES, ids=_rid)
def test_batch_rhs_host(case):
    _run_rhs("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RHS_CASES, ids=_rid)
def test_batch_rhs_gpu(case):
    _run_rhs("cuda", *case)


@pytest.mark.parametrize("case", FLAG_CASES, ids=lambda c: _rid(c[:8]) + "-%d%d%d" % tuple(int(x) for x in c[8:]))
def test_batch_rhs_flags_host(case):
    _run_rhs("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FLAG_CASES, ids=lambda c: _rid(c[:8]) + "-%d%d%d" % tuple(int(x) for x in c[8:]))
def test_batch_rhs_flags_gpu(case):
    _run_rhs("cuda", *case)


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_batch_rhs_refuses_bad_k(device):
    native = gj.load_native()
    M = torch.zeros((2, 4, 4), dtype=torch.float64, device=device)
    for k in (0, 65):
        V = torch.zeros((2, 4, max(k, 1)), dtype=torch.float64, device=device)
        with pytest.raises(native.GJError):
            ops.device_for(V).batch_rhs("fp64", M.data_ptr(), 16, 4, 4, 2, V.data_ptr(), 4 * max(k, 1), max(k, 1), k, 0, 0,
                                        0, V.data_ptr(), 4 * max(k, 1), max(k, 1), 1.0)
