"""gj.batched end to end: inverse, refined solve, slogdet and rcond of a stack (..., n, n), on the host
executor and on the GPU.

Bounds (derived, not measured; m = max(n, 16) is the inverter's block size, u the engine dtype's unit
roundoff, kappa = ||A||_inf ||inv(A)||_inf, asserted < 1e4 for the inputs):

  inverse   max |got - ref| <= m u kappa max|ref|, ref = ldexp(numpy inverse of the scaled matrix as the
            engine dtype holds it, e_b): the first-order forward bound of tests/test_block_inverse_edges.py;
            undoing the scaling is exact.
  solve     every column converged; the backward error recomputed in longdouble,
            eta = ||b - A x|| / (||A|| ||x|| + ||b||), is <= tol + gamma(n + 2): the rule stopped at tol on a
            residual computed in fp64, whose own rounding is gamma(n + 2) (|b| + |A| |x|).  The forward error
            against a longdouble solve is <= 2 kappa eta / (1 - kappa eta) (x solves a system perturbed by eta
            exactly); the reference is a longdouble elimination refined twice in longdouble.
  slogdet   sign equal to numpy's, |logabsdet - ref| <= n cond_inf 2^-52 (tests/test_slogdet_ops.py), and the
            bits of ops.slogdet_batch on the same blocks.
  rcond     relative error <= 4 m u kappa against 1 / (||A|| ||numpy inv||): the computed inverse's norm is
            off by at most m u kappa relatively (the inverse bound summed over a row), the margin covers the
            reference and the two norms' roundings.
"""
import functools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj

LD = np.longdouble
UNIT = {"fp64": 2.0 ** -53, "fp32": 2.0 ** -24}
_ND = {"fp64": np.float64, "fp32": np.float32}
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
INV_CASES = ([(n, nb, "fp64") for n in (1, 5, 15, 16, 37, 128, 129, 256, 257, 300) for nb in (1, 3)] +
             [(n, nb, "fp32") for n in (16, 128, 256, 257) for nb in (1, 3)] + [(16, 300, "fp64"), (16, 300, "fp32")])


def gamma(q, u=2.0 ** -53):
    return q * u / (1 - q * u)


@functools.lru_cache(maxsize=None)
def _stack(n, nb, seed=0):
    """well-conditioned random matrices, every member at its own scale"""
    rng = np.random.default_rng([61, n, nb, seed])
    A = rng.uniform(-1, 1, (nb, n, n)) + 2.0 * np.sqrt(n) * np.eye(n)
    A *= np.ldexp(1.0, (np.arange(nb) * 11) % 31 - 15)[:, None, None]
    A.setflags(write=False)
    return A


def _dev(a, device):
    """the stack as the input of a device: numpy on the host, a CUDA tensor on the GPU"""
    return a if device == "cpu" else torch.tensor(a, device="cuda")


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _rule(norm):
    e = np.zeros(norm.shape, dtype=np.int32)
    ok = np.isfinite(norm) & (norm > 0)
    e[ok] = 1 - np.frexp(norm[ok])[1]
    return e


def _kappa(A64, ref):
    k = np.abs(A64).sum(1).max() * np.abs(ref).sum(1).max()
    assert k < 1e4, k  # the inputs are meant to be well conditioned
    return k


# ------------------------------------------------------------------ inverse
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", INV_CASES, ids=lambda c: "n%d-nb%d-%s" % c)
def test_inverse(case, device):
    n, nb, dt = case
    A = _stack(n, nb)
    F = gj.batched.factor(_dev(A, device), dtype=dt)
    got = _np(F.inverse())
    assert got.shape == A.shape and got.dtype == np.float64 and F.valid.all() and F.valid.shape == (nb,)
    assert (F.n, F.nb, F.dtype) == (n, nb, dt)
    m = max(n, 16)
    for b in range(nb):
        e = int(F.exponents[b])
        As = np.ldexp(A[b], e).astype(_ND[dt]).astype(np.float64)  # what the inverter saw
        refs = np.linalg.inv(As)
        kappa = _kappa(As, refs)
        ref = np.ldexp(refs, e)
        err, bound = np.abs(got[b] - ref).max(), m * UNIT[dt] * kappa * np.abs(ref).max()
        assert err <= bound, (b, err, bound)


# ------------------------------------------------------------------ mixed scales
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dt,n", [("fp64", 37), ("fp64", 130), ("fp32", 37)])
def test_mixed_scales_are_exact(dt, n, device):
    shifts = [-600, -70, 0, 70, 600] if dt == "fp64" else [-70, 0, 70]
    base = _stack(n, 1)[0] * np.ldexp(1.0, 15)  # (undo _stack's own scale of member 0)
    if dt == "fp32":
        base = base.astype(np.float32).astype(np.float64)
    A = np.stack([np.ldexp(base, s) for s in shifts])
    F = gj.batched.factor(_dev(A, device), dtype=dt)
    inv = _np(F.inverse())
    assert F.valid.all()
    assert np.array_equal(F.exponents, _rule(np.abs(A).sum(2).max(1)))
    z = shifts.index(0)
    for i, s in enumerate(shifts):
        assert np.array_equal(inv[i], np.ldexp(inv[z], -s)), s


# ------------------------------------------------------------------ singular and NaN members
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_bad_members_do_not_touch_the_others(dt, device):
    n = 37
    good = _stack(n, 3)
    A = np.stack([good[0], good[1].copy(), good[1], good[2].copy(), good[2]])
    A[1, 5, :] = 0.0      # a zero row
    A[3, 7, 9] = np.nan
    F = gj.batched.factor(_dev(A, device), dtype=dt, check=False)
    assert F.valid.tolist() == [True, False, True, False, True]
    inv = _np(F.inverse())
    assert np.isnan(inv[[1, 3]]).all()
    ref = _np(gj.batched.factor(_dev(good, device), dtype=dt).inverse())
    assert np.array_equal(inv[[0, 2, 4]], ref)
    B = np.random.default_rng(5).uniform(-1, 1, (5, n, 3))
    X = _np(F.solve(_dev(B, device)))
    assert np.isnan(X[[1, 3]]).all() and np.isfinite(X[[0, 2, 4]]).all()
    assert not F.infos["converged"][[1, 3]].any() and F.infos["converged"][[0, 2, 4]].all()
    Xg = _np(gj.batched.factor(_dev(good, device), dtype=dt).solve(_dev(B[[0, 2, 4]], device)))
    assert np.array_equal(X[[0, 2, 4]], Xg)
    assert F.rcond()[1] == 0.0 and F.rcond()[3] == 0.0
    with pytest.raises(gj.SingularMatrixError) as ei:
        gj.batched.factor(_dev(A, device), dtype=dt)
    assert "[1, 3]" in str(ei.value)


# ------------------------------------------------------------------ chunking
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n,dt", [(16, "fp64"), (37, "fp32"), (130, "fp64")])
def test_chunks_give_the_same_bits(n, dt, device):
    nb, m, es = 7, max(n, 16), 8 if dt == "fp64" else 4
    A = _dev(_stack(n, nb), device)
    whole = gj.batched.factor(A, dtype=dt)
    assert whole.chunk == nb
    # the workspace is grown one matrix's panel and inverses at a time until a chunk holds three matrices
    # (what the inverter's scratch takes of it is the device's business): chunks of 3, 3 and 1
    parts = None
    for j in range(3, 40):
        parts = gj.batched.factor(A, dtype=dt, workspace_bytes=j * 2 * m * m * es)
        if parts.chunk >= 3:
            break
    assert parts.chunk == 3, parts.chunk  # at least three chunks, the last one ragged
    assert np.array_equal(_np(parts.inverse()), _np(whole.inverse()))
    assert np.array_equal(parts.exponents, whole.exponents) and parts.valid.all()
    assert np.array_equal(parts.rcond(), whole.rcond())


# ------------------------------------------------------------------ solve
def _solve_ld(A, B):
    """Gaussian elimination with partial pivoting in longdouble, and two steps of refinement"""
    n = A.shape[0]
    Al, Bl = A.astype(LD), B.astype(LD)

    def ge(rhs):
        M = np.concatenate([Al, rhs], axis=1)
        for c in range(n):
            p = c + int(np.argmax(np.abs(M[c:, c])))
            if p != c:
                M[[c, p]] = M[[p, c]]
            M[c + 1:] -= np.outer(M[c + 1:, c] / M[c, c], M[c])
        x = np.zeros((n, rhs.shape[1]), dtype=LD)
        for c in range(n - 1, -1, -1):
            x[c] = (M[c, n:] - M[c, c + 1:n] @ x[c + 1:]) / M[c, c]
        return x

    x = ge(Bl)
    for _ in range(2):
        x = x + ge(Bl - Al @ x)
    return x


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("n,k", [(5, 1), (16, 3), (37, 70), (130, 3), (130, 70)])
def test_solve_is_refined(n, k, dt, device):
    nb, tol = 3, 1e-15
    A = _stack(n, nb)
    B = np.random.default_rng([67, n, k]).uniform(-1, 1, (nb, n, k))
    F = gj.batched.factor(_dev(A, device), dtype=dt)
    X = _np(F.solve(_dev(B, device), tol=tol))
    assert X.shape == B.shape and X.dtype == np.float64
    inf = F.infos
    assert all(inf[key].shape == (nb, k) for key in ("converged", "steps", "residual", "backward_error"))
    assert inf["converged"].all()
    for b in range(nb):
        Al, xl, bl = A[b].astype(LD), X[b].astype(LD), B[b].astype(LD)
        an = np.abs(Al).sum(1).max()
        eta = np.abs(bl - Al @ xl).max(0) / (an * np.abs(xl).max(0) + np.abs(bl).max(0))
        assert (eta <= tol + gamma(n + 2)).all(), (b, float(eta.max()))
        kappa = float(an * np.abs(np.linalg.inv(A[b])).sum(1).max())
        assert kappa < 1e4
        xt = _solve_ld(A[b], B[b])
        ferr = np.abs(xl - xt).max(0) / np.abs(xt).max(0)
        bound = 2 * kappa * eta / (1 - kappa * eta)
        assert (ferr <= bound).all(), (b, float((ferr / bound).max()))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_vector_rhs_and_neighbours_of_frozen_and_nan_columns(dt, device):
    n, nb = 37, 3
    A = _stack(n, nb)
    B = np.random.default_rng(71).uniform(-1, 1, (nb, n, 5))
    F = gj.batched.factor(_dev(A, device), dtype=dt)
    X = _np(F.solve(_dev(B, device)))
    x0 = _np(F.solve(_dev(B[:, :, 0].copy(), device)))
    assert x0.shape == (nb, n) and F.infos["converged"].shape == (nb, 1)
    assert np.array_equal(x0, X[:, :, 0])
    B2 = B.copy()
    B2[:, :, 1] = 0.0          # frozen: x = 0 converges at once
    B2[1, 3, 3] = np.nan       # a NaN column of one matrix
    X2 = _np(F.solve(_dev(B2, device)))
    assert np.array_equal(X2[:, :, [0, 2, 4]], X[:, :, [0, 2, 4]])
    assert (X2[:, :, 1] == 0).all() and F.infos["converged"][:, 1].all()
    assert np.isnan(X2[1, :, 3]).all() and not F.infos["converged"][1, 3]
    assert np.array_equal(X2[[0, 2], :, 3], X[[0, 2], :, 3])


# ------------------------------------------------------------------ slogdet, rcond
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", [1, 5, 37, 130])
def test_slogdet(n, device):
    from mpi_jordan_crazy_acceleration_amd import ops
    nb = 3
    A = _stack(n, nb).copy()
    A[1] = -A[1, ::-1] if n > 1 else -A[1]  # another sign
    rs, rl = np.linalg.slogdet(A)
    tol = np.array([n * np.linalg.cond(A[b], np.inf) * 2.0 ** -52 for b in range(nb)])
    for s, l in (gj.batched.slogdet(_dev(A, device)), gj.batched.factor(_dev(A, device)).slogdet()):
        assert s.dtype == l.dtype == np.float64 and s.shape == (nb,)
        assert np.array_equal(s, rs) and (np.abs(l - rl) <= tol).all()
        t = torch.from_numpy(A).to(device)
        os_, ol = ops.slogdet_batch(t)
        assert np.array_equal(s, os_.cpu().numpy()) and np.array_equal(l, ol.cpu().numpy())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n,dt", [(5, "fp64"), (37, "fp64"), (130, "fp64"), (37, "fp32"), (130, "fp32")])
def test_rcond(n, dt, device):
    A = _stack(n, 3)
    F = gj.batched.factor(_dev(A, device), dtype=dt)
    got = F.rcond()
    m = max(n, 16)
    for b in range(3):
        ref_inv = np.linalg.inv(A[b])
        kappa = _kappa(A[b], ref_inv)
        assert abs(got[b] * kappa - 1.0) <= 4 * m * UNIT[dt] * kappa, (b, got[b] * kappa)


# ------------------------------------------------------------------ interface
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_leading_shapes_views_and_containers(dt):
    n = 17
    base = _stack(n, 6)
    A = base.reshape(2, 3, n, n)
    ref = np.linalg.inv(A)
    tol = 16 * n * UNIT[dt] * 1e2 * np.abs(ref).max(axis=(-1, -2), keepdims=True)
    F = gj.batched.factor(A, dtype=dt)
    inv = F.inverse()
    assert isinstance(inv, np.ndarray) and inv.shape == (2, 3, n, n) and inv.dtype == np.float64
    assert F.valid.shape == F.exponents.shape == F.rcond().shape == (2, 3) and F.nb == 6
    assert (np.abs(inv - ref) <= tol).all()
    # non-contiguous views: a transposed stack and a strided slice of a wider array
    At = np.ascontiguousarray(A.transpose(0, 1, 3, 2)).transpose(0, 1, 3, 2)
    assert not At.flags.c_contiguous and np.array_equal(gj.batched.inverse(At, dtype=dt), inv)
    wide = np.full((2, 3, n + 3, 2 * n + 1), np.nan)
    wide[:, :, 2:2 + n, 1:1 + 2 * n:2] = A
    assert np.array_equal(gj.batched.inverse(wide[:, :, 2:2 + n, 1:1 + 2 * n:2], dtype=dt), inv)
    # a CPU tensor comes back as a CPU tensor, float32 as float32
    t = torch.from_numpy(A.copy())
    it = gj.batched.inverse(t, dtype=dt)
    assert isinstance(it, torch.Tensor) and not it.is_cuda and it.dtype == torch.float64
    assert np.array_equal(it.numpy(), inv)
    i32 = gj.batched.inverse(A.astype(np.float32), dtype=dt)
    assert i32.dtype == np.float32 and i32.shape == A.shape
    B = np.random.default_rng(3).uniform(-1, 1, (2, 3, n, 4))
    X = gj.batched.solve(A, B, dtype=dt)
    assert X.shape == B.shape and np.abs(A @ X - B).max() <= 1e-13 * np.abs(A).max()
    xv = gj.batched.solve(t, torch.from_numpy(B[..., 0].copy()), dtype=dt)
    assert isinstance(xv, torch.Tensor) and xv.shape == (2, 3, n) and np.array_equal(xv.numpy(), X[..., 0])
    # A^T X = B for a stack
    Xt = gj.batched.solve(A.transpose(0, 1, 3, 2), B, dtype=dt)
    assert np.abs(A.transpose(0, 1, 3, 2) @ Xt - B).max() <= 1e-13 * np.abs(A).max()
    s, l = gj.batched.slogdet(A)
    assert s.shape == l.shape == (2, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_cuda_in_cuda_out(dt):
    n = 37
    A = torch.from_numpy(_stack(n, 6).reshape(2, 3, n, n).copy()).cuda()
    F = gj.batched.factor(A, dtype=dt)
    inv = F.inverse()
    assert inv.is_cuda and inv.device == A.device and inv.dtype == A.dtype and inv.shape == A.shape
    host = gj.batched.inverse(A.cpu().numpy(), dtype=dt)
    assert np.abs(inv.cpu().numpy() - host).max() <= 64 * UNIT[dt] * 1e2 * np.abs(host).max()
    B = torch.rand((2, 3, n, 5), dtype=torch.float64, device="cuda")
    X = F.solve(B)
    assert X.is_cuda and X.shape == B.shape and F.infos["converged"].all()
    At = A.transpose(-1, -2)  # a non-contiguous CUDA view
    assert torch.equal(gj.batched.inverse(At, dtype=dt), gj.batched.inverse(At.contiguous(), dtype=dt))
    a32 = gj.batched.inverse(A.float(), dtype=dt)
    assert a32.is_cuda and a32.dtype == torch.float32


def test_refusals():
    with pytest.raises(ValueError, match="gj.factor"):
        gj.batched.factor(np.zeros((2, 1025, 1025)))
    with pytest.raises(ValueError):
        gj.batched.factor(np.zeros((2, 4, 5)))
    with pytest.raises(ValueError):
        gj.batched.factor(np.zeros(4))
    with pytest.raises(ValueError):
        gj.batched.factor(np.eye(4)[None]).solve(np.zeros((1, 5)))
    # the single-matrix entry point still refuses a stack, exactly as before
    with pytest.raises(ValueError, match="A must be square"):
        gj.inverse(np.stack([np.eye(4)] * 2))
    assert gj.batched.factor(np.eye(1024)[None] * 3.0).valid.all()


# ------------------------------------------------------------------ schedule checker
@pytest.mark.parametrize("asynchronous", [False, True])
def test_factor_and_solve_under_the_schedule_checker(asynchronous):
    from mpi_jordan_crazy_acceleration_amd.batched import BatchFactored
    native = gj.load_native()
    n, nb = 37, 7
    A = _stack(n, nb)
    B = np.random.default_rng(9).uniform(-1, 1, (nb, n, 70))
    dev, hb = native.race_check_host_device(asynchronous, 1)
    F = BatchFactored(A, dtype="fp32", workspace_bytes=3 * 3 * 37 * 37 * 4, _device=dev)
    X = F.solve(B)
    assert hb.ops() > 0 and hb.races() == 0, hb.reports()
    ref = gj.batched.factor(A, dtype="fp32", workspace_bytes=3 * 3 * 37 * 37 * 4)
    assert np.array_equal(X, ref.solve(B)) and np.array_equal(F.inverse(), ref.inverse())
