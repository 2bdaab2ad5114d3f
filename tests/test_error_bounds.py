"""Error bounds of the refined solves and the condition number from the resident inverse:
Engine::solve_rhs_block with bounds (RhsResult::ferr / berr) and Engine::cond, through gj.factor(A),
gj.solve, GaussJordan.run, DistributedGaussJordan and both CLIs.

For the returned iterate x of a column, with r = b - A x in fp64, D = |A| |x| + |b| and u = 2^-53,
    berr = max_i |r_i| / D_i
    ferr = max_i (|inv(A)| (|r| + (n + 1) u D))_i / ||x||_inf
(LAPACK's xGERFS with the resident |inv(A)| in place of its norm estimate; A^T and inv(A)^T with trans).

Validity.  A = round(2^20 (U(-1, 1) + sqrt(n) I)) / 2^20, x_true integer in [-8, 8]: B = A x_true is
exact in fp64 (25 + 4 + 9 bits), so x_true is the exact solution and ||x - x_true|| / ||x|| <= ferr is
checked as it stands.  (With numpy's LU and dgesvx at n = 96, k = 3: true error 2-3e-16, dgesvx ferr
2.9e-13 .. 3.5e-13, this formula 3.5e-13 .. 3.8e-13, berr 6e-17 .. 8e-17.)

Tightness.  With Xi = F.inverse() as stored, r_ld = B - A x and D in longdouble, the fp64 residual
the engine used is within gamma(n + 1) D of r_ld, so
    lower = || |Xi| (max(|r_ld| - gamma(n+1) D, 0) + (n+1) u D) || / ||x|| (1 - gamma(2n))
    upper = || |Xi| (|r_ld| + gamma(n+1) D + (n+1) u D) || / ||x|| (1 + gamma(2n))
bracket ferr (gamma(2n) covers the fp64 products |A||x| and |Xi| G, the sum and the division), and
|berr - max_i |r_ld|_i / D_i| <= 2 gamma(n + 1).  Derived from the residual's own error bound, not
measured.

Sizes: n in {96, 301} with m in {16, 59}; k in {1, 3, 70} (70: two column groups); both dtypes, plain
and transposed; on the CPU executors and, marked gpu, on CUDA tensors.
"""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = LD(2) ** -53
SIZES = [(96, 16), (301, 59)]
KS = [1, 3, 70]


def gamma(q):
    return q * U / (1 - q * U)


@functools.lru_cache(maxsize=None)
def _system(n):
    """A, x_true (n x 70) with A x_true and A^T x_true exact in fp64"""
    rng = np.random.default_rng([53, n])
    A = np.round(2.0 ** 20 * (rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n))) / 2.0 ** 20
    xt = rng.integers(-8, 9, (n, 70)).astype(np.float64)
    xt[0, :] = 8.0  # no zero column
    for t in (A, xt):
        t.setflags(write=False)
    return A, xt


@functools.lru_cache(maxsize=None)
def _factored(n, m, dt, device):
    A = _system(n)[0]
    return gj.factor(A if device == "cpu" else torch.from_numpy(A.copy()).to(device), block_size=m, dtype=dt)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _check_bounds(A, B, x, infos, Xi, trans, x_true=None, what=""):
    """validity against x_true (when given) and the longdouble bracket of ferr / berr, column by column"""
    n = A.shape[0]
    Aop, Xop = (A.T, Xi.T) if trans else (A, Xi)
    B2, x2 = B.reshape(n, -1), x.reshape(n, -1)
    assert len(infos) == B2.shape[1]
    Al, xl, Bl = Aop.astype(LD), x2.astype(LD), B2.astype(LD)
    r = np.abs(Bl - Al @ xl)
    D = np.abs(Al) @ np.abs(xl) + np.abs(Bl)
    g1, nu = gamma(LD(n + 1)), LD(n + 1) * U
    aX = np.abs(Xop).astype(LD)
    xn = np.abs(xl).max(axis=0)
    lower = (aX @ (np.maximum(r - g1 * D, 0) + nu * D)).max(axis=0) / xn * (1 - gamma(LD(2 * n)))
    upper = (aX @ (r + g1 * D + nu * D)).max(axis=0) / xn * (1 + gamma(LD(2 * n)))
    berr_ld = (r / D).max(axis=0)
    for j, info in enumerate(infos):
        ferr, berr = info["ferr"], info["berr"]
        print(f"{what} col {j}: ferr {ferr:.3e} in [{float(lower[j]):.3e}, {float(upper[j]):.3e}] berr {berr:.3e} "
              f"(ld {float(berr_ld[j]):.3e}) converged {info['converged']}")
        assert lower[j] <= ferr <= upper[j], (j, float(lower[j]), ferr, float(upper[j]))
        assert abs(LD(berr) - berr_ld[j]) <= 2 * g1, (j, berr, float(berr_ld[j]))
        if x_true is not None:
            err = float(np.abs(x2[:, j] - x_true[:, j]).max() / np.abs(x2[:, j]).max())
            print(f"{what} col {j}: true error {err:.3e}")
            assert info["converged"] and err <= ferr, (j, err, ferr)


def _exact_case(device, n, m, dt, trans, k):
    A, xt = _system(n)
    F = _factored(n, m, dt, device)
    B = (A.T if trans else A) @ xt[:, :k]
    b = B[:, 0] if k == 1 else B  # one right-hand side: a vector, the block path as one column
    bb = b if device == "cpu" else torch.from_numpy(b).to(device)
    x = _np(F.solve(bb, trans=trans, bounds=True))
    assert x.shape == b.shape and len(F.infos) == k
    _check_bounds(A, B, x, F.infos, _np(F.inverse()).astype(np.float64), trans, x_true=xt[:, :k],
                  what=f"n{n} {dt} {'trans' if trans else 'plain'}")


_CASES = [(n, m, dt, trans, k) for n, m in SIZES for dt in ("fp64", "fp32") for trans in (False, True) for k in KS]


def _id(c):
    return f"n{c[0]}m{c[1]}-{c[2]}-{'trans' if c[3] else 'plain'}-k{c[4]}"


@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_exact_solution_host(case):
    _exact_case("cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_exact_solution_gpu(case):
    native = gj.load_native()
    _exact_case("cuda", *case)
    n, m, dt, trans, k = case
    kw = 16 if min(k, 64) <= 16 else 32 if min(k, 64) <= 32 else 64
    if k == 70:  # the last group has 6 columns, at the call's leading dimension
        kw = 16
    name = native.last_abs_kernel()
    assert name.startswith(f"{'abst' if trans else 'abs'}{kw}:{'f64' if dt == 'fp64' else 'f32'}:"), name


# ------------------------------------------------------------------ the option changes nothing else
def _option_off_case(device):
    n, m = 96, 16
    A, xt = _system(n)
    rng = np.random.default_rng(3)
    B = rng.standard_normal((n, 5))
    Bd = B if device == "cpu" else torch.from_numpy(B).to(device)
    for dt in ("fp64", "fp32"):
        F = _factored(n, m, dt, device)
        for trans in (False, True):
            x0 = _np(F.solve(Bd, trans=trans))
            off = [dict(i) for i in F.infos]
            assert all("ferr" not in i and "berr" not in i for i in off)
            x1 = _np(F.solve(Bd, trans=trans, bounds=True))
            assert np.array_equal(x0.view(np.int64), x1.view(np.int64))  # bit for bit
            on = [dict(i) for i in F.infos]
            assert [{k: v for k, v in i.items() if k not in ("ferr", "berr")} for i in on] == off
            assert all(np.isfinite(i["ferr"]) and np.isfinite(i["berr"]) for i in on)


def test_option_off_host():
    _option_off_case("cpu")


@pytest.mark.gpu
def test_option_off_gpu():
    _option_off_case("cuda")


def _special_columns(device):
    n, m = 96, 16
    A, xt = _system(n)
    F = _factored(n, m, "fp64", device)
    for trans in (False, True):
        Aop = A.T if trans else A
        # a zero column of b: x = 0, the numerator of ferr is returned undivided (LAPACK's rule)
        B = Aop @ xt[:, :3]
        B[:, 1] = 0.0
        x = _np(F.solve(B if device == "cpu" else torch.from_numpy(B).to(device), trans=trans, bounds=True))
        assert (x[:, 1] == 0).all()
        z = F.infos[1]
        assert np.isfinite(z["ferr"]) and 0 <= z["ferr"] < 1e-290 and z["berr"] == 1.0  # (0 + safe1) / (0 + safe1)
        keep = [0, 2]
        _check_bounds(A, B[:, keep], x[:, keep], [F.infos[j] for j in keep], _np(F.inverse()), trans,
                      x_true=xt[:, keep])
        # a NaN in b: NaN bounds for that column only
        B = Aop @ xt[:, :3]
        B[5, 2] = np.nan
        x = _np(F.solve(B if device == "cpu" else torch.from_numpy(B).to(device), trans=trans, bounds=True))
        assert np.isnan(F.infos[2]["ferr"]) and np.isnan(F.infos[2]["berr"])
        _check_bounds(A, B[:, :2], x[:, :2], F.infos[:2], _np(F.inverse()), trans, x_true=xt[:, :2])


def test_zero_and_nan_columns_host():
    _special_columns("cpu")


@pytest.mark.gpu
def test_zero_and_nan_columns_gpu():
    _special_columns("cuda")


# ------------------------------------------------------------------ an ill-conditioned system
def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble"""
    n = A.shape[0]
    M = np.concatenate([A.astype(LD), b.astype(LD).reshape(n, -1)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c + 1:] -= np.outer(M[c + 1:, c] / M[c, c], M[c])
    x = np.zeros((n, M.shape[1] - n), dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (M[i, n:] - M[i, i + 1:n] @ x[i + 1:]) / M[i, i]
    return x


def _hilbert(device):
    n, m = 10, 16
    i = np.arange(n)
    A = 1.0 / (i[:, None] + i[None, :] + 1.0)
    b = A @ np.ones(n)
    F = gj.factor(A if device == "cpu" else torch.from_numpy(A).to(device), block_size=m)
    x = _np(F.solve(b if device == "cpu" else torch.from_numpy(b).to(device), bounds=True))
    xl = _solve_ld(A, b)[:, 0]
    err = float(np.abs(x.astype(LD) - xl).max() / np.abs(x).max())
    info = F.infos[0]
    print(f"hilbert n=10: error {err:.3e} ferr {info['ferr']:.3e} berr {info['berr']:.3e} "
          f"converged {info['converged']} cond_inf {F.cond():.3e}")
    assert np.isfinite(info["ferr"]) and info["ferr"] >= err


def test_hilbert_host():
    _hilbert("cpu")


@pytest.mark.gpu
def test_hilbert_gpu():
    _hilbert("cuda")


# ------------------------------------------------------------------ more than one rank
def _run_ranks(n, m, dt, ranks, trans, **kw):
    A, xt = _system(n)
    B = (A.T if trans else A) @ xt[:, :3]
    g = gj.GaussJordan(block_size=m, ranks=ranks, device="cpu", dtype=dt, residual="never", host_threads=1, **kw)
    rep = g.run(n, input=A, rhs=B, keep_solution=True, keep_inverse=True, trans=trans, bounds=True, cond=True)
    assert rep["status"] == 0, rep["message"]
    return A, B, xt[:, :3], rep


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_three_loopback_ranks(dt):
    n, m = 301, 59
    for trans in (False, True):
        A, B, xt, one = _run_ranks(n, m, dt, 1, trans)
        _, _, _, three = _run_ranks(n, m, dt, 3, trans, comm="loopback")
        _check_bounds(A, B, three["x"], three["axb_columns"], three["inverse"], trans, x_true=xt, what=f"p=3 {dt}")
        if np.array_equal(one["x"], three["x"]) and np.array_equal(one["inverse"], three["inverse"]):
            # the same iterate from the same inverse: the bounds differ by the order of the sums alone
            for a, b in zip(one["axb_columns"], three["axb_columns"]):
                for key in ("ferr", "berr"):
                    assert abs(LD(a[key]) - LD(b[key])) <= gamma(LD(n + 2)) * LD(a[key]), (key, a[key], b[key])
        for key, p in (("one", 1), ("inf", np.inf)):  # each against its own inverse (fp32: they differ)
            for rep in (one, three):
                want = np.linalg.norm(A, p) * np.linalg.norm(rep["inverse"], p)
                assert abs(rep["cond"][key] - want) <= n * 2.0 ** -53 * want


def _assert_equal_bounds(one, many, n):
    for j, (a, b) in enumerate(zip(one, many)):
        for key in ("ferr", "berr"):
            rel = float(abs(LD(a[key]) - LD(b[key])) / LD(a[key]))
            print(f"col {j} {key}: one rank {a[key]:.6e}, ranks {b[key]:.6e}, relative difference {rel:.3e}")
    for a, b in zip(one, many):
        for key in ("ferr", "berr"):
            assert abs(LD(a[key]) - LD(b[key])) <= gamma(LD(n + 2)) * LD(a[key]), (key, a[key], b[key])


# The look-ahead depth 0 means "chosen by the engine", and the engine chooses differently at p = 1 and at
# p > 1: the two sweeps then round differently and their inverses differ in the last bits, at the same
# pivots (so before the bounds existed).  A comparison between rank counts fixes the depth on both
# sides; the inverses are then bit-equal.
_DEPTH = 1


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("n,m", SIZES)
def test_three_loopback_ranks_equal_one_rank_bounds(n, m, dt):
    """The bounds of 3 loopback ranks equal the 1-rank bounds within gamma(n + 2), relatively, for
    A X = B at one look-ahead depth.

    The ranks then hold rows of the same inverse and every row's sums run in the same order at any rank
    count, so the iterate and its residual are the same and the bounds differ by nothing but the
    grouping of the non-negative sums behind D and |inv(A)| G (gamma(n + 2) covers any order).  For
    A^T X = B the iterate itself is a sum over the ranks, differs in its last bits between rank counts,
    and r = b - A^T x -- rounding noise of x -- with it: there the bounds of each rank count are held to
    the longdouble bracket and the exact solution instead (test_three_loopback_ranks)."""
    A, B, xt, one = _run_ranks(n, m, dt, 1, False, depth=_DEPTH)
    _, _, _, three = _run_ranks(n, m, dt, 3, False, comm="loopback", depth=_DEPTH)
    assert np.array_equal(one["inverse"], three["inverse"]) and np.array_equal(one["x"], three["x"])
    _assert_equal_bounds(one["axb_columns"], three["axb_columns"], n)
    for key in ("one", "inf"):
        assert abs(one["cond"][key] - three["cond"][key]) <= float(gamma(LD(n + 2))) * one["cond"][key]


def test_schedule_checker_reports_nothing():
    n, m = 96, 16
    for trans in (False, True):
        A, B, xt, ref = _run_ranks(n, m, "fp32", 3, trans, comm="loopback")
        _, _, _, rep = _run_ranks(n, m, "fp32", 3, trans, comm="async", jitter_us=30.0, race_check=True)
        assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
        assert np.array_equal(rep["x"], ref["x"])
        assert [(c["ferr"], c["berr"]) for c in rep["axb_columns"]] == [(c["ferr"], c["berr"])
                                                                         for c in ref["axb_columns"]]
        assert rep["cond"] == ref["cond"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, n, m, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from mpi_jordan_crazy_acceleration_amd.parallel import DistributedGaussJordan

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        A, xt = _system(n)
        d = DistributedGaussJordan(n, m, dtype="fp64", host_threads=1, depth=_DEPTH)
        d.load(A)
        st = d.solve()
        out = {}
        for trans in (False, True):
            X, infos = d.solve_rhs((A.T if trans else A) @ xt[:, :3], A_rows=A, trans=trans, bounds=True)
            out[trans] = (X, [dict(i) for i in infos])
        X0, infos0 = d.solve_rhs(A @ xt[:, :3], A_rows=A)
        kappa = (d.cond(1, A_rows=A), d.cond(np.inf, A_rows=A))
        q.put((rank, st["status"], out, [dict(i) for i in infos0], kappa, d.gather_inverse()))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _gloo_run(world, n, m):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, n, m, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_gloo_ranks():
    world, n, m = 3, 96, 16
    res = _gloo_run(world, n, m)
    A, xt = _system(n)
    Xi = next(r[5] for r in res if r[5] is not None)
    F = gj.factor(A, block_size=m, depth=_DEPTH)
    for rank, status, out, infos0, kappa, _ in res:
        assert status == 0
        assert all("ferr" not in i for i in infos0)
        assert out[False][1] == res[0][2][False][1] and out[True][1] == res[0][2][True][1]  # the same on every rank
        assert kappa == res[0][4]
        for trans in (False, True):
            X, infos = out[trans]
            _check_bounds(A, (A.T if trans else A) @ xt[:, :3], X, infos, Xi, trans, x_true=xt[:, :3], what="gloo")
        for p, kp in zip((1, np.inf), kappa):
            assert abs(kp - F.cond(p)) <= float(gamma(LD(n + 2))) * F.cond(p)


def test_gloo_ranks_equal_one_rank_bounds():
    """The bounds of 3 gloo ranks equal the 1-rank bounds within gamma(n + 2), relatively (A X = B at one
    look-ahead depth, as test_three_loopback_ranks_equal_one_rank_bounds)."""
    world, n, m = 3, 96, 16
    res = _gloo_run(world, n, m)
    A, xt = _system(n)
    F = gj.factor(A, block_size=m, depth=_DEPTH)
    x = F.solve(A @ xt[:, :3], bounds=True)
    assert np.array_equal(x, res[0][2][False][0])
    _assert_equal_bounds(F.infos, res[0][2][False][1], n)


# ------------------------------------------------------------------ after a low-rank update
def _update_case(device):
    n, m = 96, 16
    A, xt = _system(n)
    rng = np.random.default_rng(9)
    Uu = rng.integers(-2, 3, (n, 2)).astype(np.float64)
    Vv = rng.integers(-512, 513, (n, 2)) / 1024.0
    A2 = A + Uu @ Vv.T  # exact
    for dt in ("fp64", "fp32"):
        F = gj.factor(A if device == "cpu" else torch.from_numpy(A.copy()).to(device), block_size=m, dtype=dt)
        k0 = F.cond(1), F.cond(np.inf)
        F.update(Uu, Vv)
        Xi = _np(F.inverse()).astype(np.float64)
        for p, old in zip((1, np.inf), k0):
            want = np.linalg.norm(A2, p) * np.linalg.norm(Xi, p)
            assert abs(F.cond(p) - want) <= n * 2.0 ** -53 * want and F.cond(p) != old
        for trans in (False, True):
            B = (A2.T if trans else A2) @ xt[:, :3]
            x = _np(F.solve(B if device == "cpu" else torch.from_numpy(B).to(device), trans=trans, bounds=True))
            _check_bounds(A2, B, x, F.infos, Xi, trans, x_true=xt[:, :3], what=f"updated {dt}")


def test_after_update_host():
    _update_case("cpu")


@pytest.mark.gpu
def test_after_update_gpu():
    _update_case("cuda")


# ------------------------------------------------------------------ cond
def _cond_case(device, n, m, dt):
    A = _system(n)[0]
    F = _factored(n, m, dt, device)
    Xi = _np(F.inverse()).astype(np.float64)
    for p in (1, np.inf):
        got = F.cond(p)
        want = np.linalg.norm(A, p) * np.linalg.norm(Xi, p)
        assert abs(got - want) <= n * 2.0 ** -53 * want, (p, got, want)
        assert F.rcond(p) == 1.0 / got and F.cond(p) == got
        kappa = np.linalg.cond(A, p)
        assert kappa < 1e3
        # first order: the stored inverse is within about n kappa u of inv(A), relatively (u of the engine dtype)
        rtol = 1e-8 if dt == "fp64" else n * n * kappa * 2.0 ** -24
        assert n * n * kappa * 2.0 ** -53 < 1e-8
        assert abs(got - kappa) <= rtol * kappa, (p, got, kappa)
    assert F.cond() == F.cond(np.inf)
    with pytest.raises(ValueError):
        F.cond(2)
    with pytest.raises(ValueError):
        F.rcond("fro")


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("n,m", SIZES)
def test_cond_host(n, m, dt):
    _cond_case("cpu", n, m, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("n,m", SIZES)
def test_cond_gpu(n, m, dt):
    _cond_case("cuda", n, m, dt)


def test_cond_function():
    n, m = 96, 16
    A = _system(n)[0]
    for p in (1, np.inf):
        assert abs(gj.cond(A, p, block_size=m) - np.linalg.cond(A, p)) <= 1e-8 * np.linalg.cond(A, p)
    assert gj.cond(np.ones((8, 8)), 1, block_size=4) == float("inf")
    assert gj.cond(np.zeros((5, 5)), block_size=4) == float("inf")
    with pytest.raises(ValueError):
        gj.cond(A, 2, block_size=m)
    rep = gj.GaussJordan(block_size=m, device="cpu", residual="never").run(n, input=A, cond=True)
    assert abs(rep["cond"]["one"] - np.linalg.cond(A, 1)) <= 1e-8 * rep["cond"]["one"]
    assert abs(rep["cond"]["inf"] - np.linalg.cond(A, np.inf)) <= 1e-8 * rep["cond"]["inf"]
    assert "cond" not in gj.GaussJordan(block_size=m, device="cpu", residual="never").run(n, input=A)


def test_run_and_solve_accept_bounds():
    n, m = 96, 16
    A, xt = _system(n)
    B = A @ xt[:, :3]
    g = gj.GaussJordan(block_size=m, device="cpu", residual="never")
    on = g.run(n, input=A, rhs=B, keep_solution=True, keep_inverse=True, bounds=True)
    off = g.run(n, input=A, rhs=B, keep_solution=True)
    assert np.array_equal(on["x"], off["x"])
    assert all("ferr" not in c for c in off["axb_columns"])
    _check_bounds(A, B, on["x"], on["axb_columns"], on["inverse"], False, x_true=xt[:, :3], what="run")
    # one right-hand side: the block path as one column, and only then per-column infos
    one = g.run(n, input=A, rhs=B[:, 0], keep_solution=True, keep_inverse=True, bounds=True)
    assert "axb_columns" not in g.run(n, input=A, rhs=B[:, 0]) and len(one["axb_columns"]) == 1
    _check_bounds(A, B[:, :1], one["x"], one["axb_columns"], one["inverse"], False, x_true=xt[:, :1], what="run k=1")
    x = gj.solve(A, B, block_size=m, bounds=True)
    assert np.array_equal(x, gj.solve(A, B, block_size=m))


@pytest.mark.gpu
def test_run_gpu_ranks():
    """three ranks on one GPU (thread ranks, the loopback communicator): every rank's kernels and the sums
    over the ranks"""
    n, m = 301, 59
    A, xt = _system(n)
    for dt, trans in (("fp64", False), ("fp32", True)):
        B = (A.T if trans else A) @ xt[:, :3]
        g = gj.GaussJordan(block_size=m, ranks=3, device="gpu", dtype=dt, residual="never", comm="async")
        rep = g.run(n, input=A, rhs=B, keep_solution=True, keep_inverse=True, trans=trans, bounds=True, cond=True)
        assert rep["status"] == 0, rep["message"]
        _check_bounds(A, B, rep["x"], rep["axb_columns"], rep["inverse"], trans, x_true=xt[:, :3], what=f"gpu p=3 {dt}")
        want = np.linalg.norm(A, np.inf) * np.linalg.norm(rep["inverse"], np.inf)
        assert abs(rep["cond"]["inf"] - want) <= n * 2.0 ** -53 * want


# ------------------------------------------------------------------ the two CLIs
def _lines(out):
    return [l for l in out.splitlines() if not l.startswith("glob_time") and not l.startswith("[Gloo]")]


def _gj(gj_bin, *args):
    p = subprocess.run([gj_bin, "--device", "cpu", *map(str, args)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout, p.stderr


def _pycli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", MASTER_PORT=str(_free_port()), RANK="0",
               WORLD_SIZE="1", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "-m", "mpi_jordan_crazy_acceleration_amd.cli", "--device", "cpu",
                        *map(str, args)], cwd="/tmp", env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout, p.stderr


def _json(err):
    return json.loads([l for l in err.splitlines() if l.startswith("{")][-1])


def test_clis_agree(gj_bin):
    base = ["--gen", "random", "--seed", 3, "--json", 77, 15]
    flags = ["--cond", "--bounds", "--rhs", "random", "--nrhs", 3]
    out, err = _gj(gj_bin, *flags, *base)
    pout, perr = _pycli(*flags, *base)
    assert "\n".join(_lines(out)) == "\n".join(_lines(pout))  # byte for byte, the time aside
    ja, jb = _json(err), _json(perr)
    for key in ("axb_ferr_cols", "axb_berr_cols"):
        assert len(ja[key]) == 3 and np.allclose(ja[key], jb[key], rtol=1e-6, atol=0)  # (%.6e in build/gj)
    assert np.isclose(ja["cond"]["one"], jb["cond"]["one"], rtol=1e-14)
    assert np.isclose(ja["cond"]["inf"], jb["cond"]["inf"], rtol=1e-14)
    A = generate_matrix(77, "random", 3)
    assert abs(ja["cond"]["inf"] - np.linalg.cond(A, np.inf)) <= 1e-6 * ja["cond"]["inf"]


def test_cli_stdout_without_the_flags_is_unchanged(gj_bin):
    base = ["--gen", "random", "--seed", 3, "--json", 77, 15]
    rhs = ["--rhs", "random", "--nrhs", 3]
    plain, plain_err = _gj(gj_bin, *rhs, *base)
    with_bounds, bounds_err = _gj(gj_bin, "--bounds", *rhs, *base)
    assert _lines(plain) == _lines(with_bounds)  # --bounds leaves stdout alone
    jp, jb = _json(plain_err), _json(bounds_err)
    assert {k for k in jb if k not in jp} == {"axb_ferr_cols", "axb_berr_cols"}
    assert all(jb[k] == jp[k] for k in jp if "seconds" not in k and "time" not in k and k != "gflops_nominal"
               and k != "host_wait_ms")
    # --cond: one more line, after the residual line and after the slogdet line
    both, both_err = _gj(gj_bin, "--cond", "--det", *rhs, *base)
    det_only, _ = _gj(gj_bin, "--det", *rhs, *base)
    a, b = _lines(det_only), _lines(both)
    extra = [l for l in b if l.startswith("cond: ")]
    assert len(extra) == 1 and [l for l in b if l is not extra[0]] == a
    assert b[b.index(extra[0]) - 1].startswith("slogdet: ") and b[b.index(extra[0]) - 2].startswith("residual: ")
    c, _ = _gj(gj_bin, "--cond", *base)
    cl = _lines(c)
    i = [j for j, l in enumerate(cl) if l.startswith("cond: ")]
    assert len(i) == 1 and cl[i[0] - 1].startswith("residual: ") and i[0] == len(cl) - 1
    tag, k1, kinf = cl[i[0]].split()
    jd = _json(both_err)["cond"]
    assert f"{jd['one']:e}" == k1 and f"{jd['inf']:e}" == kinf
    # the module CLI without the flags prints what it printed before them
    p0, _ = _pycli(*base)
    g0, _ = _gj(gj_bin, *base)
    assert _lines(p0) == _lines(g0) and not any(l.startswith(("cond", "solution")) for l in _lines(p0))
