"""gj.autograd: differentiable solve, slogdet and inverse from one inversion.

Inputs.  A = uniform(-1, 1) + sqrt(n) I from default_rng([5, n]): kappa_inf is about 27 at n = 12, 103 at
n = 200 and 71 at n = 130; every test asserts kappa_inf <= 200 as a condition on its input.

gradcheck (CPU, fp64 engine) with torch's default tolerances, at n = 12 with block_size 5 (npad 15) and
n = 8 with block_size 8.

Comparisons with a closed form (numpy, from numpy.linalg.solve / inv in fp64 on the CPU), elementwise:
    |got - ref| <= 32 n kappa_inf(A) u max|ref|
with u = 2^-53 for everything from an fp64 engine and for the solve gradients of an fp32 engine (Y and X
are refined against the fp64 rows), and u = 2^-24 for the slogdet and inverse gradients of an fp32 engine
(and for a loss that contains one).  This is the first-order forward-error bound of a backward-stable
inverse with the usual n-slack: a derived ceiling, not a measurement.  A wrong transposition or sign
misses it by ten orders.  Closed forms, Gbar the upstream gradient:
    X = A^-1 B:   Abar = -(A^-T Gbar) X^T, Bbar = A^-T Gbar      X = A^-T B:  Abar = -X (A^-1 Gbar)^T, Bbar = A^-1 Gbar
    log|det A|:   Abar = lbar A^-T                               X = A^-1:    Abar = -X^T Gbar X^T
"""
import functools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.models import gauss_jordan as gjm

U64, U32 = 2.0 ** -53, 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _problem(n, k):
    """A, B (n x k), the upstream gradients of a solve and of the inverse, y; kappa_inf(A)"""
    rng = np.random.default_rng([5, n])
    A = rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n)
    B = rng.uniform(-1, 1, (n, k))
    GX = rng.uniform(-1, 1, (n, k))
    GI = rng.uniform(-1, 1, (n, n))
    y = rng.uniform(-1, 1, n)
    kappa = np.abs(A).sum(1).max() * np.abs(np.linalg.inv(A)).sum(1).max()
    assert kappa <= 200, kappa
    for a in (A, B, GX, GI, y):
        a.setflags(write=False)
    return A, B, GX, GI, y, float(kappa)


@functools.lru_cache(maxsize=None)
def _closed_forms(n, k):
    A, B, GX, GI, y, _ = _problem(n, k)
    Ai = np.linalg.inv(A)
    out = {}
    X, Y = np.linalg.solve(A, B), np.linalg.solve(A.T, GX)
    out["solve"] = (-Y @ X.T, Y)
    Xt, Yt = np.linalg.solve(A.T, B), np.linalg.solve(A, GX)
    out["solve_t"] = (-Xt @ Yt.T, Yt)
    out["slogdet"] = 1.75 * Ai.T
    out["inverse"] = -Ai.T @ GI @ Ai.T
    out["loss"] = 0.5 * Ai.T - 0.5 * np.outer(np.linalg.solve(A.T, y), np.linalg.solve(A, y))
    return out


def _close(got, ref, n, kappa, u, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    bound = 32 * n * kappa * u * np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{what}: n={n} max err {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref.shape
    assert err <= bound, (what, err, bound)


def _t(a, device="cpu", dtype=torch.float64, grad=False):
    return torch.from_numpy(np.array(a)).to(device=device, dtype=dtype).requires_grad_(grad)


def _compare_all(n, m, k, device, engine_dtype):
    """every gradient of the module against its closed form, through one DiffFactored"""
    A, B, GX, GI, y, kappa = _problem(n, k)
    cf = _closed_forms(n, k)
    u_solve = U64
    u_inv = U64 if engine_dtype == "fp64" else U32
    At = _t(A, device, grad=True)
    F = gj.autograd.factor(At, block_size=m, dtype=engine_dtype)

    def grads(out, gout, *inputs):
        gs = torch.autograd.grad(out, inputs, gout)
        for g, t in zip(gs, inputs):
            assert g.device == t.device and g.dtype == t.dtype and g.shape == t.shape
        return gs

    for trans, key in ((False, "solve"), (True, "solve_t")):
        Bt = _t(B, device, grad=True)
        X = F.solve(Bt, trans=trans)
        assert X.device == Bt.device and X.dtype == Bt.dtype
        gA, gB = grads(X, _t(GX, device), At, Bt)
        _close(gA, cf[key][0], n, kappa, u_solve, f"{key} dA {engine_dtype}")
        _close(gB, cf[key][1], n, kappa, u_solve, f"{key} dB {engine_dtype}")
    s, l = F.slogdet()
    assert s.ndim == 0 and l.ndim == 0 and s.dtype == l.dtype == torch.float64 and l.device == At.device
    assert not s.requires_grad and l.requires_grad
    sn, ln = np.linalg.slogdet(A)
    assert float(s.detach()) == sn and abs(float(l.detach()) - ln) <= 32 * n * kappa * u_inv * max(1.0, abs(ln))
    (gA,) = grads(l, torch.tensor(1.75, dtype=torch.float64, device=device), At)
    _close(gA, cf["slogdet"], n, kappa, u_inv, f"slogdet dA {engine_dtype}")
    (gA,) = grads(F.inverse(), _t(GI, device), At)
    _close(gA, cf["inverse"], n, kappa, u_inv, f"inverse dA {engine_dtype}")
    # one graph: the Gaussian log-likelihood
    yt = _t(y, device)
    loss = 0.5 * (yt @ F.solve(yt)) + 0.5 * F.slogdet()[1]
    (gA,) = grads(loss, None, At)
    _close(gA, cf["loss"], n, kappa, u_inv, f"loss dA {engine_dtype}")


# ---------------------------------------------------------------- CPU, fp64 engine: gradcheck
_GC = [(12, 5), (8, 8)]


@pytest.mark.parametrize("n,m", _GC)
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("k", [0, 3])
def test_gradcheck_solve(n, m, trans, k):
    A, B, *_ = _problem(n, 3)
    At = _t(A, grad=True)
    Bt = _t(B[:, 0] if k == 0 else B, grad=True)  # k = 0: a vector b
    assert torch.autograd.gradcheck(lambda a, b: gj.autograd.solve(a, b, block_size=m, trans=trans), (At, Bt))


@pytest.mark.parametrize("n,m", _GC)
def test_gradcheck_slogdet(n, m):
    At = _t(_problem(n, 3)[0], grad=True)
    assert torch.autograd.gradcheck(lambda a: gj.autograd.slogdet(a, block_size=m)[1], (At,))


@pytest.mark.parametrize("n,m", _GC)
def test_gradcheck_inverse(n, m):
    At = _t(_problem(n, 3)[0], grad=True)
    assert torch.autograd.gradcheck(lambda a: gj.autograd.inverse(a, block_size=m), (At,))


# ---------------------------------------------------------------- CPU: closed forms
def test_wide_rhs_two_pieces():
    """70 columns: the backward's two pieces of 64 and 6 columns add up to -Y X^T"""
    n, m, k = 40, 16, 70
    A, B, GX, _, _, kappa = _problem(n, k)
    cf = _closed_forms(n, k)
    for trans, key in ((False, "solve"), (True, "solve_t")):
        At, Bt = _t(A, grad=True), _t(B, grad=True)
        X = gj.autograd.solve(At, Bt, block_size=m, trans=trans)
        X.backward(_t(GX))
        _close(At.grad, cf[key][0], n, kappa, U64, f"wide {key} dA")
        _close(Bt.grad, cf[key][1], n, kappa, U64, f"wide {key} dB")


@pytest.mark.parametrize("engine_dtype", ["fp64", "fp32"])
def test_closed_forms_cpu(engine_dtype):
    _compare_all(40, 16, 5, "cpu", engine_dtype)


def test_one_graph_one_inversion(monkeypatch):
    """forward and backward of 1/2 y^T inv(A) y + 1/2 log|det A| through one handle: one construction"""
    n, m = 40, 16
    A, _, _, _, y, kappa = _problem(n, 5)
    count = []
    init = gjm.Factored.__init__

    def counting(self, *a, **kw):
        count.append(1)
        return init(self, *a, **kw)

    monkeypatch.setattr(gjm.Factored, "__init__", counting)
    At, yt = _t(A, grad=True), _t(y)
    F = gj.autograd.factor(At, block_size=m)
    loss = 0.5 * (yt @ F.solve(yt)) + 0.5 * F.slogdet()[1]
    loss.backward()
    assert len(count) == 1
    _close(At.grad, _closed_forms(n, 5)["loss"], n, kappa, U64, "loss dA")
    Ai = np.linalg.inv(A)
    assert abs(float(loss.detach()) - (0.5 * y @ Ai @ y + 0.5 * np.linalg.slogdet(A)[1])) <= 32 * n * kappa * U64 * 10


def test_fp32_tensors_keep_their_dtype():
    A, B, *_ = _problem(12, 3)
    At, Bt = _t(A, dtype=torch.float32, grad=True), _t(B, dtype=torch.float32, grad=True)
    X = gj.autograd.solve(At, Bt, block_size=5)
    assert X.dtype == torch.float32
    X.sum().backward()
    assert At.grad.dtype == torch.float32 and Bt.grad.dtype == torch.float32 and At.grad.shape == (12, 12)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(200, 16), (130, 64)])
@pytest.mark.parametrize("engine_dtype", ["fp64", "fp32"])
def test_closed_forms_gpu(n, m, engine_dtype):
    _compare_all(n, m, 5, "cuda", engine_dtype)


@pytest.mark.gpu
def test_wide_rhs_gpu():
    n, m, k = 130, 64, 70
    A, B, GX, _, _, kappa = _problem(n, k)
    At, Bt = _t(A, "cuda", grad=True), _t(B, "cuda", grad=True)
    gj.autograd.solve(At, Bt, block_size=m).backward(_t(GX, "cuda"))
    assert At.grad.is_cuda and Bt.grad.is_cuda
    _close(At.grad, _closed_forms(n, k)["solve"][0], n, kappa, U64, "wide solve dA gpu")


# ---------------------------------------------------------------- guards
def test_update_between_forward_and_backward():
    A, B, *_ = _problem(12, 3)
    At = _t(A, grad=True)
    F = gj.autograd.factor(At, block_size=5)
    outs = [F.solve(_t(B)).sum(), F.slogdet()[1], F.inverse().sum()]
    F.handle.update(0.01 * np.ones(12), np.ones(12))
    for o in outs:
        with pytest.raises(RuntimeError, match="updated"):
            o.backward()
    assert At.grad is None


def test_double_backward_raises():
    A, B, *_ = _problem(12, 3)
    At = _t(A, grad=True)
    X = gj.autograd.solve(At, _t(B), block_size=5)
    (g,) = torch.autograd.grad(X.sum(), At, create_graph=True, retain_graph=True)
    with pytest.raises(RuntimeError):  # the first gradient carries no graph
        g.sum().backward()
    go = torch.ones_like(X, requires_grad=True)  # a graph through the upstream gradient: torch's own message
    (g,) = torch.autograd.grad(X, At, go, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g.sum().backward()


def test_argument_errors():
    A, B, *_ = _problem(12, 3)
    with pytest.raises(TypeError, match="gj.factor"):
        gj.autograd.factor(np.array(A))
    At = _t(A, grad=True)
    with pytest.raises(ValueError):
        gj.autograd.solve(At, _t(B), block_size=5, trans=True, precise=True)
    with pytest.raises(ValueError):
        gj.autograd.factor(At, block_size=5).solve(_t(B), trans=True, precise=True)
    with pytest.raises(gj.SingularMatrixError):
        gj.autograd.factor(torch.ones((8, 8), dtype=torch.float64, requires_grad=True), block_size=4)
    with pytest.raises(gj.SingularMatrixError):
        gj.autograd.slogdet(torch.ones((8, 8), dtype=torch.float64, requires_grad=True), block_size=4)


def test_precise_solve_is_differentiable():
    n, k = 12, 3
    A, B, GX, _, _, kappa = _problem(n, k)
    At, Bt = _t(A, grad=True), _t(B, grad=True)
    gj.autograd.solve(At, Bt, block_size=5, precise=True).backward(_t(GX))
    _close(At.grad, _closed_forms(n, k)["solve"][0], n, kappa, U64, "precise dA")


def test_existing_entry_points_still_detach():
    A, B, *_ = _problem(12, 3)
    b = _t(B[:, 0])
    x0 = gj.solve(_t(A), b, block_size=5)
    x1 = gj.solve(_t(A, grad=True), b, block_size=5)
    assert not x1.requires_grad and x1.grad_fn is None
    assert torch.equal(x0.view(torch.int64), x1.view(torch.int64))
    assert not gj.inverse(_t(A, grad=True), block_size=5).requires_grad


def test_engine_refuses_more_than_one_rank():
    """Engine.grad_matrix and Engine.vjp_inverse are single-rank: BadArgs (5) on every rank of p = 3"""
    native = gj.load_native()
    assert native.loopback_grad_probe(3, 24, 4) == [(5, 5)] * 3
    assert native.loopback_grad_probe(1, 24, 4) == [(0, 0)]
