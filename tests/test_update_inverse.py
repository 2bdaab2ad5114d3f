"""Low-rank update of the resident inverse (Engine::update_inverse, Factored.update,
DistributedGaussJordan.update, GaussJordan.run(update=)): after update(U, V) the handle stands for
A' = A + U V^T, its inverse formed by the matrix inversion lemma

    inv(A + U V^T) = X - (X U) inv(I_k + V^T X U) (V^T X),   X = inv(A)

in one pass over X (Device::rank_update).  Mirrors tests/test_solve_trans.py.

Tolerances.  After an update both solves must report every column converged (backward error <= 1e-15
against the rows of A') and agree with np.linalg.solve on A' (or its transpose) to 1e-8 relative,
the tolerance of test_solve_trans.py for these matrices.  The updated inverse must pass the
project's own gate, rho = ||A' X' - I||_inf / (||A'|| ||X'|| eps) <= RHO_PER_N n (utils/metrics.py).
A numpy simulation of the formula on exactly these inputs, the inverse stored in the engine dtype,
gave rho / n <= 0.105 against the gate's 2 (worst: random, k = 64, fp64, where kappa_1(C) ~ 1e5),
convergence in at most 3 refinement steps and at most 2.4e-12 relative error: the formula alone
stays inside both conditions.  The updated inverse differs from the old one by far more than any of
these, so an update that does nothing fails.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.models.gauss_jordan import SingularMatrixError
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
from mpi_jordan_crazy_acceleration_amd.utils.metrics import RHO_PER_N, residual_ok, residual_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 240, 16


def _uv(n, k):
    rng = np.random.default_rng(11 + k)
    U = rng.standard_normal((n, k))
    V = rng.standard_normal((n, k))
    return U, V


def _rhs(n):
    return np.random.default_rng(2).standard_normal((n, 3))


def _close(X, ref):
    return all(np.abs(X[:, j] - ref[:, j]).max() <= 1e-8 * np.abs(ref[:, j]).max() for j in range(ref.shape[1]))


def _gate(F, A2):
    """the handle's inverse against A2 through the engine's own residual and norm"""
    n = A2.shape[0]
    res = F._eng.residual_rows(np.ascontiguousarray(A2))
    na, ni = np.abs(A2).sum(axis=1).max(), F._eng.result_norm_inf()
    rho = residual_ratio(res, na, ni, F.dtype)
    print(f"rho / n = {rho / n:.3e} (gate {RHO_PER_N})")
    assert residual_ok(res, n, na, ni, F.dtype), (rho / n, RHO_PER_N)


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("k", [1, 5, 16, 64])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("gen", ["random", "randshift"])
def test_update_accuracy_one_rank(gen, dtype, k):
    A = generate_matrix(N, gen, 3)
    U, V = _uv(N, k)
    A2 = A + U @ V.T
    B = _rhs(N)
    F = gj.factor(A, block_size=M, dtype=dtype, device="cpu")
    X0 = F.inverse().copy()
    info = F.update(U, V)
    assert set(info) == {"k", "min_pivot", "cond1", "seconds"} and info["k"] == k and info["min_pivot"] > 0
    assert F.updates == 1 and F.last_update == info
    assert np.array_equal(A, generate_matrix(N, gen, 3)), "the caller's matrix was written"
    X1 = F.inverse()
    assert np.abs(X1 - X0).max() > 1e-3 * np.abs(X0).max(), "the inverse did not move"
    X = F.solve(B)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == 3
    assert _close(X, np.linalg.solve(A2, B))
    Xt = F.solve(B, trans=True)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == 3
    assert _close(Xt, np.linalg.solve(A2.T, B))
    _gate(F, A2)


@pytest.mark.parametrize("k", [1, 5, 16, 64])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("gen", ["random", "randshift"])
def test_update_accuracy_three_ranks(gen, dtype, k):
    A = generate_matrix(N, gen, 3)
    U, V = _uv(N, k)
    A2 = A + U @ V.T
    B = _rhs(N)
    g = gj.GaussJordan(block_size=M, ranks=3, device="cpu", dtype=dtype, residual="always")
    for trans in (False, True):
        rep = g.run(N, gen=gen, seed=3, rhs=B, keep_solution=True, keep_inverse=True, trans=trans, update=(U, V))
        assert rep["status"] == 0, rep["message"]
        assert rep["update"]["k"] == k and rep["update"]["min_pivot"] > 0
        assert all(c["converged"] for c in rep["axb_columns"]) and len(rep["axb_columns"]) == 3
        assert _close(rep["x"], np.linalg.solve(A2.T if trans else A2, B))
    X1 = rep["inverse"]
    na, ni = np.abs(A2).sum(axis=1).max(), np.abs(X1).sum(axis=1).max()
    print(f"rho / n = {residual_ratio(rep['residual'], na, ni, dtype) / N:.3e} (gate {RHO_PER_N})")
    assert residual_ok(rep["residual"], N, na, ni, dtype)
    X0 = np.linalg.inv(A)
    assert np.abs(X1 - X0).max() > 1e-3 * np.abs(X0).max()


# ------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_two_updates_equal_one(dtype):
    A = generate_matrix(N, "random", 3)
    U1, V1 = _uv(N, 5)
    U2, V2 = _uv(N, 16)
    A2 = A + U1 @ V1.T + U2 @ V2.T
    F = gj.factor(A, block_size=M, dtype=dtype, device="cpu")
    F.update(U1, V1)
    F.update(U2, V2)
    assert F.updates == 2 and F.last_update["k"] == 16
    _gate(F, A2)
    G = gj.factor(A, block_size=M, dtype=dtype, device="cpu")
    G.update(np.concatenate([U1, U2], axis=1), np.concatenate([V1, V2], axis=1))
    assert G.updates == 1 and G.last_update["k"] == 21
    _gate(G, A2)
    B = _rhs(N)
    for H in (F, G):
        assert _close(H.solve(B), np.linalg.solve(A2, B)) and all(i["converged"] for i in H.infos)


def test_vector_equals_one_column():
    A = generate_matrix(N, "randshift", 3)
    U, V = _uv(N, 1)
    F = gj.factor(A, block_size=M, device="cpu")
    G = gj.factor(A, block_size=M, device="cpu")
    F.update(U[:, 0], V[:, 0])
    G.update(U, V)
    assert F.last_update["k"] == 1
    assert np.array_equal(F.inverse().view(np.int64), G.inverse().view(np.int64))
    assert np.array_equal(F._a64, G._a64)


# ------------------------------------------------------------------ refusal
def _refusal(F, n, eye, to):
    e0, e1 = np.zeros(n), np.zeros(n)
    e0[0], e1[1] = 1.0, 1.0
    X0 = F.inverse()
    for U, V in ((-e0, e0), (np.stack([-e0, e1], axis=1), np.stack([e0, e1], axis=1))):  # C = 0; C = diag(0, 2)
        with pytest.raises(SingularMatrixError):
            F.update(to(U), to(V))
        assert F.updates == 0 and F.last_update is None
        X1 = F.inverse()
        assert (torch.equal(X1, X0) and torch.equal(X1, eye)) if isinstance(X1, torch.Tensor) else \
            (np.array_equal(X1.view(np.int64), X0.view(np.int64)) and np.array_equal(X1, eye))
    b = np.arange(1.0, n + 1)
    x = F.solve(to(b))  # still the old A = I
    assert np.array_equal(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, b)
    assert all(i["converged"] for i in F.infos)
    # and an update it can take still goes through
    F.update(to(e0), to(e0))  # A = diag(2, 1, ...)
    assert F.updates == 1
    x = F.solve(to(b))
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    assert x[0] == 0.5 and np.array_equal(x[1:], b[1:])


def test_singular_update_is_refused_and_leaves_the_handle():
    n = 64
    _refusal(gj.factor(np.eye(n), block_size=16, device="cpu"), n, np.eye(n), lambda a: a)


# ------------------------------------------------------------------ arguments and other forms
def test_arguments():
    A = generate_matrix(N, "randshift", 3)
    F = gj.factor(A, block_size=M, device="cpu")
    X0 = F.inverse().copy()
    with pytest.raises(ValueError):
        F.update(np.zeros((N, 65)), np.zeros((N, 65)))
    with pytest.raises(ValueError):
        F.update(np.zeros(N + 1), np.zeros(N + 1))
    with pytest.raises(ValueError):
        F.update(np.zeros((N, 2)), np.zeros((N, 3)))
    assert F.updates == 0 and np.array_equal(F.inverse(), X0)
    C = gj.load_native()
    with pytest.raises(RuntimeError):  # the engine itself: BadArgs
        F._eng.update_inverse(np.zeros((N, 65)), np.zeros((N, 65)))
    eng = C.Engine(C.host_device(1), C.self_comm(), N, M, "fp64")
    eng.generate("randshift", 3)
    with pytest.raises(RuntimeError):  # before solve()
        eng.update_inverse(np.zeros((N, 1)), np.zeros((N, 1)))


def test_torch_in_torch_out():
    A = generate_matrix(N, "randshift", 3)
    U, V = _uv(N, 5)
    A2 = A + U @ V.T
    F = gj.factor(torch.from_numpy(A), block_size=M, device="cpu")
    info = F.update(torch.from_numpy(U), torch.from_numpy(V).to(torch.float32).to(torch.float64))
    assert info["k"] == 5 and F.updates == 1
    B = torch.from_numpy(_rhs(N))
    X = F.solve(B)
    assert isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.device.type == "cpu"
    V32 = V.astype(np.float32).astype(np.float64)
    assert _close(X.numpy(), np.linalg.solve(A + U @ V32.T, B.numpy()))
    assert isinstance(F.inverse(), torch.Tensor)
    # numpy and torch arguments give the same bits
    G = gj.factor(A, block_size=M, device="cpu")
    G.update(U, V32)
    assert np.array_equal(G.inverse(), F.inverse().numpy())
    assert not np.allclose(A2, A)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_run_update_ranks_agree_and_keys(dtype):
    U, V = _uv(N, 5)
    B = _rhs(N)
    kw = dict(gen="random", seed=3, rhs=B, keep_solution=True, keep_inverse=True)
    reps = {p: gj.GaussJordan(block_size=M, ranks=p, device="cpu", dtype=dtype).run(N, update=(U, V), **kw)
            for p in (1, 3)}
    for rep in reps.values():
        assert rep["status"] == 0 and set(rep["update"]) == {"k", "min_pivot", "cond1", "seconds"}
    assert _close(reps[3]["x"], reps[1]["x"])
    A2 = generate_matrix(N, "random", 3) + U @ V.T
    assert _close(reps[1]["x"], np.linalg.solve(A2, B))
    assert np.abs(reps[3]["inverse"] - reps[1]["inverse"]).max() <= 1e-3 * np.abs(reps[1]["inverse"]).max()
    # the same run without update=: exactly the old keys, the old inverse
    old = gj.GaussJordan(block_size=M, ranks=3, device="cpu", dtype=dtype).run(N, **kw)
    assert old["status"] == 0 and "update" not in old
    assert set(reps[3]) - set(old) == {"update"} and set(old) <= set(reps[3])
    assert _close(old["x"], np.linalg.solve(generate_matrix(N, "random", 3), B))
    # a singular update through run(): reported as singular, like a singular matrix
    e0 = np.zeros(64)
    e0[0] = 1.0
    bad = gj.GaussJordan(block_size=16, ranks=3, device="cpu", dtype=dtype).run(64, gen="identity", update=(-e0, e0))
    assert bad["status"] == 1 and "update" not in bad
    with pytest.raises(ValueError):
        gj.GaussJordan(block_size=M, device="cpu").run(N, gen="random", update=(np.zeros((N, 65)), np.zeros((N, 65))))


# ------------------------------------------------------------------ one process per rank (gloo)
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
        A = generate_matrix(n, "random", 11)
        U, V = _uv(n, 3)
        B = np.random.default_rng(6).standard_normal((n, 3))
        d = DistributedGaussJordan(n, m, dtype="fp32", host_threads=2)
        d.load(A)
        st = d.solve()
        info = d.update(U, V)
        X, infos = d.solve_rhs(B, A_rows=A + U @ V.T)
        q.put((rank, st["status"], info["k"], X, [dict(i) for i in infos]))
    finally:
        dist.destroy_process_group()


def test_gloo_update_then_solve_rhs():
    import torch.multiprocessing as mp

    world, n, m = 3, 50, 6
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, n, m, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    A = generate_matrix(n, "random", 11)
    U, V = _uv(n, 3)
    B = np.random.default_rng(6).standard_normal((n, 3))
    ref = np.linalg.solve(A + U @ V.T, B)
    old = np.linalg.solve(A, B)
    for rank, status, k, X, infos in out:
        assert status == 0 and k == 3 and X.shape == B.shape
        assert np.array_equal(X, out[0][3])  # the same X on every rank
        assert all(i["converged"] for i in infos)
        assert np.abs(X - ref).max() <= 1e-8 * np.abs(ref).max()
        assert np.abs(X - old).max() > 1e-3 * np.abs(old).max()


# ------------------------------------------------------------------ schedule check, jittered ranks
def test_update_path_race_free_and_schedule_independent():
    n, m, ranks = 240, 16, 3
    U, V = _uv(n, 5)
    g = dict(block_size=m, ranks=ranks, device="cpu", dtype="fp32", residual="never", host_threads=1)
    run = dict(gen="random", seed=3, rhs="random", nrhs=3, keep_solution=True, update=(U, V))
    ref = gj.GaussJordan(comm="loopback", **g).run(n, **run)
    rep = gj.GaussJordan(comm="async", jitter_us=30.0, race_check=True, **g).run(n, **run)
    assert ref["status"] == 0 and rep["status"] == 0, rep["message"]
    assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
    assert rep["x"].shape == (n, 3) and np.array_equal(rep["x"], ref["x"])
    assert all(c["converged"] for c in rep["axb_columns"])
    assert rep["update"]["k"] == 5


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_factor_update():
    native = gj.load_native()
    n, m, k = 1024, 64, 9
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(generate_matrix(n, "randshift", 5)).to(dev, torch.float32)
    A64 = A.double()
    rng = np.random.default_rng(8)
    U = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    V = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    B = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    C = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    F = gj.factor(A, block_size=m, dtype="fp32")
    X0 = F.inverse().clone()
    info = F.update(U, V)
    assert info["k"] == k and F.updates == 1
    assert native.last_rank_update_kernel().startswith("rku")  # (the last launch: the fp64 rows of A)
    assert torch.equal(A.double(), A64), "the caller's matrix was written"
    A2 = A64 + U @ V.T
    assert float((F.inverse() - X0).abs().max()) > 1e-3 * float(X0.abs().max())
    X = F.solve(B)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == k
    Xt = F.solve(C, trans=True)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == k
    for x, b in ((X, B), (Xt, C)):
        assert x.device == A64.device and x.dtype == torch.float64 and x.shape == b.shape
    assert float((A2 @ X - B).abs().max() / B.abs().max()) < 1e-12
    assert float((A2.T @ Xt - C).abs().max() / C.abs().max()) < 1e-12


@pytest.mark.gpu
def test_gpu_update_fp64_k64_gate():
    native = gj.load_native()
    n, m, k = 2048, 128, 64
    dev = torch.device("cuda", 0)
    A = generate_matrix(n, "random", 3)
    U, V = _uv(n, k)
    F = gj.factor(torch.from_numpy(A).to(dev), block_size=m, dtype="fp64")
    X0 = F.inverse().clone()
    info = F.update(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev))
    assert info["k"] == k and native.last_rank_update_kernel() == "rku64:f64:vec"
    assert float((F.inverse() - X0).abs().max()) > 1e-3 * float(X0.abs().max())
    A2 = A + U @ V.T
    assert float((F._a64.cpu() - torch.from_numpy(A2)).abs().max()) <= 1e-12 * np.abs(A2).max()
    _gate(F, A2)


@pytest.mark.gpu
def test_gpu_run_update_three_ranks():
    n, m, k = 1536, 128, 3
    U, V = _uv(n, k)
    g = gj.GaussJordan(block_size=m, ranks=3, device="gpu", dtype="fp32", residual="never", comm="async")
    rep = g.run(n, gen="randshift", seed=3, rhs="random", nrhs=k, keep_solution=True, update=(U, V))
    assert rep["status"] == 0, rep["message"]
    assert rep["update"]["k"] == k and len(rep["axb_columns"]) == k
    for c in rep["axb_columns"]:
        assert c["converged"], c["history"]
        assert c["history"][-1] < 1e-10  # the bound of test_gpu_trans_refinement
    one = gj.GaussJordan(block_size=m, ranks=1, device="gpu", dtype="fp32", residual="never").run(
        n, gen="randshift", seed=3, rhs="random", nrhs=k, keep_solution=True, update=(U, V))
    assert one["status"] == 0 and _close(rep["x"], one["x"])
    old = gj.GaussJordan(block_size=m, ranks=1, device="gpu", dtype="fp32", residual="never").run(
        n, gen="randshift", seed=3, rhs="random", nrhs=k, keep_solution=True)
    assert np.abs(old["x"] - one["x"]).max() > 1e-3 * np.abs(one["x"]).max()  # the update shows in x


@pytest.mark.gpu
def test_gpu_singular_update_is_refused():
    n = 256
    dev = torch.device("cuda", 0)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    _refusal(gj.factor(eye.clone(), block_size=64, dtype="fp64"), n, eye, lambda a: torch.from_numpy(a).to(dev))
