"""A^T X = B from the resident inverse (Engine::solve_rhs_block with trans) and the handle that keeps
an inverse for reuse (gj.factor): every column refined in fp64 by the rule of the one-vector path,
x_0 = inv(A)^T b, r = b - A^T x, x += inv(A)^T r, each product this rank's term over its own rows
(Device::panel_rhs_t) summed over the ranks.  Mirrors tests/test_solve_block.py.

Tolerances.  A converged column has backward error ||r|| / (||A||_1 ||x|| + ||b||) <= 1e-15, the
path's own tolerance (inf-norms of the vectors; ||A^T||_inf = ||A||_1).  Against
np.linalg.solve(A.T, B) the columns are held to ||x_j - ref_j|| <= 1e-8 ||ref_j||: the crude bound
kappa_1 n 1e-15 = 2.51e4 * 240 * 1e-15 = 6e-9 for the random matrix (kappa_1 computed with numpy,
seed 3) and less for randshift; a numpy simulation of this refinement with numpy's inverse
converges in 2 steps at 6e-14 on both matrices.  The matrices are not symmetric: the transposed
solution differs from the plain one by far more than 1e-3, so a forgotten transpose fails.
"""
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


def _trans_run(device, dtype, n, m, ranks, gen, B, seed=3, **kw):
    g = gj.GaussJordan(block_size=m, ranks=ranks, device=device, dtype=dtype, residual="never", **kw)
    rep = g.run(n, gen=gen, seed=seed, rhs=B, keep_solution=True, trans=True)
    assert rep["status"] == 0, rep["message"]
    assert rep["trans"] is True
    return rep


def _check_columns(rep, A, B, fp32):
    X, cols = rep["x"], rep["axb_columns"]
    assert X.shape == B.shape and len(cols) == B.shape[1]
    ref = np.linalg.solve(A.T, B)
    plain = np.linalg.solve(A, B)
    for j, c in enumerate(cols):
        if not B[:, j].any():
            assert c["converged"] and c["steps"] == 0 and not X[:, j].any()  # a zero column: exactly 0
            continue
        assert c["converged"] and c["backward_error"] < 1e-15, (j, c)
        if fp32:
            assert c["history"][0] > 1e-7  # x = inv32(A)^T b alone: fp32 accuracy
        assert np.abs(X[:, j] - ref[:, j]).max() <= 1e-8 * np.abs(ref[:, j]).max(), j
        assert np.abs(X[:, j] - plain[:, j]).max() > 1e-3 * np.abs(plain[:, j]).max(), j  # not A x = b
    assert rep["axb_residual"] == max(c["residual"] for c in cols)
    assert rep["refine_converged"] is True


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_trans_block_accuracy(dtype, ranks):
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    B = np.concatenate([np.random.default_rng(0).standard_normal((n, 5)), np.zeros((n, 1))], axis=1)
    _check_columns(_trans_run("cpu", dtype, n, m, ranks, "random", B), A, B, dtype == "fp32")


def test_trans_two_groups_of_columns():
    n, m, k = 1000, 60, 70  # 64 + 6 columns; a ragged last block, three ranks
    A = generate_matrix(n, "randshift", 3)
    B = np.random.default_rng(1).standard_normal((n, k))
    _check_columns(_trans_run("cpu", "fp32", n, m, 3, "randshift", B), A, B, True)


def test_trans_one_vector():
    # a single vector with trans takes the block path with one column
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    b = np.random.default_rng(4).standard_normal(n)
    rep = _trans_run("cpu", "fp32", n, m, 1, "random", b)
    assert rep["x"].shape == (n, 1) and len(rep["axb_columns"]) == 1 and rep["refine_converged"] is True
    ref = np.linalg.solve(A.T, b)
    assert np.abs(rep["x"][:, 0] - ref).max() <= 1e-8 * np.abs(ref).max()


def _engine(n, m, dtype, kind, seed):
    C = gj.load_native()
    eng = C.Engine(C.host_device(2), C.self_comm(), n, m, dtype)
    eng.generate(kind, seed)
    assert eng.solve()["status"] == 0
    return eng


def test_trans_frozen_column_is_bitwise_untouched():
    # B = [A^T e_0, random]: the first column converges at sweep 0 and is frozen while the second one
    # is refined further; its x equals, bit for bit, its x from a solve of [A^T e_0] alone.  Whether a
    # random column needs a step at fp64 depends on the column, so the first few seeds are tried
    # until one does (the zero-step columns tell nothing about freezing).
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    eng = _engine(n, m, "fp64", "random", 3)
    a0 = np.ascontiguousarray(A[0, :])  # A^T e_0
    X1, i1, _ = eng.solve_rhs_block(a0[:, None].copy(), gen=("random", 3), trans=True)
    assert i1[0]["converged"] and i1[0]["steps"] == 0
    assert np.abs(X1[:, 0] - np.eye(n)[0]).max() < 1e-9
    tried = 0
    for seed in range(40):
        B = np.stack([a0, np.random.default_rng(seed).standard_normal(n)], axis=1)
        X, infos, meta = eng.solve_rhs_block(B, gen=("random", 3), trans=True)
        assert infos[0]["converged"] and infos[0]["steps"] == 0 and len(infos[0]["history"]) == 1
        assert np.array_equal(X[:, 0], X1[:, 0])
        if infos[1]["steps"] >= 1:
            assert meta["sweeps"] >= 2  # column 0 sat frozen through at least one more sweep
            tried += 1
            if tried == 3:
                break
    assert tried > 0, "no random column needed a refinement step"


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_plain_path_is_unchanged(dtype):
    # trans=False and the keyword omitted are the same call, and a run's x is that of the call form
    # without the keyword
    n, m = 240, 16
    eng = _engine(n, m, dtype, "random", 3)
    B = np.random.default_rng(5).standard_normal((n, 4))
    X0, i0, _ = eng.solve_rhs_block(B, gen=("random", 3))
    X1, i1, _ = eng.solve_rhs_block(B, gen=("random", 3), trans=False)
    assert np.array_equal(X0, X1) and [dict(i) for i in i0] == [dict(i) for i in i1]
    g = gj.GaussJordan(block_size=m, device="cpu", dtype=dtype, residual="never")
    r0 = g.run(n, gen="random", seed=3, rhs=B, keep_solution=True)
    r1 = g.run(n, gen="random", seed=3, rhs=B, keep_solution=True, trans=False)
    assert r0["status"] == 0 and "trans" not in r0 and "trans" not in r1
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["x"], X0)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_factor(dtype):
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    rng = np.random.default_rng(7)
    B, C = rng.standard_normal((n, 4)), rng.standard_normal((n, 3))
    F = gj.factor(A, block_size=m, dtype=dtype, device="cpu")
    assert F.n == n and F.dtype == dtype
    X = F.solve(B)
    assert np.array_equal(X, gj.solve(A, B, block_size=m, dtype=dtype, device="cpu"))
    x = F.solve(B[:, 0])  # a vector keeps its shape, and is the one-vector path of gj.solve
    assert x.shape == (n,) and np.array_equal(x, gj.solve(A, B[:, 0], block_size=m, dtype=dtype, device="cpu"))
    Xt = F.solve(C, trans=True)  # the same inversion
    ref = np.linalg.solve(A.T, C)
    assert Xt.shape == C.shape and all(i["converged"] for i in F.infos)
    for j in range(C.shape[1]):
        assert np.abs(Xt[:, j] - ref[:, j]).max() <= 1e-8 * np.abs(ref[:, j]).max()
    xt = F.solve(C[:, 1], trans=True)
    assert xt.shape == (n,) and np.array_equal(xt, Xt[:, 1])
    assert np.array_equal(xt, gj.solve(A, C[:, 1], block_size=m, dtype=dtype, device="cpu", trans=True))
    assert np.array_equal(F.inverse(), gj.inverse(A, block_size=m, dtype=dtype, device="cpu"))
    # torch in, torch out
    Ft = gj.factor(torch.from_numpy(A), block_size=m, dtype=dtype, device="cpu")
    Xtt = Ft.solve(torch.from_numpy(C), trans=True)
    assert isinstance(Xtt, torch.Tensor) and Xtt.dtype == torch.float64 and np.array_equal(Xtt.numpy(), Xt)
    assert isinstance(Ft.inverse(), torch.Tensor) and np.array_equal(Ft.inverse().numpy(), F.inverse())
    with pytest.raises(ValueError):
        F.solve(np.zeros(n + 1))


def _cli(gj_bin, *args):
    p = subprocess.run([gj_bin, "--device", "cpu", *map(str, args)], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_trans(gj_bin, tmp_path):
    xf = tmp_path / "x.bin"
    n, m = 300, 16
    base = ["--dtype", "fp32", "--gen", "randshift", "--seed", 2, "--rhs", "random", "--json"]
    rc, out, err = _cli(gj_bin, *base, "--trans", "--nrhs", 4, "--out-x", xf, n, m)
    assert rc == 0, err
    d = json.loads(err.strip().splitlines()[-1])
    assert d["trans"] is True and d["nrhs"] == 4
    assert all(d["refine_converged_cols"]) and d["refine_converged"] is True
    lines = out.strip().split("\n")
    assert lines[-1].startswith("ATx-b residual: ") and not any(ln.startswith("Ax-b residual") for ln in lines)
    assert float(lines[-1].split()[-1]) == pytest.approx(d["axb_residual"], rel=1e-5)
    X = np.fromfile(xf, dtype="<f8").reshape(n, 4)
    A = generate_matrix(n, "randshift", 2)
    # the right-hand sides of the plain run: X_plain = inv(A) B, so B = A X_plain up to 1e-12
    rc0, _, err0 = _cli(gj_bin, *base, "--nrhs", 4, "--out-x", xf, n, m)
    assert rc0 == 0, err0
    B = A @ np.fromfile(xf, dtype="<f8").reshape(n, 4)
    ref = np.linalg.solve(A.T, B)
    assert np.abs(X - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.abs(A.T @ X - B).max() < 1e-9 and max(d["axb_residual_cols"]) < 1e-9
    # one vector with --trans
    rc1, out1, err1 = _cli(gj_bin, *base, "--trans", n, m)
    d1 = json.loads(err1.strip().splitlines()[-1])
    assert rc1 == 0 and d1["trans"] is True and "nrhs" not in d1 and out1.strip().split("\n")[-1].startswith("ATx-b")
    # without --trans nothing changes: today's form, the same stdout as --nrhs 1, no "trans" key
    rc2, out2, _ = _cli(gj_bin, *base, "--nrhs", 1, n, m)
    rc3, out3, err3 = _cli(gj_bin, *base, n, m)
    strip = lambda s: "\n".join(ln for ln in s.split("\n") if not ln.startswith("glob_time"))  # noqa: E731
    assert rc2 == 0 and rc3 == 0 and strip(out2) == strip(out3)
    assert out3.strip().split("\n")[-1].startswith("Ax-b residual: ")
    assert "trans" not in json.loads(err3.strip().splitlines()[-1])


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
        B = np.random.default_rng(6).standard_normal((n, 3))
        d = DistributedGaussJordan(n, m, dtype="fp32", host_threads=2)
        d.load(A)
        st = d.solve()
        X, infos = d.solve_rhs(B, A_rows=A, trans=True)
        q.put((rank, st["status"], X, [dict(i) for i in infos]))
    finally:
        dist.destroy_process_group()


def test_gloo_solve_rhs_trans():
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
    B = np.random.default_rng(6).standard_normal((n, 3))
    ref = np.linalg.solve(A.T, B)
    for rank, status, X, infos in out:
        assert status == 0 and X.shape == B.shape
        assert np.array_equal(X, out[0][2])  # the same X on every rank
        assert all(i["converged"] for i in infos)
        assert np.abs(X - ref).max() <= 1e-8 * np.abs(ref).max()


# ------------------------------------------------------------------ schedule check, jittered ranks
def test_trans_path_race_free_and_schedule_independent():
    n, m, ranks = 240, 16, 3
    g = dict(block_size=m, ranks=ranks, device="cpu", dtype="fp32", residual="never", host_threads=1)
    run = dict(gen="random", seed=3, rhs="random", nrhs=3, keep_solution=True, trans=True)
    ref = gj.GaussJordan(comm="loopback", **g).run(n, **run)
    rep = gj.GaussJordan(comm="async", jitter_us=30.0, race_check=True, **g).run(n, **run)
    assert ref["status"] == 0 and rep["status"] == 0, rep["message"]
    assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
    assert rep["x"].shape == (n, 3) and np.array_equal(rep["x"], ref["x"])
    assert all(c["converged"] for c in rep["axb_columns"])


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n,m,gen,k,kw", [
    ("fp64", 2048, 128, "random", 5, {}),
    ("fp32", 3000, 64, "randshift", 17, {}),
    ("fp32", 1536, 128, "randshift", 3, dict(ranks=3, comm="async")),
])
def test_gpu_trans_refinement(dtype, n, m, gen, k, kw):
    kw = dict(kw)
    ranks = kw.pop("ranks", 1)
    g = gj.GaussJordan(block_size=m, ranks=ranks, device="gpu", dtype=dtype, residual="never", **kw)
    rep = g.run(n, gen=gen, seed=3, rhs="random", nrhs=k, keep_solution=True, trans=True)
    assert rep["status"] == 0, rep["message"]
    assert rep["trans"] is True and len(rep["axb_columns"]) == k and rep["x"].shape == (n, k)
    for c in rep["axb_columns"]:
        assert c["converged"], c["history"]
        assert c["history"][-1] < 1e-10  # the bound of test_gpu_block_refinement


@pytest.mark.gpu
def test_gpu_factor():
    native = gj.load_native()
    n, m = 1024, 64
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(generate_matrix(n, "randshift", 5)).to(dev, torch.float32)
    A64 = A.double()  # the fp32 matrix itself, widened: what the handle refines against
    rng = np.random.default_rng(8)
    B = torch.from_numpy(rng.standard_normal((n, 9))).to(dev)
    C = torch.from_numpy(rng.standard_normal((n, 9))).to(dev)
    F = gj.factor(A, block_size=m, dtype="fp32")  # one fp32 inversion
    assert F.n == n and F.dtype == "fp32"
    X = F.solve(B)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == 9
    Xt = F.solve(C, trans=True)
    assert all(i["converged"] for i in F.infos) and len(F.infos) == 9
    assert native.last_rhs_t_kernel().startswith("rhst16:f")
    for x, b in ((X, B), (Xt, C)):
        assert x.device == A64.device and x.dtype == torch.float64 and x.shape == b.shape
    assert float((A64 @ X - B).abs().max() / B.abs().max()) < 1e-12
    assert float((A64.T @ Xt - C).abs().max() / C.abs().max()) < 1e-12
    inv = F.inverse()
    assert inv.device == A64.device and inv.dtype == torch.float32
    assert float((inv.double() @ A64 - torch.eye(n, device=dev, dtype=torch.float64)).abs().max()) < 1e-3
