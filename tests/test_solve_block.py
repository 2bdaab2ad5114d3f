"""A X = B for a block of right-hand sides (Engine::solve_rhs_block): every column refined in fp64 by
the rule of the one-vector path (Engine::solve_rhs, tests/test_refine.py), all columns per sweep.

Tolerances.  A converged column has backward error ||r|| / (||A|| ||x|| + ||b||) <= 1e-15, the path's
own tolerance.  Against np.linalg.solve the columns are held to ||x_j - x_ref|| <= 1e-9 ||x_ref||
(inf-norms): kappa_inf n 1e-15 is the crude bound, 1.8e4 * 240 * 1e-15 = 4e-9 for the random matrix
(kappa_inf = 1.82e4, seed 3, computed with numpy) and far less for randshift (kappa_inf = 386 at
n = 1000), and the one-vector test passes at the same 1e-9.
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


def _block_run(device, dtype, n, m, ranks, gen, B, seed=3, **kw):
    g = gj.GaussJordan(block_size=m, ranks=ranks, device=device, dtype=dtype, residual="never", **kw)
    rep = g.run(n, gen=gen, seed=seed, rhs=B, keep_solution=True)
    assert rep["status"] == 0, rep["message"]
    return rep


def _check_columns(rep, A, B, fp32):
    X, cols = rep["x"], rep["axb_columns"]
    assert X.shape == B.shape and len(cols) == B.shape[1]
    ref = np.linalg.solve(A, B)
    for j, c in enumerate(cols):
        if not B[:, j].any():
            assert c["converged"] and c["steps"] == 0 and not X[:, j].any()  # a zero column: exactly 0
            continue
        assert c["converged"] and c["backward_error"] < 1e-15, (j, c)
        if fp32:
            assert c["history"][0] > 1e-7  # x = inv32(A) b alone: fp32 accuracy
        assert np.abs(X[:, j] - ref[:, j]).max() <= 1e-9 * np.abs(ref[:, j]).max(), j
    assert rep["axb_residual"] == max(c["residual"] for c in cols)
    assert rep["refine_converged"] is True


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_block_matches_one_vector_accuracy(dtype, ranks):
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    B = np.concatenate([np.random.default_rng(0).standard_normal((n, 5)), np.zeros((n, 1))], axis=1)
    _check_columns(_block_run("cpu", dtype, n, m, ranks, "random", B), A, B, dtype == "fp32")


def test_two_groups_of_columns():
    n, m, k = 1000, 60, 70  # 64 + 6 columns; a ragged last block, three ranks
    A = generate_matrix(n, "randshift", 3)
    B = np.random.default_rng(1).standard_normal((n, k))
    _check_columns(_block_run("cpu", "fp32", n, m, 3, "randshift", B), A, B, True)


def _engine(n, m, dtype, kind, seed):
    C = gj.load_native()
    eng = C.Engine(C.host_device(2), C.self_comm(), n, m, dtype)
    eng.generate(kind, seed)
    assert eng.solve()["status"] == 0
    return eng


def test_frozen_column_is_bitwise_untouched():
    # B = [A e_0, random]: the first column converges at sweep 0 and is frozen while the second one
    # is refined further; its x equals, bit for bit, its x from a solve of [A e_0] alone.  Whether a
    # random column needs a step at fp64 depends on the column, so the first few seeds are tried
    # until one does (the zero-step columns tell nothing about freezing).
    n, m = 240, 16
    A = generate_matrix(n, "random", 3)
    eng = _engine(n, m, "fp64", "random", 3)
    X1, i1, _ = eng.solve_rhs_block(np.ascontiguousarray(A[:, :1]), gen=("random", 3))
    assert i1[0]["converged"] and i1[0]["steps"] == 0
    tried = 0
    for seed in range(40):
        B = np.stack([A[:, 0], np.random.default_rng(seed).standard_normal(n)], axis=1)
        X, infos, meta = eng.solve_rhs_block(B, gen=("random", 3))
        assert infos[0]["converged"] and infos[0]["steps"] == 0 and len(infos[0]["history"]) == 1
        assert np.array_equal(X[:, 0], X1[:, 0])
        if infos[1]["steps"] >= 1:
            assert meta["sweeps"] >= 2  # column 0 sat frozen through at least one more sweep
            tried += 1
            if tried == 3:
                break
    assert tried > 0, "no random column needed a refinement step"


@pytest.mark.parametrize("n,m", [(12, 3), (16, 4)])
def test_diverging_columns_return_best_iterate(n, m):
    # test_refine.py::test_diverging_refinement_returns_best_iterate, per column: b_j = (j + 1) ones
    rep = gj.GaussJordan(block_size=m, device="cpu", dtype="fp32").run(n, gen="hilbert", rhs="ones", nrhs=3)
    assert rep["status"] == 0 and not rep["refine_converged"]
    assert len(rep["axb_columns"]) == 3
    for j, c in enumerate(rep["axb_columns"]):
        h = c["history"]
        assert not c["converged"]
        assert len(h) >= 2 and h[-1] > h[0]
        assert c["residual"] == pytest.approx(min(h) * (j + 1), rel=1e-12)  # ||b_j||_inf = j + 1
        assert c["steps"] == h.index(min(h))


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_one_column_block_agrees_with_solve_rhs(dtype):
    n, m = 240, 16
    eng = _engine(n, m, dtype, "random", 3)
    b = np.random.default_rng(4).standard_normal(n)
    x, info = eng.solve_rhs_generated("random", 3, b)
    X, infos, _ = eng.solve_rhs_block(b[:, None].copy(), gen=("random", 3))
    assert info["converged"] and infos[0]["converged"]
    assert np.abs(X[:, 0] - x).max() <= 1e-12 * np.abs(x).max()


def test_solve_with_matrix_rhs_is_refined():
    # before the block path this was inverse(A) @ B on the host: fp32 accuracy, about 1e-5
    n = 240
    A = generate_matrix(n, "random", 3)
    B = np.random.default_rng(2).standard_normal((n, 4))
    X = gj.solve(A, B, block_size=16, device="cpu", dtype="fp32")
    assert X.shape == B.shape
    assert np.abs(A @ X - B).max() / np.abs(B).max() < 1e-12
    Xt = gj.solve(torch.from_numpy(A), torch.from_numpy(B), block_size=16, device="cpu", dtype="fp32")
    assert isinstance(Xt, torch.Tensor) and Xt.shape == B.shape and np.array_equal(Xt.numpy(), X)


def _cli(gj_bin, *args):
    p = subprocess.run([gj_bin, "--device", "cpu", *map(str, args)], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_nrhs(gj_bin, tmp_path):
    xf = tmp_path / "x.bin"
    base = ["--dtype", "fp32", "--gen", "randshift", "--seed", 2, "--rhs", "random", "--json"]
    rc, out, err = _cli(gj_bin, *base, "--nrhs", 4, "--out-x", xf, 300, 16)
    assert rc == 0, err
    d = json.loads(err.strip().splitlines()[-1])
    assert d["nrhs"] == 4
    for key in ("axb_residual_cols", "axb_backward_error_cols", "refine_steps_cols", "refine_converged_cols",
                "axb_history_cols"):
        assert len(d[key]) == 4, key
    assert all(d["refine_converged_cols"]) and d["refine_converged"] is True
    assert d["axb_residual"] == pytest.approx(max(d["axb_residual_cols"]), rel=1e-5)
    lines = out.strip().split("\n")
    assert lines[-1].startswith("Ax-b residual: ") and sum(ln.startswith("Ax-b residual") for ln in lines) == 1
    assert float(lines[-1].split()[-1]) == pytest.approx(d["axb_residual"], rel=1e-5)
    X = np.fromfile(xf, dtype="<f8").reshape(300, 4)
    A = generate_matrix(300, "randshift", 2)
    # column 0 is the right-hand side of the one-vector run (seed + 0)
    rc1, out1, err1 = _cli(gj_bin, *base, "--out-x", xf, 300, 16)
    x = np.fromfile(xf, dtype="<f8")
    assert rc1 == 0 and np.abs(X[:, 0] - x).max() <= 1e-12 * np.abs(x).max()
    assert max(d["axb_residual_cols"]) < 1e-9 and np.isfinite(A @ X).all()
    # without --nrhs nothing changes: the same stdout as --nrhs 1
    rc2, out2, _ = _cli(gj_bin, *base, "--nrhs", 1, 300, 16)
    rc3, out3, _ = _cli(gj_bin, *base, 300, 16)
    strip = lambda s: "\n".join(ln for ln in s.split("\n") if not ln.startswith("glob_time"))  # noqa: E731
    assert rc2 == 0 and rc3 == 0 and strip(out2) == strip(out3)


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
        X, infos = d.solve_rhs(B, A_rows=A)
        Xg, infos_g = d.solve_rhs(B[:, 0], A_rows=A[d.global_row_ids()])
        q.put((rank, st["status"], X, [dict(i) for i in infos], Xg))
    finally:
        dist.destroy_process_group()


def test_gloo_solve_rhs():
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
    ref = np.linalg.solve(A, B)
    for rank, status, X, infos, Xg in out:
        assert status == 0 and X.shape == B.shape and Xg.shape == (n,)
        assert np.array_equal(X, out[0][2])  # the same X on every rank
        assert all(i["converged"] for i in infos)
        assert np.abs(X - ref).max() <= 1e-9 * np.abs(ref).max()
        assert np.abs(Xg - ref[:, 0]).max() <= 1e-9 * np.abs(ref[:, 0]).max()


# ------------------------------------------------------------------ schedule check, jittered ranks
def test_block_path_race_free_and_schedule_independent():
    n, m, ranks = 240, 16, 3
    g = dict(block_size=m, ranks=ranks, device="cpu", dtype="fp32", residual="never", host_threads=1)
    ref = gj.GaussJordan(comm="loopback", **g).run(n, gen="random", seed=3, rhs="random", nrhs=3, keep_solution=True)
    rep = gj.GaussJordan(comm="async", jitter_us=30.0, race_check=True, **g).run(
        n, gen="random", seed=3, rhs="random", nrhs=3, keep_solution=True)
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
def test_gpu_block_refinement(dtype, n, m, gen, k, kw):
    kw = dict(kw)
    ranks = kw.pop("ranks", 1)
    g = gj.GaussJordan(block_size=m, ranks=ranks, device="gpu", dtype=dtype, residual="never", **kw)
    rep = g.run(n, gen=gen, seed=3, rhs="random", nrhs=k, keep_solution=True)
    assert rep["status"] == 0, rep["message"]
    assert len(rep["axb_columns"]) == k and rep["x"].shape == (n, k)
    for c in rep["axb_columns"]:
        assert c["converged"], c["history"]
        assert c["history"][-1] < 1e-10  # the bound of test_gpu_fp32_refinement


@pytest.mark.gpu
def test_gpu_solve_resident_block():
    native = gj.load_native()
    n, m = 1024, 64
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(generate_matrix(n, "randshift", 5)).to(dev, torch.float32)
    A64 = A.double()
    B9 = torch.from_numpy(np.random.default_rng(8).standard_normal((n, 9))).to(dev, torch.float32)
    before = native.last_rhs_kernel()
    for b in (B9[:, 0].contiguous(), B9[:, :1].contiguous()):  # k = 1: the one-vector path
        x = gj.solve(A, b, block_size=m, dtype="fp32")
        assert native.last_rhs_kernel() == before
        assert x.device == A.device and x.dtype == A.dtype and x.shape == b.shape
        r = (A64 @ x.double() - b.double()).abs().max() / b.double().abs().max()
        assert float(r) < 1e-5  # x rounded to A's dtype (fp32)
    X = gj.solve(A, B9, block_size=m, dtype="fp32")
    assert native.last_rhs_kernel().startswith("rhs16:")
    assert X.device == A.device and X.dtype == A.dtype and X.shape == B9.shape
    Xd, infos = gj.GaussJordan(block_size=m, dtype="fp32", residual="never").solve_resident(A64, B9.double())
    assert len(infos) == 9 and all(i["converged"] for i in infos)
    assert Xd.dtype == torch.float64 and Xd.device == A.device
    r = (A64 @ Xd - B9.double()).abs().max() / B9.double().abs().max()
    assert float(r) < 1e-12
    assert float((X.double() - Xd).abs().max()) <= 1e-6 * float(Xd.abs().max())
