"""Extra-precise refinement: solve(..., precise=True) (Engine::solve_rhs_block with precise), on the host
executor and, at the same sizes, on the GPU.

Systems with an exactly known solution.  rng = default_rng(seed); L = tril(rng.integers(-1, 2, (n, n)) *
(rng.random((n, n)) < dens), -1) + I, U likewise with triu(., 1) + I, A = (L @ U)[rng.permutation(n)],
x_true = default_rng(100 + seed).integers(-9, 10, (n, k)), b = A @ x_true: small integers, so A and b
are exact in fp64 (asserted: |A| < 2^20, |b| < 2^50) and x_true is the solution.  Unit triangular
factors with entries in {-1, 0, 1} make these matrices ill-conditioned at small n.

Seeds, picked on the host executor such that the sweep does not report a singular matrix, numpy's
kappa_inf is >= 1e8 (fp64 engine) or kappa_inf 2^-24 < 0.1 (fp32 engine), and the solve without the
option is at least 100 times less accurate:
    fp64 engine  (n, dens, m, seed)  kappa_inf    error without  with the option
                 (96, .25, 16, 1)    2.9e8        1.5e-10        4.9e-17
                 (128, .25, 32, 2)   1.7e10       1.1e-9         9.1e-20
                 (128, .25, 32, 8)   1.2e11       2.4e-8         8.9e-20
                 (200, .15, 48, 5)   1.1e11       1.9e-8         4.3e-18     (n ragged)
                 (256, .12, 48, 0)   1.2e11       1.8e-8         3.7e-19     (n ragged)
    fp32 engine  (48, .25, 16, 3)    1.7e5        3.5e-13        9.9e-17
                 (64, .25, 32, 0)    8.0e5        9.4e-13        2.4e-19
(errors: max over the columns of ||x - x_true||_inf / ||x_true||_inf; without: the smallest column).
On the MI355X the same seeds give, over the columns: without the option 3.5e-10 ... 1.8e-7 (fp64 engine)
and 2.3e-13 ... 3.1e-12 (fp32 engine), with it <= 9.9e-17 after 1-3 (fp64) and 6-7 (fp32) corrections.

Assertions.  With precise=True every column is `converged` and ||x - x_true||_inf / ||x_true||_inf <=
2^-52 (the exactly rounded answer has error 0; 2 u is what convergence at delta <= u ||x|| guarantees)
and err_est is at least the true error.  Without it, on the same inputs, the error is at least 100
times larger -- the test that fails without the feature, together with the keyword's absence.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SYS64 = [(96, .25, 16, 1), (128, .25, 32, 2), (128, .25, 32, 8), (200, .15, 48, 5), (256, .12, 48, 0)]
SYS32 = [(48, .25, 16, 3), (64, .25, 32, 0)]
NEW_KEYS = ("dx_rel", "dx_ratio", "err_est")


@functools.lru_cache(maxsize=None)
def _system(n, dens, seed, k=3):
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-1, 2, (n, n)) * (rng.random((n, n)) < dens), -1) + np.eye(n)
    Uu = np.triu(rng.integers(-1, 2, (n, n)) * (rng.random((n, n)) < dens), 1) + np.eye(n)
    A = (L @ Uu)[rng.permutation(n)]
    xt = np.random.default_rng(100 + seed).integers(-9, 10, (n, k)).astype(np.float64)
    b = A @ xt
    assert np.abs(A).max() < 2 ** 20 and np.abs(b).max() < 2 ** 50  # exact
    for t in (A, xt, b):
        t.setflags(write=False)
    return A, xt, b, float(np.linalg.cond(A, np.inf))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a, device):
    return a if device == "cpu" else torch.from_numpy(np.array(a)).to(device)


@functools.lru_cache(maxsize=None)
def _factored(case, dt, device):
    n, dens, m, seed = case
    return gj.factor(_dev(_system(n, dens, seed)[0], device), block_size=m, dtype=dt)


def _errors(x, xt):
    x2, t2 = x.reshape(xt.shape[0], -1), xt.reshape(xt.shape[0], -1)
    return np.abs(x2 - t2).max(axis=0) / np.abs(t2).max(axis=0)


def _accuracy_case(device, case, dt):
    n, dens, m, seed = case
    A, xt, b, kappa = _system(n, dens, seed)
    if dt == "fp64":
        assert kappa >= 1e8
    else:
        assert kappa * 2.0 ** -24 < 0.1
    F = _factored(case, dt, device)
    x1 = _np(F.solve(_dev(b, device), precise=True))
    on = [dict(i) for i in F.infos]
    x0 = _np(F.solve(_dev(b, device)))
    e1, e0 = _errors(x1, xt), _errors(x0, xt)
    for j, info in enumerate(on):
        print(f"n{n} seed {seed} {dt} kappa {kappa:.2e} col {j}: error {e0[j]:.3e} -> {e1[j]:.3e}, steps {info['steps']}, "
              f"dx_rel {info['dx_rel']:.3e} dx_ratio {info['dx_ratio']:.3e} err_est {info['err_est']:.3e}")
    for j, info in enumerate(on):
        assert info["converged"], (j, info)
        assert e1[j] <= 2.0 ** -52, (j, e1[j])
        assert info["err_est"] >= e1[j] and info["dx_rel"] <= U and 0 <= info["dx_ratio"] < 1, (j, info)
        assert e0[j] >= 100 * max(e1[j], 2.0 ** -52), (j, e0[j], e1[j])
    # a vector takes the block path as one column
    xv = _np(F.solve(_dev(b[:, 0].copy(), device), precise=True))
    assert xv.shape == (n,) and len(F.infos) == 1 and np.array_equal(xv, x1[:, 0])
    assert {k: v for k, v in F.infos[0].items()} == on[0]


@pytest.mark.parametrize("case", SYS64, ids=lambda c: f"n{c[0]}m{c[2]}s{c[3]}")
def test_fp64_engine_host(case):
    _accuracy_case("cpu", case, "fp64")


@pytest.mark.parametrize("case", SYS32, ids=lambda c: f"n{c[0]}m{c[2]}s{c[3]}")
def test_fp32_engine_host(case):
    _accuracy_case("cpu", case, "fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SYS64, ids=lambda c: f"n{c[0]}m{c[2]}s{c[3]}")
def test_fp64_engine_gpu(case):
    native = gj.load_native()
    _accuracy_case("cuda", case, "fp64")
    assert native.last_rhs_dd_kernel().startswith("rhsdd16:f64:"), native.last_rhs_dd_kernel()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SYS32, ids=lambda c: f"n{c[0]}m{c[2]}s{c[3]}")
def test_fp32_engine_gpu(case):
    _accuracy_case("cuda", case, "fp32")


# ------------------------------------------------------------------ a diverging column
def _diverging(device):
    # kappa eps_32 > 1: the fp32 inverse cannot contract the error.  The column stops unconverged and the
    # iterate with the smallest correction is returned: never a larger one than x_0's
    for case in ((128, .25, 32, 8), (128, .25, 32, 2)):
        n, dens, m, seed = case
        A, xt, b, kappa = _system(n, dens, seed)
        assert kappa * 2.0 ** -24 > 1
        F = _factored(case, "fp32", device)
        x = _np(F.solve(_dev(b, device), precise=True))
        infos = [dict(i) for i in F.infos]
        x0 = _np(F.solve(_dev(b, device), precise=True, max_refine=0))
        first = [dict(i) for i in F.infos]
        for j, (a, z) in enumerate(zip(infos, first)):
            print(f"seed {seed} col {j}: steps {a['steps']} dx_rel {a['dx_rel']:.3e} (x_0: {z['dx_rel']:.3e}) "
                  f"dx_ratio {a['dx_ratio']:.3e} err_est {a['err_est']:.3e}")
            assert not a["converged"] and not z["converged"] and z["steps"] == 0
            # the rule compares the corrections themselves: delta = dx_rel ||x||_inf of each iterate (the
            # division and this product round once each, hence 4 u)
            delta, delta0 = a["dx_rel"] * np.abs(x[:, j]).max(), z["dx_rel"] * np.abs(x0[:, j]).max()
            assert delta <= delta0 * (1 + 4 * U), (delta, delta0)
            assert a["err_est"] >= a["dx_rel"]
            if a["steps"] == 0:
                assert np.array_equal(x[:, j], x0[:, j])


def test_diverging_column_host():
    _diverging("cpu")


@pytest.mark.gpu
def test_diverging_column_gpu():
    _diverging("cuda")


# ------------------------------------------------------------------ zero and NaN columns, groups, frozen columns
def _special_columns(device):
    case = (128, .25, 32, 2)
    A, xt, b, _ = _system(*case[:2], case[3])
    F = _factored(case, "fp64", device)
    ref = _np(F.solve(_dev(b, device), precise=True))
    B = np.array(b)
    B[:, 1] = 0.0
    x = _np(F.solve(_dev(B, device), precise=True))
    z = F.infos[1]
    assert (x[:, 1] == 0).all() and z["converged"] and z["steps"] == 0 and z["dx_rel"] == 0
    assert np.array_equal(x[:, [0, 2]], ref[:, [0, 2]])
    B = np.array(b)
    B[5, 2] = np.nan
    x = _np(F.solve(_dev(B, device), precise=True))
    c = F.infos[2]
    assert not c["converged"] and c["steps"] == 0 and np.isnan(c["dx_rel"]) and np.isnan(x[:, 2]).any()
    assert np.array_equal(x[:, :2], ref[:, :2]) and all(i["converged"] for i in F.infos[:2])


def test_zero_and_nan_columns_host():
    _special_columns("cpu")


@pytest.mark.gpu
def test_zero_and_nan_columns_gpu():
    _special_columns("cuda")


def _groups_and_frozen(device):
    # 70 columns: a group of 64 and one of 6.  Exact right-hand sides, random ones and a zero column
    # stop after different numbers of corrections; a column that stopped after s of them must hold what
    # a run with a budget of s corrections returns for it: later sweeps did not touch it
    case = (200, .15, 48, 5)
    n = case[0]
    A, xt, b, _ = _system(case[0], case[1], case[3], 70)
    B = np.array(b)
    B[:, 1::2] = np.random.default_rng(5).standard_normal((n, 35))
    B[:, 4] = 0.0
    F = _factored(case, "fp64", device)
    X = _np(F.solve(_dev(B, device), precise=True))
    infos = [dict(i) for i in F.infos]
    assert len(infos) == 70 and all(i["converged"] for i in infos)
    steps = sorted({i["steps"] for i in infos})
    assert len(steps) >= 3, steps
    exact = [j for j in range(0, 70, 2) if j != 4]
    assert (_errors(X[:, exact], xt[:, exact]) <= 2.0 ** -52).all()
    for s in steps:
        Xs = _np(F.solve(_dev(B, device), precise=True, max_refine=s))
        for j, i in enumerate(infos):
            if i["steps"] == s:
                assert np.array_equal(Xs[:, j].view(np.int64), X[:, j].view(np.int64)), (s, j)
                assert F.infos[j]["converged"]


def test_groups_and_frozen_columns_host():
    _groups_and_frozen("cpu")


@pytest.mark.gpu
def test_groups_and_frozen_columns_gpu():
    _groups_and_frozen("cuda")


# ------------------------------------------------------------------ the option off changes nothing
def _option_off(device):
    case = (96, .25, 16, 1)
    A, xt, b, _ = _system(*case[:2], case[3])
    for dt in ("fp64", "fp32"):
        F = _factored(case, dt, device)
        for bb in (b, b[:, 0].copy()):
            x0 = _np(F.solve(_dev(bb, device)))
            i0 = [dict(i) for i in F.infos]
            x1 = _np(F.solve(_dev(bb, device), precise=False))
            i1 = [dict(i) for i in F.infos]
            assert np.array_equal(x0.view(np.int64), x1.view(np.int64)) and i0 == i1
            assert all(k not in i for i in i0 for k in NEW_KEYS)
            xb = _np(F.solve(_dev(bb, device), bounds=True))
            assert all(k not in i for i in F.infos for k in NEW_KEYS)
            if bb.ndim == 2:  # (a vector with bounds takes the block path, without it the one-vector path)
                assert np.array_equal(xb.view(np.int64), x0.view(np.int64))


def test_option_off_host():
    _option_off("cpu")
    # the vector path is still the one-vector path: no per-column infos in the report without a flag
    case = (96, .25, 16, 1)
    A, xt, b, _ = _system(*case[:2], case[3])
    g = gj.GaussJordan(block_size=16, device="cpu", residual="never")
    off = g.run(96, input=A, rhs=b[:, 0], keep_solution=True)
    assert "axb_columns" not in off and "precise" not in off
    on = g.run(96, input=A, rhs=b[:, 0], keep_solution=True, precise=True)
    assert on["precise"] is True and len(on["axb_columns"]) == 1 and all(k in on["axb_columns"][0] for k in NEW_KEYS)
    assert _errors(on["x"], xt[:, 0])[0] <= 2.0 ** -52 <= 1e-12 <= _errors(off["x"], xt[:, 0])[0]
    many = g.run(96, input=A, rhs=b, keep_solution=True)
    assert all(k not in c for c in many["axb_columns"] for k in NEW_KEYS)
    x = gj.solve(A, b, block_size=16, precise=True)
    assert (_errors(x, xt) <= 2.0 ** -52).all()


@pytest.mark.gpu
def test_option_off_gpu():
    _option_off("cuda")


# ------------------------------------------------------------------ with bounds; refused with trans
def _with_bounds(device):
    for case, dt in (((128, .25, 32, 2), "fp64"), ((200, .15, 48, 5), "fp64"), ((48, .25, 16, 3), "fp32")):
        A, xt, b, _ = _system(*case[:2], case[3])
        F = _factored(case, dt, device)
        x = _np(F.solve(_dev(b, device), precise=True, bounds=True))
        both = [dict(i) for i in F.infos]
        x1 = _np(F.solve(_dev(b, device), precise=True))
        assert np.array_equal(x.view(np.int64), x1.view(np.int64))
        assert [{k: v for k, v in i.items() if k not in ("ferr", "berr")} for i in both] == [dict(i) for i in F.infos]
        e = _errors(x, xt)
        for j, i in enumerate(both):
            print(f"{case} {dt} col {j}: error {e[j]:.3e} ferr {i['ferr']:.3e} berr {i['berr']:.3e} err_est {i['err_est']:.3e}")
            assert i["ferr"] >= e[j] and np.isfinite(i["ferr"]) and np.isfinite(i["berr"]) and i["berr"] >= 0


def test_with_bounds_host():
    _with_bounds("cpu")


@pytest.mark.gpu
def test_with_bounds_gpu():
    _with_bounds("cuda")


def test_trans_is_refused():
    case = (96, .25, 16, 1)
    A, xt, b, _ = _system(*case[:2], case[3])
    F = _factored(case, "fp64", "cpu")
    g = gj.GaussJordan(block_size=16, device="cpu", residual="never")
    with pytest.raises(ValueError):
        F.solve(b, trans=True, precise=True)
    with pytest.raises(ValueError):
        gj.solve(A, b, block_size=16, trans=True, precise=True)
    with pytest.raises(ValueError):
        g.run(96, input=A, rhs=b, trans=True, precise=True)
    with pytest.raises(ValueError):
        F._eng.solve_rhs_block(np.ascontiguousarray(b), rows=np.ascontiguousarray(A), trans=True, precise=True)
    assert (_errors(F.solve(A.T @ xt, trans=True), xt) < 1e-6).all()  # trans alone still works


@pytest.mark.gpu
def test_trans_is_refused_gpu():
    case = (96, .25, 16, 1)
    A, xt, b, _ = _system(*case[:2], case[3])
    Ad = _dev(A, "cuda")
    with pytest.raises(ValueError):
        gj.GaussJordan(block_size=16).solve_resident(Ad, _dev(b, "cuda"), trans=True, precise=True)
    with pytest.raises(ValueError):
        gj.solve(Ad, _dev(b, "cuda"), block_size=16, trans=True, precise=True)
    x = gj.solve(Ad, _dev(b, "cuda"), block_size=16, precise=True)
    assert x.is_cuda and (_errors(_np(x), xt) <= 2.0 ** -52).all()


# ------------------------------------------------------------------ more than one rank
# (the look-ahead depth is fixed on both sides of a comparison between rank counts: the engine chooses it
# differently at p = 1 and p > 1, and the inverses then differ in their last bits)
_DEPTH = 1


def _run_ranks(case, dt, ranks, **kw):
    n, dens, m, seed = case
    A, xt, b, _ = _system(n, dens, seed)
    g = gj.GaussJordan(block_size=m, ranks=ranks, device=kw.pop("device", "cpu"), dtype=dt, residual="never",
                       host_threads=1, **kw)
    rep = g.run(n, input=A, rhs=b, keep_solution=True, precise=True)
    assert rep["status"] == 0, rep["message"]
    return xt, rep


@pytest.mark.parametrize("case,dt", [((200, .15, 48, 5), "fp64"), ((96, .25, 16, 1), "fp64"), ((48, .25, 16, 3), "fp32")])
def test_three_loopback_ranks(case, dt):
    xt, one = _run_ranks(case, dt, 1, depth=_DEPTH)
    _, three = _run_ranks(case, dt, 3, comm="loopback", depth=_DEPTH)
    # the ranks hold rows of the same inverse and every row's sums run in the same order at any rank count
    assert np.array_equal(one["x"], three["x"]) and one["axb_columns"] == three["axb_columns"]
    assert (_errors(three["x"], xt) <= 2.0 ** -52).all() and all(c["converged"] for c in three["axb_columns"])
    assert all(c["err_est"] >= e for c, e in zip(three["axb_columns"], _errors(three["x"], xt)))


def test_schedule_checker_reports_nothing():
    case = (96, .25, 16, 1)
    xt, ref = _run_ranks(case, "fp64", 3, comm="loopback")
    _, rep = _run_ranks(case, "fp64", 3, comm="async", jitter_us=30.0, race_check=True)
    assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
    assert np.array_equal(rep["x"], ref["x"]) and rep["axb_columns"] == ref["axb_columns"]
    n, dens, m, seed = case
    A, _, b, _ = _system(n, dens, seed)
    g = gj.GaussJordan(block_size=m, ranks=3, device="cpu", residual="never", host_threads=1, comm="async",
                       race_check=True)
    both = g.run(n, input=A, rhs=b, keep_solution=True, precise=True, bounds=True)
    assert both["race_ops"] > 0 and both["race_count"] == 0, both["races"]


@pytest.mark.gpu
def test_gpu_ranks():
    """three ranks on one GPU (thread ranks): every rank's kernels, the norms made global"""
    case = (200, .15, 48, 5)
    xt, rep = _run_ranks(case, "fp64", 3, device="gpu", comm="async")
    assert (_errors(rep["x"], xt) <= 2.0 ** -52).all() and all(c["converged"] for c in rep["axb_columns"])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, case, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from mpi_jordan_crazy_acceleration_amd.parallel import DistributedGaussJordan

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n, dens, m, seed = case
        A, xt, b, _ = _system(n, dens, seed)
        d = DistributedGaussJordan(n, m, dtype="fp64", host_threads=1, depth=_DEPTH)
        d.load(A)
        st = d.solve()
        X, infos = d.solve_rhs(b, A_rows=A, precise=True)
        X0, infos0 = d.solve_rhs(b, A_rows=A)
        refused = False
        try:
            d.solve_rhs(b, A_rows=A, trans=True, precise=True)
        except ValueError:
            refused = True
        q.put((rank, st["status"], X, [dict(i) for i in infos], X0, [dict(i) for i in infos0], refused))
    finally:
        dist.destroy_process_group()


def test_gloo_ranks():
    import torch.multiprocessing as mp

    world, case = 3, (96, .25, 16, 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n, dens, m, seed = case
    A, xt, b, _ = _system(n, dens, seed)
    F = gj.factor(A, block_size=m, depth=_DEPTH)
    x1 = F.solve(b, precise=True)
    for rank, status, X, infos, X0, infos0, refused in res:
        assert status == 0 and refused
        assert np.array_equal(X, res[0][2]) and infos == res[0][3]  # the same on every rank
        assert np.array_equal(X, x1) and infos == [dict(i) for i in F.infos]  # and as one rank
        assert (_errors(X, xt) <= 2.0 ** -52).all() and all(i["converged"] for i in infos)
        assert all(k not in i for i in infos0 for k in NEW_KEYS)
        assert (_errors(X0, xt) >= 100 * 2.0 ** -52).all()


# ------------------------------------------------------------------ after a low-rank update
def _after_update(device):
    case = (128, .25, 32, 2)
    n = case[0]
    A, xt, _, _ = _system(*case[:2], case[3])
    rng = np.random.default_rng(9)
    Uu = rng.integers(-2, 3, (n, 2)).astype(np.float64)
    Vv = rng.integers(-2, 3, (n, 2)).astype(np.float64)
    A2 = A + Uu @ Vv.T  # exact
    b2 = A2 @ xt
    assert np.abs(b2).max() < 2 ** 50 and np.linalg.cond(A2, np.inf) >= 1e8
    F = gj.factor(_dev(A, device), block_size=case[2])
    F.update(Uu, Vv)
    x1 = _np(F.solve(_dev(b2, device), precise=True))
    assert all(i["converged"] for i in F.infos) and (_errors(x1, xt) <= 2.0 ** -52).all()
    assert all(i["err_est"] >= e for i, e in zip(F.infos, _errors(x1, xt)))
    x0 = _np(F.solve(_dev(b2, device)))
    assert (_errors(x0, xt) >= 100 * 2.0 ** -52).all()


def test_after_update_host():
    _after_update("cpu")


@pytest.mark.gpu
def test_after_update_gpu():
    _after_update("cuda")


# ------------------------------------------------------------------ the two CLIs
def _lines(out):
    return [l for l in out.splitlines() if not l.startswith("glob_time") and not l.startswith("[Gloo]")]


def _gj(gj_bin, *args, rc=0):
    p = subprocess.run([gj_bin, "--device", "cpu", *map(str, args)], capture_output=True, text=True, timeout=120)
    assert p.returncode == rc, p.stdout + p.stderr
    return p.stdout, p.stderr


def _pycli(*args, rc=0):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", MASTER_PORT=str(_free_port()), RANK="0",
               WORLD_SIZE="1", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "-m", "mpi_jordan_crazy_acceleration_amd.cli", "--device", "cpu",
                        *map(str, args)], cwd="/tmp", env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == rc, p.stdout + p.stderr
    return p.stdout, p.stderr


def _json(err):
    return json.loads([l for l in err.splitlines() if l.startswith("{")][-1])


def _same_but_residual(a, b):
    """stdout line by line, the value of the right-hand-side residual aside"""
    la, lb = _lines(a), _lines(b)
    assert len(la) == len(lb)
    for x, y in zip(la, lb):
        if x.startswith("Ax-b residual: "):
            assert y.startswith("Ax-b residual: ") and float(y.split()[-1]) >= 0
        else:
            assert x == y


def test_clis(gj_bin):
    base = ["--gen", "random", "--seed", 3, "--json", 77, 15]
    rhs = ["--rhs", "random", "--nrhs", 3]
    plain, plain_err = _gj(gj_bin, *rhs, *base)
    out, err = _gj(gj_bin, "--precise", *rhs, *base)
    _same_but_residual(plain, out)
    jp, jo = _json(plain_err), _json(err)
    assert {k for k in jo if k not in jp} == {"precise", "axb_dx_rel_cols", "axb_err_est_cols"}
    assert jo["precise"] is True and len(jo["axb_dx_rel_cols"]) == 3 and len(jo["axb_err_est_cols"]) == 3
    assert all(0 <= v <= U * 1.000001 for v in jo["axb_dx_rel_cols"]) and jo["refine_converged"] is True
    assert all(max(10, 77 ** .5) * U * 0.999999 <= v < 1e-10 for v in jo["axb_err_est_cols"])
    pout, perr = _pycli("--precise", *rhs, *base)
    assert "\n".join(_lines(out)) == "\n".join(_lines(pout))  # byte for byte, the time aside
    pj = _json(perr)
    assert pj["precise"] is True
    for key in ("axb_dx_rel_cols", "axb_err_est_cols"):
        assert np.allclose(jo[key], pj[key], rtol=1e-6, atol=0)  # (%.6e in build/gj)
    pplain, pplain_err = _pycli(*rhs, *base)
    _same_but_residual(pplain, pout)
    assert {k for k in pj if k not in _json(pplain_err)} == {"precise", "axb_dx_rel_cols", "axb_err_est_cols"}
    # one right-hand side: the block path as one column
    one, one_err = _gj(gj_bin, "--precise", "--rhs", "ones", *base)
    assert len(_json(one_err)["axb_err_est_cols"]) == 1
    # not with --trans: usage, exit 1
    _gj(gj_bin, "--precise", "--trans", *rhs, *base, rc=1)
    _pycli("--precise", "--trans", *rhs, *base, rc=1)
