"""The log-determinant of the factored matrix: Engine::slogdet (csrc/solver/engine.cpp) through
gj.factor(A).slogdet(), gj.slogdet / gj.det, GaussJordan.run(det=True), both CLIs' --det.

Every step's pivot block inverse H_t is kept (SolveOptions::track_det) and
det(A) = sgn(sigma)^m / prod_t det(H_t), sigma the block permutation of the pivots; Factored.update
multiplies by det(I + V^T inv(A) U).

Reference: numpy.linalg.slogdet in fp64.  The sign must be equal and |logabsdet - ref| <=
n * cond_inf(A) * eps, eps = 2^-52 for fp64 engines and 2^-23 for fp32 engines: the first-order bound
|tr(inv(A) E)| <= n ||inv(A)|| ||E|| for a backward error of one ulp per entry (derived, not measured).
A dropped, doubled or stale block moves the log by log|det H_t| = O(m), far outside it.
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
from mpi_jordan_crazy_acceleration_amd.models.gauss_jordan import SingularMatrixError
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}
SHAPES = [(240, 16), (250, 16), (75, 15), (77, 15), (40, 1), (10, 12)]
GENS = ["random", "randshift", "absdiff"]
SEED = 3


@functools.lru_cache(maxsize=None)
def _case(n, gen):
    """the matrix, numpy's slogdet of it and cond_inf (computed once per matrix)"""
    A = generate_matrix(n, gen, SEED)
    A.setflags(write=False)
    sign, logabs = np.linalg.slogdet(A)
    return A, float(sign), float(logabs), float(np.linalg.cond(A, np.inf))


def _ref(A):
    sign, logabs = np.linalg.slogdet(A)
    return float(sign), float(logabs), float(np.linalg.cond(A, np.inf))


def _check(got, sign, logabs, n, cond, dtype, what=""):
    bound = n * cond * EPS[dtype]
    err = abs(got[1] - logabs)
    print(f"{what} {dtype}: sign {got[0]:+.0f} (ref {sign:+.0f}), |dlog| = {err:.3e}, bound {bound:.3e}")
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert got[0] == sign, (got, sign, logabs)
    assert err <= bound, (err, bound)


def _uv(n, k):  # the update of tests/test_update_inverse.py
    rng = np.random.default_rng(11 + k)
    U = rng.standard_normal((n, k))
    V = rng.standard_normal((n, k))
    return U, V


# ------------------------------------------------------------------ one host rank against numpy
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_factor_slogdet_cpu(shape, gen, dtype):
    n, m = shape
    A, sign, logabs, cond = _case(n, gen)
    F = gj.factor(A, block_size=m, device="cpu", dtype=dtype)
    _check(F.slogdet(), sign, logabs, n, cond, dtype, f"n={n} m={m} {gen}")
    assert F.slogdet() == F.slogdet()  # cached


@pytest.mark.parametrize("shape,flips", [((77, 15), True), ((250, 16), False)], ids=["m15", "m16"])
def test_sign_of_the_block_permutation(shape, flips):
    """randshift with block rows 0 and 1 swapped: the pivots take them in the other order, an odd
    block permutation sigma, and det changes sign with it exactly when m is odd (sgn(sigma)^m)"""
    n, m = shape
    A, sign, logabs, cond = _case(n, "randshift")
    S = A.copy()
    S[:m], S[m:2 * m] = A[m:2 * m], A[:m]
    rep = gj.GaussJordan(block_size=m, device="cpu").run(n, input=S, det=True)
    piv = list(rep["stats"]["pivots"])
    seen, cycles = set(), 0
    for t in range(len(piv)):
        if t not in seen:
            cycles += 1
            while t not in seen:
                seen.add(t)
                t = piv[t]
    assert (len(piv) - cycles) % 2 == 1, piv  # precondition of this test: sigma is odd
    ssign, slog, scond = _ref(S)
    assert ssign == (-sign if flips else sign)  # (numpy agrees: m row swaps)
    _check(tuple(rep["slogdet"]), ssign, slog, n, scond, "fp64", f"swapped m={m}")
    got = gj.factor(A, block_size=m, device="cpu").slogdet()
    assert (tuple(rep["slogdet"])[0] == -got[0]) == flips


# ------------------------------------------------------------------ three loopback ranks
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("gen", ["random", "randshift"])
def test_three_ranks_agree(gen, dtype):
    n, m = 250, 16
    A, sign, logabs, cond = _case(n, gen)
    one = gj.GaussJordan(block_size=m, ranks=1, device="cpu", dtype=dtype).run(n, gen=gen, seed=SEED, det=True)
    rep = gj.GaussJordan(block_size=m, ranks=3, device="cpu", dtype=dtype, comm="loopback").run(
        n, gen=gen, seed=SEED, det=True)
    assert rep["status"] == 0 and one["status"] == 0
    _check(tuple(one["slogdet"]), sign, logabs, n, cond, dtype, "p=1")
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, dtype, "p=3")
    assert abs(rep["slogdet"][1] - one["slogdet"][1]) <= n * cond * EPS[dtype]
    ranks = np.asarray(rep["slogdet_ranks"])
    assert ranks.shape == (3, 2)
    for r in range(3):  # the same bits on every rank
        assert np.array_equal(ranks[r].view(np.uint64), ranks[0].view(np.uint64))
    assert list(ranks[0]) == list(rep["slogdet"])


@pytest.mark.parametrize("comm", ["loopback", "async"])
def test_three_ranks_race_check_clean(comm):
    n, m = 250, 16
    A, sign, logabs, cond = _case(n, "random")
    rep = gj.GaussJordan(block_size=m, ranks=3, device="cpu", comm=comm, race_check=True).run(
        n, gen="random", seed=SEED, det=True)
    assert rep["status"] == 0
    assert rep["race_count"] == 0, rep["races"][:5]
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, "fp64", comm)


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("comm", ["loopback", "async"])
def test_one_block_race_check_clean(comm, ranks):
    """n <= m: one pivot block (Nr = 1), so the two outputs are two doubles and the partial sums that
    go through the all-reduce need room of their own; ranks 1 and 2 of three own no step at all"""
    n, m = 10, 12
    A, sign, logabs, cond = _case(n, "random")
    rep = gj.GaussJordan(block_size=m, ranks=ranks, device="cpu", comm=comm, race_check=True).run(
        n, gen="random", seed=SEED, det=True)
    assert rep["status"] == 0
    assert rep["race_count"] == 0, rep["races"][:5]
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, "fp64", f"Nr=1 {comm} p={ranks}")
    ranks_ = np.asarray(rep["slogdet_ranks"])
    assert all(np.array_equal(r.view(np.uint64), ranks_[0].view(np.uint64)) for r in ranks_)


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("opts", [dict(depth=1), dict(depth=2), dict(depth=4), dict(pivot="partial")],
                         ids=["d1", "d2", "d4", "partial"])
def test_depths_and_pivot_rule(opts, ranks):
    n, m = 250, 16
    A, sign, logabs, cond = _case(n, "random")
    rep = gj.GaussJordan(block_size=m, ranks=ranks, device="cpu", comm="loopback" if ranks > 1 else "auto",
                         **opts).run(n, gen="random", seed=SEED, det=True)
    assert rep["status"] == 0
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, "fp64", str(opts))


# ------------------------------------------------------------------ after updates
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_slogdet_follows_update(k, dtype):
    n, m = 240, 16
    A = _case(n, "randshift")[0]
    U, V = _uv(n, k)
    A2 = A + U @ V.T
    F = gj.factor(A, block_size=m, device="cpu", dtype=dtype)
    F.update(U, V)  # (the determinant of A is taken from the stash before the panel moves on)
    sign, logabs, cond = _ref(A2)
    _check(F.slogdet(), sign, logabs, n, cond, dtype, f"k={k}")
    # and once more on top, the value asked for in between
    U2, V2 = _uv(n, 3)
    F.update(U2, V2)
    A3 = A2 + U2 @ V2.T
    sign, logabs, cond = _ref(A3)
    _check(F.slogdet(), sign, logabs, n, cond, dtype, f"k={k}+3")


@pytest.mark.parametrize("ranks", [1, 3])
def test_run_reports_the_determinant_after_the_update(ranks):
    n, m = 240, 16
    A = _case(n, "randshift")[0]
    U, V = _uv(n, 5)
    rep = gj.GaussJordan(block_size=m, ranks=ranks, device="cpu", comm="loopback" if ranks > 1 else "auto").run(
        n, gen="randshift", seed=SEED, update=(U, V), det=True)
    assert rep["status"] == 0 and rep["update"]["k"] == 5
    sign, logabs, cond = _ref(A + U @ V.T)
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, "fp64", f"run(update=, det=) p={ranks}")
    ranks_ = np.asarray(rep["slogdet_ranks"])
    assert all(np.array_equal(r.view(np.uint64), ranks_[0].view(np.uint64)) for r in ranks_)


def test_update_keys_and_engine_fields():
    n, m = 240, 16
    A = _case(n, "randshift")[0]
    U, V = _uv(n, 5)
    F = gj.factor(A, block_size=m, device="cpu")
    s0, l0 = F.slogdet()
    assert set(F.update(U, V)) == {"k", "min_pivot", "cond1", "seconds"}
    G = gj.factor(A, block_size=m, device="cpu")
    info = G._eng.update_inverse(U, V)
    sc, lc = np.linalg.slogdet(np.eye(5) + V.T @ np.linalg.solve(A, U))
    assert info["sign_c"] == sc and abs(info["logabsdet_c"] - lc) <= 1e-10
    s1, l1 = F.slogdet()
    assert s1 == s0 * sc and abs(l1 - (l0 + lc)) <= 1e-10


def test_refused_update_leaves_the_determinant():
    n = 64
    F = gj.factor(2.0 * np.eye(n), block_size=16, device="cpu")
    before = F.slogdet()
    assert before[0] == 1.0 and abs(before[1] - n * np.log(2.0)) <= n * EPS["fp64"]
    e0 = np.zeros(n)
    e0[0] = 1.0
    with pytest.raises(SingularMatrixError):
        F.update(-2.0 * e0, e0)  # C = 1 + e0^T (I / 2) (-2 e0) = 0
    after = F.slogdet()
    assert np.array_equal(np.array(after).view(np.uint64), np.array(before).view(np.uint64))
    # ... also when the determinant had not been asked for before the refusal
    G = gj.factor(2.0 * np.eye(n), block_size=16, device="cpu")
    with pytest.raises(SingularMatrixError):
        G.update(-2.0 * e0, e0)
    assert np.array_equal(np.array(G.slogdet()).view(np.uint64), np.array(before).view(np.uint64))
    F.update(e0, e0)  # diag(3, 2, ...)
    s, l = F.slogdet()
    assert s == 1.0 and abs(l - (np.log(3.0) + (n - 1) * np.log(2.0))) <= n * EPS["fp64"]


# ------------------------------------------------------------------ convenience functions
def test_slogdet_of_a_singular_matrix():
    A = np.random.default_rng(0).standard_normal((12, 12))
    A[7] = A[3]
    assert gj.slogdet(A, block_size=4, device="cpu") == (0.0, -np.inf)
    assert gj.det(A, block_size=4, device="cpu") == 0.0
    assert gj.slogdet(np.zeros((5, 5)), device="cpu") == (0.0, -np.inf)


def test_det_small():
    A = np.random.default_rng(1).standard_normal((10, 10))
    d = gj.det(A, device="cpu")
    ref = np.linalg.det(A)
    assert isinstance(d, float) and abs(d - ref) <= 1e-12 * abs(ref)
    assert gj.slogdet(A, device="cpu")[0] == np.sign(ref)
    T = torch.from_numpy(A)
    assert gj.det(T, device="cpu") == d and gj.factor(T, device="cpu").det() == d


def test_det_overflows_like_numpy():
    A = 1e10 * np.eye(40)
    assert gj.det(A, block_size=8, device="cpu") == np.inf
    A[0, 0] = -1e10
    assert gj.det(A, block_size=8, device="cpu") == -np.inf
    s, l = gj.slogdet(A, block_size=8, device="cpu")
    assert s == -1.0 and abs(l - 40 * np.log(1e10)) <= 1e-10


# ------------------------------------------------------------------ off is off
@pytest.mark.parametrize("ranks", [1, 3])
def test_tracking_does_not_change_the_inverse(ranks):
    n, m = 250, 16
    A = _case(n, "random")[0]
    kw = dict(block_size=m, device="cpu", ranks=ranks, comm="loopback" if ranks > 1 else "auto")
    off = gj.inverse(A, **kw)
    on = gj.inverse(A, det=True, **kw)
    assert np.array_equal(off.view(np.uint64), on.view(np.uint64))


def test_engine_without_tracking_refuses():
    C = gj.load_native()
    eng = C.Engine(C.host_device(1), C.self_comm(), 40, 8, "fp64")
    eng.generate("randshift", SEED)
    assert eng.solve()["status"] == 0
    assert eng.slogdet()["status"] == 5  # BadArgs
    on = C.Engine(C.host_device(1), C.self_comm(), 40, 8, "fp64", track_det=True)
    on.generate("randshift", SEED)
    assert on.slogdet()["status"] == 5  # before solve()
    assert on.solve()["status"] == 0
    d = on.slogdet()
    A, sign, logabs, cond = _case(40, "randshift")
    assert d["status"] == 0
    _check((d["sign"], d["logabsdet"]), sign, logabs, 40, cond, "fp64", "engine")
    on.generate("random", SEED)  # a new input: the old value is gone with the old inverse
    assert on.solve()["status"] == 0
    A, sign, logabs, cond = _case(40, "random")
    d = on.slogdet()
    _check((d["sign"], d["logabsdet"]), sign, logabs, 40, cond, "fp64", "engine, second solve")


# ------------------------------------------------------------------ the two CLIs
def _lines(out):
    return [l for l in out.splitlines() if not l.startswith("glob_time") and not l.startswith("[Gloo]")]


def _gj(gj_bin, *args):
    p = subprocess.run([gj_bin, "--device", "cpu", *map(str, args)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout, p.stderr


def _pycli(*args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "-m", "mpi_jordan_crazy_acceleration_amd.cli", "--device", "cpu",
                        *map(str, args)], cwd="/tmp", env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout, p.stderr


def _json(err):
    return json.loads([l for l in err.splitlines() if l.startswith("{")][-1])


def test_cli_det_adds_one_line(gj_bin):
    n, m = 77, 15
    args = ["--gen", "random", "--seed", SEED, "--json", n, m]
    A, sign, logabs, cond = _case(n, "random")
    plain, plain_err = _gj(gj_bin, *args)
    with_det, det_err = _gj(gj_bin, "--det", *args)
    a, b = _lines(plain), _lines(with_det)
    extra = [l for l in b if l.startswith("slogdet: ")]
    assert len(extra) == 1 and not any(l.startswith("slogdet") for l in a)
    assert [l for l in b if l is not extra[0]] == a  # nothing else moved
    assert b.index(extra[0]) == [i for i, l in enumerate(b) if l.startswith("residual: ")][0] + 1
    tag, s, l = extra[0].split()
    assert s == f"{int(sign):d}"
    _check((float(s), float(l)), sign, logabs, n, cond, "fp64", "build/gj")
    assert "slogdet" not in _json(plain_err)
    jd = _json(det_err)
    assert jd["slogdet"] == [float(s), float(l)]
    assert {k for k in jd if k != "slogdet"} == set(_json(plain_err))
    # the module CLI: the same line, character for character, and nothing without the flag
    py_plain, py_plain_err = _pycli(*args)
    py_det, py_det_err = _pycli("--det", *args)
    pa, pb = _lines(py_plain), _lines(py_det)
    assert [l for l in pb if l.startswith("slogdet")] == extra
    assert [l for l in pb if not l.startswith("slogdet")] == pa
    assert pb.index(extra[0]) == [i for i, l in enumerate(pb) if l.startswith("residual: ")][0] + 1
    assert "slogdet" not in _json(py_plain_err) and _json(py_det_err)["slogdet"] == jd["slogdet"]


def test_module_cli_det_three_processes():
    """DistributedGaussJordan(det=True).slogdet() over gloo: three processes, each with a third of the
    pivot blocks, agree on the sum (rank 0 prints it)"""
    n, m = 77, 15
    A, sign, logabs, cond = _case(n, "random")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", "--master-port", str(port), "--local-ranks-filter", "0", "-m",
           "mpi_jordan_crazy_acceleration_amd.cli", "--device", "cpu", "--det", "--gen", "random", "--seed",
           str(SEED), str(n), str(m)]
    p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("slogdet: ")]
    assert len(line) == 1, p.stdout
    _check((float(line[0].split()[1]), float(line[0].split()[2])), sign, logabs, n, cond, "fp64", "gloo p=3")


# ------------------------------------------------------------------ GPU
GPU_SHAPES = [(240, 16), (250, 16), (40, 1), (517, 60), (300, 256), (1000, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("gen", ["random", "randshift"])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_factor_slogdet_gpu(shape, gen, dtype):
    n, m = shape
    A, sign, logabs, cond = _case(n, gen)
    F = gj.factor(torch.tensor(A, device="cuda"), block_size=m, dtype=dtype)
    _check(F.slogdet(), sign, logabs, n, cond, dtype, f"gpu n={n} m={m} {gen}")
    assert gj.load_native().last_slogdet_kernel() == \
        f"sld:{'lds' if m <= 128 else 'glob'}:{'f64' if dtype == 'fp64' else 'f32'}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_slogdet_follows_update_gpu(dtype):
    n, m, k = 240, 16, 5
    A = _case(n, "randshift")[0]
    U, V = _uv(n, k)
    F = gj.factor(torch.tensor(A, device="cuda"), block_size=m, dtype=dtype)
    F.update(torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda())
    sign, logabs, cond = _ref(A + U @ V.T)
    _check(F.slogdet(), sign, logabs, n, cond, dtype, "gpu k=5")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_three_ranks_gpu(dtype):
    n, m = 250, 16
    A, sign, logabs, cond = _case(n, "random")
    rep = gj.GaussJordan(block_size=m, ranks=3, device="gpu", comm="loopback", dtype=dtype).run(
        n, gen="random", seed=SEED, det=True)
    assert rep["status"] == 0
    _check(tuple(rep["slogdet"]), sign, logabs, n, cond, dtype, "gpu p=3")
    ranks = np.asarray(rep["slogdet_ranks"])
    for r in range(3):
        assert np.array_equal(ranks[r].view(np.uint64), ranks[0].view(np.uint64))


@pytest.mark.gpu
def test_tracking_does_not_change_the_inverse_gpu():
    n, m = 517, 60
    A = torch.tensor(_case(n, "random")[0], device="cuda")
    off = gj.inverse(A, block_size=m)
    on = gj.inverse(A, block_size=m, det=True)
    assert torch.equal(off.view(torch.int64), on.view(torch.int64))
