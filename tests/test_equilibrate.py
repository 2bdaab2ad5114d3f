"""Power-of-two equilibration ahead of the sweep (SolveOptions::equilibrate) through every layer:
gj.inverse / gj.factor / GaussJordan.run, DistributedGaussJordan over gloo, both CLIs, on the host
executor and (gpu-marked twins) on CUDA tensors.

The rule, re-implemented here in numpy (_rule): rexp[i] = 1 - frexp(max_j |A[i][j]|).exponent (0 for a
maximum that is 0 or not finite), cexp[j] by the same rule from the column maxima of ldexp(|A|, rexp[i]),
As = ldexp(A, rexp[i] + cexp[j]) is what the sweep inverts and inv(A)[i][j] = ldexp(Y[i][j], cexp[i] +
rexp[j]).  Scaling by powers of two is exact, so the equilibrated inverse must equal, bit for bit, the
plain inverse of As with the exponents undone -- the test that pins the whole path.

Inputs: B = randshift(n, seed 3) (cond_inf about 1e2) with every third row times 2^-60, every fifth
column times 2^-60, rows and columns times 2^(-40 .. 40), and B times 2^-70 as a whole.  The plain sweep
calls all of them singular (its tests are absolute in ||A||_inf); that is the premise, asserted.

Bounds, derived, not measured:
    inverse   ||As Ys - I||_inf <= 2 n ||As|| ||Ys|| eps   (utils/metrics.py residual_bound, on the
              scaled pair, where the residual means something: Ys = ldexp(X, -(cexp[i] + rexp[j])))
    solves    every column within 1e-8 of np.linalg.solve, relative to the column's max
              (test_update_inverse.py's tolerance), and converged
    slogdet   sign equal; |dlog| <= n cond_inf(As) eps_dtype + 4 * 2^-52 (|log|det As|| + ln2 |sum exp|):
              test_slogdet.py's first-order bound on the matrix the sweep saw, plus the roundings of
              forming ln2 * sum, the subtraction and numpy's own sum of that size
"""
import functools
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.models.gauss_jordan import SingularMatrixError
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
from mpi_jordan_crazy_acceleration_amd.utils.metrics import residual_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GJ = os.path.join(ROOT, "build", "gj")
SHAPES = [(96, 16), (200, 64), (300, 128)]
PATTERNS = ["rows", "cols", "both", "tiny"]
EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}
_ND = {"fp64": np.float64, "fp32": np.float32}
LN2 = float(np.log(2.0))


def _exponents(amax):
    e = np.zeros(amax.shape, np.int32)
    ok = (amax > 0) & np.isfinite(amax)
    e[ok] = 1 - np.frexp(amax[ok])[1]
    return e


def _rule(A):
    """(rexp, cexp, As) of the matrix as the engine holds it (fp64 values)"""
    r = _exponents(np.abs(A).max(axis=1))
    c = _exponents(np.ldexp(np.abs(A), r[:, None]).max(axis=0))
    return r, c, np.ldexp(A, r[:, None] + c[None, :])


def _undo(Y, r, c, dtype="fp64"):
    return np.ldexp(Y, c[:, None] + r[None, :]).astype(_ND[dtype]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _bad(n, pattern, span=40):
    B = generate_matrix(n, "randshift", 3)
    i = np.arange(n)
    if pattern == "rows":
        A = np.ldexp(B, np.where(i % 3 == 0, -60, 0)[:, None])
    elif pattern == "cols":
        A = np.ldexp(B, np.where(i % 5 == 0, -60, 0)[None, :])
    elif pattern == "both":
        rng = np.random.default_rng([5, n, span])
        A = np.ldexp(B, rng.integers(-span, span + 1, n)[:, None] + rng.integers(-span, span + 1, n)[None, :])
    else:
        A = np.ldexp(B, -70)
    A.setflags(write=False)
    return A


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float64).view(np.int64),
                                                 np.asarray(b, np.float64).view(np.int64))


def _check_inverse(A, X, dtype="fp64"):
    r, c, As = _rule(A.astype(_ND[dtype]).astype(np.float64))
    Ys = np.ldexp(X, -(c[:, None] + r[None, :]))
    n = A.shape[0]
    res = np.abs(As @ Ys - np.eye(n)).sum(axis=1).max()
    bound = residual_bound(n, np.abs(As).sum(axis=1).max(), np.abs(Ys).sum(axis=1).max(), dtype)
    print(f"n={n} {dtype}: scaled residual {res:.3e}, bound {bound:.3e}")
    assert np.isfinite(X).all() and res <= bound, (res, bound)


# ------------------------------------------------------------------ singular without, right with
def _singular_without_right_with(n, m, pattern, to_dev):
    A = _bad(n, pattern)
    with pytest.raises(SingularMatrixError):
        gj.inverse(to_dev(A), block_size=m)
    X = gj.inverse(to_dev(A), block_size=m, equilibrate=True)
    _check_inverse(A, X.cpu().numpy() if isinstance(X, torch.Tensor) else X)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_singular_without_right_with_host(shape, pattern):
    _singular_without_right_with(*shape, pattern, lambda a: a)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_singular_without_right_with_gpu(shape, pattern):
    _singular_without_right_with(*shape, pattern, lambda a: torch.from_numpy(a.copy()).cuda())


# ------------------------------------------------------------------ bitwise identity with an explicit run
def _identity(n, m, dtype, pattern, **kw):
    """run(A, equilibrate) == undo(run(As)) bit for bit, the report says what was applied"""
    A = _bad(n, pattern, span=40 if dtype == "fp64" else 20)
    r, c, As = _rule(A.astype(_ND[dtype]).astype(np.float64))
    assert r.any() or c.any()
    g = dict(block_size=m, dtype=dtype, residual="never", **kw)
    rep = gj.GaussJordan(equilibrate=True, **g).run(n, input=A, keep_inverse=True)
    ref = gj.GaussJordan(**g).run(n, input=As, keep_inverse=True)
    assert rep["status"] == 0 and ref["status"] == 0, (rep["message"], ref["message"])
    assert _bits_equal(rep["inverse"], _undo(ref["inverse"], r, c, dtype))
    q = rep["equilibrate"]
    assert q["applied"] is True and "equilibrate" not in ref
    assert tuple(q["row_exp_range"]) == (r.min(), r.max()) and tuple(q["col_exp_range"]) == (c.min(), c.max())
    _check_inverse(A, rep["inverse"], dtype)


_ID_CASES = [(96, 16, "fp64", "both"), (200, 64, "fp32", "both"), (300, 128, "fp64", "rows"),
             (300, 128, "fp32", "both"), (200, 64, "fp64", "cols")]


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("case", _ID_CASES, ids=lambda c: f"n{c[0]}-m{c[1]}-{c[2]}-{c[3]}")
def test_bitwise_identity_host(case, ranks):
    _identity(*case, ranks=ranks, device="cpu", host_threads=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("case", _ID_CASES, ids=lambda c: f"n{c[0]}-m{c[1]}-{c[2]}-{c[3]}")
def test_bitwise_identity_gpu(case, ranks):
    _identity(*case, ranks=ranks, device="gpu", comm="auto" if ranks == 1 else "async")


def _resident_identity(dtype):
    # the CUDA-tensor path (upload device-to-device, the engine's own dtype conversion)
    n, m = 300, 128
    A = _bad(n, "both", span=40 if dtype == "fp64" else 20)
    tdt = torch.float64 if dtype == "fp64" else torch.float32
    At = torch.from_numpy(A.copy()).cuda().to(tdt)
    r, c, As = _rule(At.double().cpu().numpy())
    X = gj.inverse(At, block_size=m, dtype=dtype, equilibrate=True)
    Y = gj.inverse(torch.from_numpy(As).cuda().to(tdt), block_size=m, dtype=dtype)
    assert X.dtype == tdt and _bits_equal(X.double().cpu().numpy(), _undo(Y.double().cpu().numpy(), r, c, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_bitwise_identity_resident_gpu(dtype):
    _resident_identity(dtype)


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
        A = _bad(n, "both")
        r, c, As = _rule(A)
        out = {}
        for name, M, eq in (("eq", A, True), ("ref", As, False)):
            s = DistributedGaussJordan(n, m, host_threads=1, equilibrate=eq, det=True)
            s.load(M)
            st = s.solve()
            out[name] = (st["status"], s.gather_inverse(), s.equilibration, s.slogdet(), st.get("equilibrate"))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_bitwise_identity_gloo_ranks():
    world, n, m = 2, 96, 16
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, n, m, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    r, c, As = _rule(_bad(n, "both"))
    for rank in range(world):
        (s1, X, e1, d1, q1), (s0, Y, e0, d0, q0) = res[rank]["eq"], res[rank]["ref"]
        assert s1 == 0 and s0 == 0 and e0 is None and q0 is None
        assert e1["applied"] and np.array_equal(e1["row_exp"], r) and np.array_equal(e1["col_exp"], c)
        assert e1["row_exp"].dtype == np.int32 and q1["applied"]
        assert d1 == res[0]["eq"][3]  # the same bits on every rank
        assert d1[0] == d0[0] and abs(d1[1] - (d0[1] - LN2 * (int(r.sum()) + int(c.sum())))) <= 4 * 2.0 ** -52 * (
            abs(d0[1]) + LN2 * abs(int(r.sum()) + int(c.sum())))
    X, Y = res[0]["eq"][1], res[0]["ref"][1]  # (gathered on rank 0)
    assert _bits_equal(X, _undo(Y, r, c))


# ------------------------------------------------------------------ the handle: exponents, skip, solves, det
def _to_cpu(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _exponents_case(to_dev):
    for (n, m), pattern in zip(SHAPES, ("both", "rows", "cols")):
        A = _bad(n, pattern)
        r, c, _ = _rule(A)
        q = gj.factor(to_dev(A), block_size=m, equilibrate=True).equilibration
        assert q["applied"] is True
        for got, want in ((q["row_exp"], r), (q["col_exp"], c)):
            assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)


def test_exponents_host():
    _exponents_case(lambda a: a)


@pytest.mark.gpu
def test_exponents_gpu():
    _exponents_case(lambda a: torch.from_numpy(a.copy()).cuda())


def _skip_case(to_dev):
    for (n, m), div in zip(SHAPES, (8, 8, 16)):
        A = generate_matrix(n, "randshift", 3) / div
        r, c, _ = _rule(A)
        assert not r.any() and not c.any()  # the premise: nothing to scale
        F = gj.factor(to_dev(A), block_size=m, equilibrate=True)
        q = F.equilibration
        assert q["applied"] is False and not q["row_exp"].any() and not q["col_exp"].any()
        plain = gj.factor(to_dev(A), block_size=m)
        assert plain.equilibration is None
        assert _bits_equal(_to_cpu(F.inverse()), _to_cpu(plain.inverse()))
        assert F.slogdet() == plain.slogdet()


def test_skip_case_host():
    _skip_case(lambda a: a)


@pytest.mark.gpu
def test_skip_case_gpu():
    _skip_case(lambda a: torch.from_numpy(a.copy()).cuda())


def _close_cols(X, ref, what):
    err = np.abs(X - ref).max(axis=0) / np.abs(ref).max(axis=0)
    print(f"{what}: max relative column error {err.max():.3e}")
    assert (err < 1e-8).all(), (what, err)


def _det_bound(As, sum_exp, dtype="fp64"):
    _, logabs_s = np.linalg.slogdet(As)
    return As.shape[0] * np.linalg.cond(As, np.inf) * EPS[dtype] + 4 * 2.0 ** -52 * (abs(logabs_s) + LN2 * abs(sum_exp))


def _handle_case(n, m, pattern, to_dev):
    A = _bad(n, pattern)
    r, c, As = _rule(A)
    sum_exp = int(r.sum()) + int(c.sum())
    rng = np.random.default_rng([9, n])
    F = gj.factor(to_dev(A), block_size=m, equilibrate=True)

    def solves(M, what):
        b = rng.standard_normal((n, 3))
        cc = rng.standard_normal((n, 3))
        X = _to_cpu(F.solve(to_dev(b)))
        assert len(F.infos) == 3 and all(i["converged"] for i in F.infos), F.infos
        _close_cols(X, np.linalg.solve(M, b), what + " solve")
        Xt = _to_cpu(F.solve(to_dev(cc), trans=True))
        assert len(F.infos) == 3 and all(i["converged"] for i in F.infos), F.infos
        _close_cols(Xt, np.linalg.solve(M.T, cc), what + " trans solve")

    def det(M, Ms, what):
        sign, logabs = np.linalg.slogdet(M)
        got = F.slogdet()
        bound = _det_bound(Ms, sum_exp)
        print(f"{what}: sign {got[0]:+.0f} (ref {sign:+.0f}), |dlog| = {abs(got[1] - logabs):.3e}, bound {bound:.3e}")
        assert got[0] == sign and abs(got[1] - logabs) <= bound

    solves(A, f"n={n} {pattern}")
    det(A, As, f"n={n} {pattern}")
    # one update, of the scaled matrix's own size: As + 0.1 U0 V0^T in the scaled picture
    U = np.ldexp(0.1 * rng.standard_normal((n, 2)), -r[:, None])
    V = np.ldexp(rng.standard_normal((n, 2)), -c[:, None])
    F.update(to_dev(U), to_dev(V))
    A2 = A + U @ V.T
    det(A2, np.ldexp(A2, r[:, None] + c[None, :]), f"n={n} {pattern} updated")
    solves(A2, f"n={n} {pattern} updated")


_HANDLE = [(96, 16, "rows"), (200, 64, "cols"), (300, 128, "both"), (200, 64, "tiny")]


@pytest.mark.parametrize("case", _HANDLE, ids=lambda c: f"n{c[0]}-m{c[1]}-{c[2]}")
def test_handle_host(case):
    _handle_case(*case, lambda a: a)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _HANDLE, ids=lambda c: f"n{c[0]}-m{c[1]}-{c[2]}")
def test_handle_gpu(case):
    _handle_case(*case, lambda a: torch.from_numpy(np.array(a)).cuda())


def test_conveniences_host():
    # gj.solve / gj.slogdet / gj.det take the option; a singular answer without it
    n, m = 96, 16
    A = _bad(n, "rows")
    r, c, As = _rule(A)
    b = A @ np.ones(n)
    with pytest.raises(SingularMatrixError):
        gj.solve(A, b, block_size=m)
    _close_cols(gj.solve(A, b, block_size=m, equilibrate=True).reshape(n, 1), np.ones((n, 1)), "gj.solve")
    assert gj.slogdet(A, block_size=m) == (0.0, float("-inf"))
    sign, logabs = np.linalg.slogdet(A)
    got = gj.slogdet(A, block_size=m, equilibrate=True)
    assert got[0] == sign and abs(got[1] - logabs) <= _det_bound(As, int(r.sum()) + int(c.sum()))
    assert gj.det(A, block_size=m, equilibrate=True) == float(got[0] * np.exp(got[1]))


# ------------------------------------------------------------------ in-process runs under the schedule checker
@pytest.mark.parametrize("ranks", [1, 3])
def test_run_race_check_host(ranks):
    n, m = 96, 16
    A = _bad(n, "both")
    rep = gj.run(n, m, ranks=ranks, device="cpu", input=A, equilibrate=True, race_check=True,
                 comm="async" if ranks > 1 else "auto")
    assert rep["status"] == 0, rep["message"]
    assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
    assert rep["equilibrate"]["applied"] is True
    X = np.linalg.inv(A)
    assert rep["residual"] <= residual_bound(n, np.abs(A).sum(axis=1).max(), np.abs(X).sum(axis=1).max())
    assert gj.run(n, m, ranks=ranks, device="cpu", input=A)["status"] == 1


@pytest.mark.gpu
def test_run_race_check_gpu():
    n, m = 300, 128
    A = _bad(n, "both")
    rep = gj.run(n, m, ranks=3, device="gpu", input=A, equilibrate=True, race_check=True, comm="async")
    assert rep["status"] == 0, rep["message"]
    assert rep["race_ops"] > 0 and rep["race_count"] == 0, rep["races"]
    assert rep["equilibrate"]["applied"] is True


# ------------------------------------------------------------------ CLIs
def _mask_time(out):
    return re.sub(r"glob_time: \d+\.\d\d", "glob_time: #", out)


def _files(tmp_path):
    n = 40
    bad = np.array(_bad(n, "rows"))
    good = generate_matrix(n, "randshift", 3) / 4
    r, c, _ = _rule(good)
    assert not r.any() and not c.any()  # well scaled: the option has nothing to do
    fb, fg = tmp_path / "bad.txt", tmp_path / "good.txt"
    np.savetxt(fb, bad, fmt="%.17g")
    np.savetxt(fg, good, fmt="%.17g")
    X = np.linalg.inv(bad)
    tol = residual_bound(n, np.abs(bad).sum(axis=1).max(), np.abs(X).sum(axis=1).max())
    return n, fb, fg, tol


def test_cli_binary(tmp_path):
    n, fb, fg, tol = _files(tmp_path)
    run = lambda *a: subprocess.run([GJ, "--device", "cpu", "-p", "2", *map(str, a)], capture_output=True, text=True,
                                    timeout=120)
    r = run(n, 8, fb)
    assert r.returncode == 2 and r.stdout.endswith("singular matrix\n")
    q = run("--equilibrate", "--json", "--check-residual", f"{float(tol):.17g}", n, 8, fb)
    assert q.returncode == 0, (q.stdout, q.stderr)
    assert q.stdout.startswith(r.stdout[:-len("singular matrix\n")])  # the A corner: the matrix as given
    assert re.search(r"^residual: \d\.\d{6}e[+-]\d\d$", q.stdout, re.M)
    rec = json.loads(q.stderr.strip().splitlines()[-1])
    assert rec["equilibrate"]["applied"] is True and rec["equilibrate"]["row_exp_range"][1] >= 57
    a, b = run(n, 8, fg), run("--equilibrate", n, 8, fg)
    assert a.returncode == 0 and b.returncode == 0 and _mask_time(a.stdout) == _mask_time(b.stdout)


def _torchrun(nproc, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "--local-ranks-filter", "0",
           "-m", "mpi_jordan_crazy_acceleration_amd.cli", "--device", "cpu", *map(str, args)]
    return subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=180)


def _lines(out):
    return "\n".join(l for l in out.splitlines() if not l.startswith("[Gloo]"))


def test_cli_module(tmp_path):
    n, fb, fg, tol = _files(tmp_path)
    r = _torchrun(2, n, 8, fb)
    assert r.returncode != 0 and _lines(r.stdout).endswith("singular matrix")
    q = _torchrun(2, "--equilibrate", "--json", n, 8, fb)
    assert q.returncode == 0, (q.stdout, q.stderr[-3000:])
    out = _lines(q.stdout)
    assert out.startswith(_lines(r.stdout)[:-len("singular matrix")])
    res = float(re.search(r"^residual: (\S+)$", out, re.M).group(1))
    assert np.isfinite(res) and res <= tol, (res, tol)
    rec = [json.loads(l) for l in q.stderr.splitlines() if l.startswith("{") and '"equilibrate"' in l][-1]
    assert rec["equilibrate"]["applied"] is True
    a, b = _torchrun(2, n, 8, fg), _torchrun(2, "--equilibrate", n, 8, fg)
    assert a.returncode == 0 and b.returncode == 0 and _mask_time(_lines(a.stdout)) == _mask_time(_lines(b.stdout))


# ------------------------------------------------------------------ option off
def test_option_off_host():
    C = gj.load_native()
    n, m = 96, 16
    A = generate_matrix(n, "randshift", 3)
    eng = C.Engine(C.host_device(1), C.self_comm(), n, m, equilibrate=False)
    assert eng.equil_exponents() is None
    eng.upload_local_rows(A)
    st = eng.solve()
    assert st["status"] == 0 and "equilibrate" not in st
    assert gj.factor(A, block_size=m).equilibration is None
    assert "equilibrate" not in gj.run(n, m, device="cpu", input=A)


@pytest.mark.gpu
def test_option_off_memory_gpu():
    # an engine built with equilibrate=False holds exactly what one at the defaults holds
    C = gj.load_native()
    n, m = 1024, 128
    dev = C.hip_device(0)

    def held(**kw):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        eng = C.Engine(dev, C.self_comm(), n, m, **kw)
        after = torch.cuda.mem_get_info()[0]
        assert eng.equil_exponents() is None or kw.get("equilibrate")
        del eng
        return before - after

    held()  # (the device's own first-use allocations)
    base = held()
    assert held(equilibrate=False) == base
    assert held(equilibrate=True) >= base
