"""Host code under AddressSanitizer + UBSan: engine, loopback ranks, reader, CLI.

GPU sanitizers are not available on this platform; the device code is exercised by the GPU tests."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_BIN = os.path.join(ROOT, "build", "gj_asan")


@pytest.fixture(scope="module")
def asan_bin():
    r = subprocess.run(["make", "-j8", "asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("asan build failed:\n" + r.stderr[-3000:])
    return ASAN_BIN


def _run(binary, *args, env_extra=None, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", **(env_extra or {}))
    p = subprocess.run([binary, "--device", "cpu", *map(str, args)], capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "ERROR: LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "runtime error:" not in p.stderr, p.stderr[-4000:]
    return p


@pytest.mark.parametrize("args", [
    ("-p", 3, "--depth", 4, 200, 16),
    ("-p", 4, "--depth", 2, "--chunk-cols", 32, 150, 7),
    ("--gen", "random", "--rhs", "random", "--profile", "--json", 300, 64),
    ("-p", 5, 33, 10),            # more ranks than some block rows
    ("--dtype", "fp32", "-p", 2, 96, 12),
    ("-p", 3, "--gen", "randshift", "--rhs", "random", "--nrhs", 5, 200, 16),             # block solve
    ("-p", 3, "--gen", "randshift", "--rhs", "random", "--nrhs", 3, "--trans", 100, 12),  # A^T, ragged last block
])
def test_asan_cli_runs(asan_bin, args):
    p = _run(asan_bin, *args)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "residual:" in p.stdout


def test_asan_file_and_errors(asan_bin, tmp_path):
    f = tmp_path / "a.txt"
    np.savetxt(f, np.random.default_rng(0).standard_normal((50, 50)), fmt="%.17g")
    assert _run(asan_bin, "-p", 2, 50, 8, f).returncode == 0
    short = tmp_path / "s.txt"
    short.write_text("1 2 3")
    assert _run(asan_bin, 50, 8, short).returncode == 2
    z = tmp_path / "z.txt"
    z.write_text("0 0 0 0")
    assert _run(asan_bin, "-p", 2, 2, 1, z).returncode == 2  # singular


INJECTED = "injected (GJ_TEST_ALLOC_NTH)"


def _alloc_sweep(binary, args, limit=1000):
    """GJ_TEST_ALLOC_NTH=n for n = 1, 2, ... until a run ends with status 0 and the injection has not
    fired.  Returns (the n of that run or None, the number of runs that exited 2 with the injected
    message, [(n, what was wrong with that run)])."""
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    injected, bad = 0, []
    for n in range(1, limit + 1):
        env["GJ_TEST_ALLOC_NTH"] = str(n)
        try:
            p = subprocess.run([binary, "--device", "cpu", *map(str, args)], capture_output=True, text=True,
                               timeout=120, env=env)
        except subprocess.TimeoutExpired:
            bad.append((n, "did not end"))
            continue
        fired = INJECTED in p.stderr or INJECTED in p.stdout
        for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"):
            if mark in p.stderr:
                bad.append((n, mark))
        if p.returncode not in (0, 2):
            bad.append((n, "exit status %d" % p.returncode))
        if p.returncode == 2 and fired:
            injected += 1
        if p.returncode == 0 and not fired:
            return n, injected, bad
    return None, injected, bad


# Every allocation of a one-rank run fails in turn: each run ends by itself with status 0 or 2 and
# loses nothing (LeakSanitizer sees the host executor's blocks), whichever allocation it was.
@pytest.mark.parametrize("args", [
    # the one-vector path and its upload_vector / local_matvec temporaries
    ("--gen", "randshift", "--rhs", "random", "--refine", 3, 64, 8),
    # the block driver, the fp64 staging of A and the widened residual
    ("--dtype", "fp32", "--gen", "randshift", "--rhs", "random", "--nrhs", 3, "--trans", 40, 8),
    # every optional work buffer
    ("--pivot", "partial", "--det", "--equilibrate", 40, 8),
])
def test_asan_alloc_failure_sweep(asan_bin, args):
    clean, injected, bad = _alloc_sweep(asan_bin, args)
    print("clean run at n = %s, %d runs exited 2 with the injected message, %d findings" % (clean, injected, len(bad)))
    assert not bad, "%d runs: %s" % (len({n for n, _ in bad}), bad[:40])
    assert clean is not None, "no clean run within 1000 values of n"
    assert injected >= 30, injected  # alloc_work alone makes more allocations than that


# The constructor refuses GJ_SPLIT=3 after the matrix panels and the work space were allocated.
@pytest.mark.parametrize("args", [(64, 8), ("-p", 3, 64, 8)])
def test_asan_constructor_throw(asan_bin, args):
    p = _run(asan_bin, *args, env_extra={"GJ_SPLIT": "3"}, timeout=120)
    assert p.returncode != 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "GJ_SPLIT" in p.stderr
