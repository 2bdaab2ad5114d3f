"""Every size-selected engine policy at test sizes, bit-compared with the small shape's own.

Engine::plan_policy picks depth, CU reservation, trailing-update build and tile, the launch merges and
the chain's latency kernels from the problem size, and every other GPU engine test (n <= 9000) runs one
corner of it.  GJ_POLICY_LIKE=<n>x<p> gives a 2048- or 4096-order engine the policy of the shapes the
project is measured by (tests/test_policy_plan.py pins the table).  Each corner is compared with a
baseline: the same n, m, p, depth, chunk plan and matrix without the variable.

  * policy: every rank of the corner reports the big shape's planned switches, every rank of the
    baseline the small shape's;
  * census (native.gemm_census): the corner launched the kernel family it is about and the baseline
    did not -- a corner whose launches are the baseline's tested nothing.  Two rows of the table
    select the very switches their small shape selects: 8192x1 (the tests' own corner) and 32768x8
    (4096 rows on 8 ranks is already a reserved, dense, depth-8-capable rank; the row differs from
    its small shape in the automatic depth alone, which both runs are given explicitly).  For these
    the planner itself says that no launch may differ, and the census must then hold the same names;
  * pivots: the baseline's and the numpy oracle's (gauss_jordan_reference through physical_pivots);
  * inverse: the baseline's bits.  Every fp64 family accumulates v_mfma_f64_16x16x4 over ascending k
    per output element; the switches change tiles, staging, streams, masks and launch splits only;
  * the baseline itself: max|inv - numpy inv| / max|numpy inv| < 1e-8, test_gpu_engine.py's criterion
    (fp32, on random + sqrt(n) I: 1e-4, test_engine_large_blocks' bound for that dtype and matrix).

Multi-rank cases run on stream-ordered virtual ranks of one GPU with jittered arrivals and the
consumption-point hash verification (GJ_VERIFY) on."""
import numpy as np
import pytest

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.utils import gauss_jordan_reference, generate_matrix, physical_pivots

pytestmark = pytest.mark.gpu

SWITCHES = ("depth", "reserve_cus", "dense_gemm", "gemm_tile", "skip_cols", "chunk_skip", "lat_reg", "lat_wide")

T128 = "glds64:t128"           # the 128-wide fp64 LDS-DMA tile, any build (launch_glds)
DENSE = "glds64:t64:b25:peel"  # the 5-per-CU build of the 64-wide tile (GemmExtra::dense)
LAT = ("lat64", "batch:lat")   # gemm_lat_f64 and its batched form, the register-fed latency tile (GemmExtra::lat_reg)

# like, n, m, p, depth, chunk_cols, dtype, generator
ROWS = [
    ("8192x1", 2048, 128, 1, 2, 512, "fp64", "random"),
    ("16384x1", 2048, 128, 1, 4, 512, "fp64", "random"),
    ("32768x1", 2048, 128, 1, 4, 512, "fp64", "random"),
    ("32768x2", 2048, 128, 2, 4, 512, "fp64", "random"),
    ("32768x4", 2048, 128, 4, 4, 512, "fp64", "random"),
    ("32768x8", 4096, 128, 8, 8, 512, "fp64", "random"),
    ("65536x1", 4096, 128, 1, 4, 2048, "fp32", "randshift"),
    # the headline corner with 384-column panels (m = 96: every look-ahead range starts on a multiple
    # of 384 = 3 * 128 columns, so MAIN still takes one launch around it), with 320-column panels
    # (m = 80, chunks of 12 + 4 blocks: the look-ahead columns [320, 640) and [640, 960) of the first
    # chunk do not both sit on the 128-column tile grid, so MAIN takes one launch per side of them, on
    # the unmasked stream), and with a ragged last block row (2000 = 15 * 128 + 80)
    ("32768x1", 1536, 96, 1, 4, 512, "fp64", "random"),
    ("32768x1", 1280, 80, 1, 4, 960, "fp64", "random"),
    ("32768x1", 2000, 128, 1, 4, 512, "fp64", "random"),
]

_CACHE = {}


def _matrix(n, gen, dtype):
    key = ("A", n, gen, dtype)
    if key not in _CACHE:
        A = generate_matrix(n, gen, 21)
        if gen == "random":
            A = A[::-1].copy()  # forces off-diagonal pivots
        if dtype == "fp32":
            A = A.astype(np.float32).astype(np.float64)  # what the fp32 engine sees, exactly
        A.setflags(write=False)
        _CACHE[key] = A
    return _CACHE[key]


def _numpy_inverse(n, gen, dtype):
    key = ("inv", n, gen, dtype)
    if key not in _CACHE:
        _CACHE[key] = np.linalg.inv(_matrix(n, gen, dtype))
    return _CACHE[key]


def _oracle_pivots(n, m, gen, dtype):
    """The numpy oracle's physical pivot sequence, once per matrix and block size.  Every step's winner
    is clear of the runner-up (asserted, _pivot_oracle.py's margin), so no step is a tie and the
    sequence is that of gauss_jordan_reference(A, m, p) at every p: p enters its rule through ties alone."""
    key = ("piv", n, m, gen, dtype)
    if key not in _CACHE:
        _, piv, gaps = gauss_jordan_reference(_matrix(n, gen, dtype), m, 1, return_gaps=True)
        assert min(gaps) >= 1e-3, gaps
        _CACHE[key] = physical_pivots(piv)
    return _CACHE[key]


def _solve(native, monkeypatch, like, n, m, p, depth, chunk_cols, dtype, gen, race_check=False):
    """one run_local solve with the launch census around it: (report, census)"""
    if like:
        monkeypatch.setenv("GJ_POLICY_LIKE", like)
    else:
        monkeypatch.delenv("GJ_POLICY_LIKE", raising=False)
    if p > 1:
        monkeypatch.setenv("GJ_VERIFY", "1")
    eng = gj.GaussJordan(block_size=m, ranks=p, device="gpu", dtype=dtype, comm="async" if p > 1 else "auto",
                         jitter_us=30.0 if p > 1 else 0.0, depth=depth, chunk_cols=chunk_cols, race_check=race_check)
    native.gemm_census(True)
    try:
        rep = eng.run(n, input=_matrix(n, gen, dtype), keep_inverse=True)
    finally:
        native.gemm_census(False)
    assert rep["status"] == 0, rep["message"]
    return rep, native.gemm_census_counts()


def _baseline(native, monkeypatch, n, m, p, depth, chunk_cols, dtype, gen):
    key = ("base", n, m, p, depth, chunk_cols, dtype, gen)
    if key not in _CACHE:
        _CACHE[key] = _solve(native, monkeypatch, None, n, m, p, depth, chunk_cols, dtype, gen)
    return _CACHE[key]


def _switches(pol):
    return {k: pol[k] for k in SWITCHES}


def _has(census, name):
    return any(name in k for k in census)


def _lat(census):
    return any(k in census for k in LAT)


@pytest.mark.parametrize("like,n,m,p,depth,chunk_cols,dtype,gen", ROWS,
                         ids=["%s-n%d-m%d-%s" % (r[0], r[1], r[2], r[6]) for r in ROWS])
def test_corner_matches_its_baseline(native, monkeypatch, like, n, m, p, depth, chunk_cols, dtype, gen):
    base, base_census = _baseline(native, monkeypatch, n, m, p, depth, chunk_cols, dtype, gen)
    got, census = _solve(native, monkeypatch, like, n, m, p, depth, chunk_cols, dtype, gen)
    print("census", like, n, m, dict(census), "baseline", dict(base_census))

    # policy: the big shape's on every rank of the corner, the small shape's on every rank of the baseline
    ln, lp = (int(v) for v in like.split("x"))
    differs = False
    for r in range(p):
        big = native.plan_policy(ln, m, lp, min(r, lp - 1), dtype, on_gpu=True, depth=depth)
        small = native.plan_policy(n, m, p, r, dtype, on_gpu=True, depth=depth, chunk_cols=chunk_cols)
        assert _switches(got["policy_ranks"][r]) == _switches(big), (r, got["policy_ranks"][r])
        assert _switches(base["policy_ranks"][r]) == _switches(small), (r, base["policy_ranks"][r])
        assert "GJ_POLICY_LIKE=" + like in got["policy_ranks"][r]["env_overrides"]
        assert not any(v.startswith("GJ_POLICY_LIKE") for v in base["policy_ranks"][r]["env_overrides"])
        for k in ("nchunks", "chunk_cols", "first_depth"):  # the chunk plan is the engine's own
            assert got["policy_ranks"][r][k] == base["policy_ranks"][r][k] == small[k], k
        differs = differs or _switches(big) != _switches(small)
    big = native.plan_policy(ln, m, lp, 0, dtype, on_gpu=True, depth=depth)
    small = native.plan_policy(n, m, p, 0, dtype, on_gpu=True, depth=depth, chunk_cols=chunk_cols)
    if m == 128 and dtype == "fp64":
        assert got["policy_ranks"][0]["nchunks"] == 4  # like the headline

    # census: the family the corner is about, absent from the baseline
    if dtype == "fp32":
        assert "glds32:t256" in census and "glds32:t256" not in base_census, (census, base_census)
        assert "glds32:t128" in base_census, base_census
    elif big["gemm_tile"] == 128:
        assert _has(census, T128) and not _has(base_census, T128), (census, base_census)
    if big["dense_gemm"]:
        assert DENSE in census, census
    else:
        assert DENSE not in census, census
    if not big["lat_reg"]:
        assert not _lat(census), census
    if dtype == "fp64":
        assert (DENSE in base_census) == small["dense_gemm"], base_census
        assert _lat(base_census) == small["lat_reg"], base_census
    if differs:
        assert dict(census) != dict(base_census), "the corner launched what its baseline launched: %r" % (census,)
    else:
        assert sorted(census) == sorted(base_census), (census, base_census)

    # pivots: the baseline's, and the fp64 oracle's (the fp32 case compares the two runs alone, as the
    # tile pair it is about differs in nothing a pivot search sees)
    assert list(got["stats"]["pivots"]) == list(base["stats"]["pivots"]), like
    if dtype == "fp64":
        assert list(base["stats"]["pivots"]) == _oracle_pivots(n, m, gen, dtype)
        assert base["stats"]["offdiag_pivots"] > 0

    # the baseline's accuracy, then the corner's bits
    ref = _numpy_inverse(n, gen, dtype)
    rel = np.abs(base["inverse"] - ref).max() / np.abs(ref).max()
    print("baseline error", like, n, m, rel)
    assert rel < (1e-8 if dtype == "fp64" else 1e-4), rel
    same = np.array_equal(got["inverse"], base["inverse"])
    assert same, "corner %s differs from its baseline: max |diff| %.3e, corner error vs numpy %.3e" % (
        like, np.abs(got["inverse"] - base["inverse"]).max(), np.abs(got["inverse"] - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("like,p", [("32768x1", 1), ("32768x4", 4)])
def test_corner_race_check(native, monkeypatch, like, p):
    """The unmasked corners under the happens-before schedule checker, as test_race_check_on_gpu runs the
    reserved one: the op sequence of an unreserved MAIN stream (one launch per chunk around the
    look-ahead columns at 32768x1, one per side at 32768x4, two chunk-pass launches, the chain on the
    small register-staged tile) has no unordered conflicting access, and the wrapped run gives the
    baseline's bits."""
    n, m, depth, cc = 2048, 128, 4, 512
    base, _ = _baseline(native, monkeypatch, n, m, p, depth, cc, "fp64", "random")
    rep, _ = _solve(native, monkeypatch, like, n, m, p, depth, cc, "fp64", "random", race_check=True)
    ln, lp = (int(v) for v in like.split("x"))
    for r in range(p):
        big = native.plan_policy(ln, m, lp, min(r, lp - 1), "fp64", on_gpu=True, depth=depth)
        assert _switches(rep["policy_ranks"][r]) == _switches(big)
    assert rep["race_ops"] > 0
    assert rep["race_count"] == 0, "\n".join(rep["races"])
    assert np.array_equal(rep["inverse"], base["inverse"])
