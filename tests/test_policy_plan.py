"""The size-selected engine policy as a pure function (Engine::plan_policy), and GJ_POLICY_LIKE.

The constructor picks panel depth, CU reservation, trailing-update build and tile, the launch merges
(skip_cols, chunk_skip), the chain's latency kernels (lat_reg, lat_wide) and the chunk plan from the
problem's shape.  Here the table of those choices for the shapes the project is measured by is pinned
key by key (README "Size-selected policies" shows the same table), the planner is compared with what
an engine on the host executor reports, and GJ_POLICY_LIKE=<n>x<p> -- a small engine with a large
problem's policy -- is checked on the host executor: reported, validated, overridable, and without
effect on a single bit of the inverse."""
import os
import re

import numpy as np
import pytest

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix

SWITCHES = ("depth", "reserve_cus", "dense_gemm", "gemm_tile", "skip_cols", "chunk_skip", "lat_reg", "lat_wide")
KEYS = SWITCHES + ("nchunks",)

# (n, p, dtype): depth, reserved CUs, dense, tile, skip_cols, chunk_skip, lat_reg, lat_wide, chunks
TABLE = {
    (8192, 1, "fp64"): (2, 32, False, 64, True, True, True, True, 2),
    (16384, 1, "fp64"): (4, 32, True, 64, True, True, True, False, 2),
    (32768, 1, "fp64"): (4, 0, False, 128, True, False, False, False, 4),
    (32768, 2, "fp64"): (4, 0, False, 128, True, False, False, False, 4),
    (32768, 4, "fp64"): (4, 0, False, 64, False, False, False, False, 4),
    (32768, 8, "fp64"): (8, 32, True, 64, True, True, True, False, 4),
    (65536, 1, "fp32"): (4, 0, False, 128, True, False, False, False, 8),
}


def expected(n, p, dtype):
    return dict(zip(KEYS, TABLE[(n, p, dtype)]))


# the table at m = 128, and its fp64 rows at m = 256
ROWS = [k + (128,) for k in TABLE] + [k + (256,) for k in TABLE if k[2] == "fp64"]


@pytest.mark.parametrize("n,p,dtype,m", ROWS, ids=["%dx%d-%s-m%d" % k for k in ROWS])
def test_planned_policy_table(native, n, p, dtype, m):
    """Every rank of the shape gets the row.  The thresholds are on rows and columns, not on blocks, so
    m = 256 gives the same rows (the chunk count too: 8192-column chunks of 32 blocks, a multiple of
    every depth here)."""
    for rank in sorted({0, p - 1}):
        got = native.plan_policy(n, m, p, rank, dtype, on_gpu=True)
        assert {k: got[k] for k in KEYS} == expected(n, p, dtype), (rank, got)
        assert got["reserve_request"] == got["reserve_cus"] and got["first_depth"] == got["depth"]
        assert got["chunk_begin"][0] == 0 and got["chunk_end"][-1] == n // m
        assert got["chunk_begin"][1:] == got["chunk_end"][:-1]
        assert got["chunk_cols"] == max(e - b for b, e in zip(got["chunk_begin"], got["chunk_end"])) * m


def test_readme_table_is_this_table():
    """the README's "Size-selected policies" table, row by row, is TABLE"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "README.md"), encoding="utf-8") as f:
        text = f.read().split("### Size-selected policies", 1)[1]
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in text.splitlines()
            if line.startswith("| N ")]
    assert len(rows) == len(TABLE)

    def cell(c):
        return {"yes": True, "no": False}[c] if c in ("yes", "no") else int(re.match(r"\d+", c).group())

    for row, want in zip(rows, TABLE.values()):
        assert tuple(cell(c) for c in row[1:]) == want, row


def test_small_corner_below_the_thresholds(native):
    """What every GPU engine test up to n = 9000 runs: the first row's switches at p = 1 up to 8192, and
    depth 4 / no lat_wide from 8193 padded columns or at p > 1"""
    for n in (2048, 4096, 8192):
        got = native.plan_policy(n, 128, 1, 0, "fp64", on_gpu=True)
        assert {k: got[k] for k in SWITCHES} == {k: expected(8192, 1, "fp64")[k] for k in SWITCHES}
    for n, p in ((9000, 1), (2048, 2), (2048, 8)):
        got = native.plan_policy(n, 128, p, 0, "fp64", on_gpu=True)
        assert (got["depth"], got["reserve_cus"], got["dense_gemm"], got["gemm_tile"], got["lat_wide"]) == \
            (4, 32, True, 64, False), (n, p, got)


def test_grant_decides_the_switches(native):
    """the switches follow the CUs the device really set aside, not the request"""
    asked = native.plan_policy(8192, 128, 1, 0, "fp64", on_gpu=True, granted_cus=0)
    assert asked["reserve_request"] == 32 and asked["reserve_cus"] == 0
    assert not (asked["dense_gemm"] or asked["skip_cols"] or asked["chunk_skip"] or asked["lat_reg"] or asked["lat_wide"])
    forced = native.plan_policy(32768, 128, 1, 0, "fp64", on_gpu=True, reserve_cus=16)
    assert forced["reserve_cus"] == 16 and forced["dense_gemm"] and forced["gemm_tile"] == 64 and forced["lat_reg"]


GRID = [(n, m, p) for n in (64, 600, 2048, 9000) for m in (8, 64, 128) for p in (1, 3, 8)]


@pytest.mark.parametrize("n,m,p", GRID, ids=["%d-%d-%d" % c for c in GRID])
def test_planner_equals_host_engine_policy(native, monkeypatch, n, m, p):
    """plan_policy(on_gpu=False) against the policy of rank 0's engine on the host executor (p > 1: the
    one-rank stand-in of a p-rank job), automatic and explicit depth, automatic and explicit chunk
    width; the chunk boundaries are checked through their count and the widest chunk"""
    for var in ("GJ_POLICY_LIKE", "GJ_RESERVE_CUS", "GJ_CHUNK_PLAN", "GJ_FIRST_DEPTH"):
        monkeypatch.delenv(var, raising=False)
    for depth in (0, 1, 3, 8):
        for cc in (0, 512):
            comm = native.self_comm() if p == 1 else native.shadow_comm(p)
            pol = native.Engine(native.host_device(1), comm, n, m, "fp64", cc, 1e-15, False, depth).policy
            plan = native.plan_policy(n, m, p, 0, "fp64", on_gpu=False, depth=depth, chunk_cols=cc)
            for k in KEYS + ("chunk_cols", "first_depth"):
                assert pol[k] == plan[k], (k, depth, cc, pol, plan)


def _host_engine(native, n=64, m=8, **kw):
    return native.Engine(native.host_device(1), native.self_comm(), n, m, "fp64", **kw)


def test_policy_like_reported_and_overridable(native, monkeypatch):
    monkeypatch.delenv("GJ_POLICY_LIKE", raising=False)
    plain = _host_engine(native).policy
    assert (plain["depth"], plain["gemm_tile"], plain["skip_cols"]) == (2, 64, False)
    monkeypatch.setenv("GJ_POLICY_LIKE", "32768x1")
    pol = _host_engine(native).policy
    assert "GJ_POLICY_LIKE=32768x1" in pol["env_overrides"]
    big = native.plan_policy(32768, 8, 1, 0, "fp64", on_gpu=False)
    assert {k: pol[k] for k in SWITCHES} == {k: big[k] for k in SWITCHES}
    assert (pol["depth"], pol["gemm_tile"], pol["skip_cols"]) == (4, 128, True)
    # the chunk plan stays this engine's own: 64 columns at depth 4
    own = native.plan_policy(64, 8, 1, 0, "fp64", on_gpu=False, depth=4)
    assert (pol["nchunks"], pol["chunk_cols"]) == (own["nchunks"], own["chunk_cols"])
    # min(depth, Nr) from the engine's own layout: 3 block columns
    assert _host_engine(native, n=24).policy["depth"] == 3
    # an explicit depth and the individual overrides still win
    assert _host_engine(native, depth=1).policy["depth"] == 1
    monkeypatch.setenv("GJ_SKIP_COLS", "0")
    pol = _host_engine(native).policy
    assert pol["skip_cols"] is False and pol["gemm_tile"] == 128
    # the rank index is clamped: rank 0 of 32768x8 is a small rank (depth 8)
    monkeypatch.setenv("GJ_POLICY_LIKE", "32768x8")
    assert _host_engine(native, n=128).policy["depth"] == 8


@pytest.mark.parametrize("bad", ["", "32768", "32768x", "x8", "32768x0", "0x1", "-4x2", "32768x1x", "32768 x 1", "1e4x1",
                                 "32768X1"])
def test_policy_like_malformed_is_bad_args(native, monkeypatch, bad):
    monkeypatch.setenv("GJ_POLICY_LIKE", bad)
    with pytest.raises(native.GJError, match="GJ_POLICY_LIKE") as e:
        _host_engine(native)
    assert e.value.status == 5  # Status::BadArgs


_A = {}


def _run(p, depth, race_check=False):
    n, m = 200, 8
    if "A" not in _A:
        _A["A"] = generate_matrix(n, "random", 21)[::-1].copy()
    eng = gj.GaussJordan(block_size=m, ranks=p, device="cpu", comm="async", depth=depth, jitter_us=300.0,
                         host_threads=1, chunk_cols=64, race_check=race_check, extra=dict(verify=True))
    rep = eng.run(n, input=_A["A"], keep_inverse=True)
    assert rep["status"] == 0, rep["message"]
    return rep


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("like,depth", [("32768x1", 4), ("32768x8", 8)])
def test_policy_like_host_runs_bit_identical(native, monkeypatch, like, depth, p):
    """n = 200, m = 8 on jittered asynchronous host ranks with the host plan of a 32768-order problem
    (32768x1: the wide tile's one-launch MAIN update around the look-ahead columns; 32768x8: depth 8)
    against the same depth and chunk plan without it: the same bits, the same pivots, and no race."""
    monkeypatch.delenv("GJ_POLICY_LIKE", raising=False)
    base = _run(p, depth)
    monkeypatch.setenv("GJ_POLICY_LIKE", like)
    got = _run(p, depth)
    checked = _run(p, depth, race_check=True)
    ln, lp = (int(v) for v in like.split("x"))
    for r in range(p):
        big = native.plan_policy(ln, 8, lp, min(r, lp - 1), "fp64", on_gpu=False, depth=depth)
        small = native.plan_policy(200, 8, p, r, "fp64", on_gpu=False, depth=depth, chunk_cols=64)
        assert {k: got["policy_ranks"][r][k] for k in SWITCHES} == {k: big[k] for k in SWITCHES}
        assert {k: base["policy_ranks"][r][k] for k in SWITCHES} == {k: small[k] for k in SWITCHES}
        for k in ("depth", "nchunks", "chunk_cols"):
            assert got["policy_ranks"][r][k] == base["policy_ranks"][r][k] == small[k]
    assert list(got["stats"]["pivots"]) == list(base["stats"]["pivots"])
    assert np.array_equal(got["inverse"], base["inverse"])
    assert np.array_equal(checked["inverse"], base["inverse"])
    assert checked["race_ops"] > 0 and checked["race_count"] == 0, "\n".join(checked["races"])
    # test_verify.py's criterion for this shape
    assert np.abs(_A["A"] @ base["inverse"] - np.eye(200)).sum(1).max() < 1e-9
