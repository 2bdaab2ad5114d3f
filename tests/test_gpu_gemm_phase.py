"""The fp64 LDS-DMA trailing-update kernel's tile-uniform fast path.

A full tile that every input mask covers entirely or not at all loads and stores C without
per-element compares (and issues no C load where it enters as 0).  That may not change a bit: every
case is compared bit for bit with the same call on the masked path -- a separately strided c_in
always takes it -- on both tile widths, and with a numpy fp64 product at test_gpu_kernels.py's
tolerance (1e-12 K for operands in [-1, 1]).  No priority variant of the kernel was kept
(profiles/gemm_phase.md), so there is none to run here."""
import itertools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops
from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix

pytestmark = pytest.mark.gpu

TILES = {64: "glds64:t64:b33:peel", 128: "glds64:t128:b23:peel"}
# one trip, a K tail, the peeled steady state; one tile, several, ragged edges
SHAPES = list(itertools.product((128, 384, 300), (128, 384, 200), (8, 40, 512)))
SENT = 7.0  # what a skipped column holds before and after


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


_OPERANDS = {}


def _operands(Mp, N, K):
    """(A^T, B, C) on the device for a physical height Mp, computed once per shape and never written"""
    key = (Mp, N, K)
    if key not in _OPERANDS:
        _OPERANDS[key] = (_rand((K, Mp), 1).cuda(), _rand((K, N), 2).cuda(), _rand((Mp, N), 3).cuda())
    return _OPERANDS[key]


def _case(M, N, K, zr=(), zh=0, zc=(0, 0), skip=(0, 0), tcols=None, rsel=None, op="acc"):
    """the stored input of one call (NaN under every input mask, SENT in the skipped columns) and
    its fp64 reference"""
    Mp = 384 if rsel else M
    At, B, C0 = _operands(Mp, N, K)
    rows = np.arange(Mp) if not rsel else np.concatenate([np.arange(b * rsel[1], (b + 1) * rsel[1]) for b in rsel[0]])
    Cin = C0.clone()
    eff = C0.cpu().numpy().copy()
    if op == "store":
        Cin[:] = float("nan")
        eff[:] = 0.0
    for r in zr:
        Cin[max(r, 0):r + zh] = float("nan")
        eff[max(r, 0):r + zh] = 0.0
    Cin[:, zc[0]:zc[1]] = float("nan")
    eff[:, zc[0]:zc[1]] = 0.0
    Cin[:, skip[0]:skip[1]] = SENT
    ref = eff + At.cpu().numpy().T @ B.cpu().numpy()
    ref[:, skip[0]:skip[1]] = SENT
    if rsel:  # the unselected row blocks are neither read nor written
        un = np.setdiff1d(np.arange(Mp), rows)
        Cin[torch.as_tensor(un, device=Cin.device)] = SENT
        ref[un] = SENT
    kw = dict(op=op, a_kmajor=True, zero_rows=zr, zero_row_height=zh, zero_cols=zc, skip_cols=skip)
    if rsel:
        kw["row_blocks"], kw["row_block_m"] = rsel
    return dict(At=At, B=B, Cin=Cin, ref=ref, kw=kw, tcols=tcols, K=K, Mp=Mp, N=N, written=rows, skip=skip)


def _call(c, native, tile, c_nt=3, general=False):
    """(C, -C^T) of one launch; general: the accumulator input through a separately strided c_in"""
    Cin = c["Cin"]
    kw = dict(c["kw"], glds_tile=tile, c_nt=c_nt)
    T = None
    if c["tcols"]:
        T = torch.full((c["tcols"], c["Mp"]), SENT, dtype=torch.float64, device="cuda")
        kw["tneg"] = T
    if general:
        wide = torch.full((c["Mp"], c["N"] + 24), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :c["N"]] = Cin
        C = torch.full_like(Cin, SENT)
        kw["c_in"] = wide[:, :c["N"]]
    else:
        C = Cin.clone()
    ops.gemm(c["At"], c["B"], C, **kw)
    assert native.last_gemm_kernel() == TILES[tile], native.last_gemm_kernel()
    return C, T


def _same(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _check(c, native, c_nts=(3,), store_ref=None):
    """every fast-path candidate against the masked path's bits, and against numpy"""
    refC, refT = store_ref if store_ref is not None else _call(c, native, 128, general=True)
    err = np.abs(refC.cpu().numpy() - c["ref"]).max()
    assert err < 1e-12 * c["K"], err
    if refT is not None:
        s0, s1 = c["skip"]
        keep = [j for j in range(c["tcols"]) if not (s0 <= j < s1)]
        rows = torch.as_tensor(c["written"], device="cuda")
        assert torch.equal(refT[keep][:, rows], -refC[rows][:, keep].t())
    for tile, c_nt in itertools.product(TILES, c_nts):
        C, T = _call(c, native, tile, c_nt)
        assert _same(C, refC), (tile, c_nt, float((C - refC).abs().max()))
        if refT is not None:
            assert _same(T, refT), (tile, c_nt)
    if store_ref is None and c["kw"]["op"] == "acc":  # the 64-wide tile's masked path: a second reference
        C, T = _call(c, native, 64, general=True)
        assert _same(C, refC) and (refT is None or _same(T, refT))


def _mid(n):  # the first row / column of a middle (or the only) 128-wide tile
    return 128 if n > 128 else 0


@pytest.mark.parametrize("mask", ["none", "rows-aligned", "rows-off64", "cols-aligned", "cols-off16", "rows-and-cols",
                                  "skip-middle", "store"])
def test_uniform_tiles_match_the_masked_path(mask, native):
    for M, N, K in SHAPES:
        zr, zh, zc, skip, op = (), 0, (0, 0), (0, 0), "acc"
        if mask in ("rows-aligned", "rows-and-cols"):
            zr, zh = (_mid(M),), 128
        if mask == "rows-off64":
            zr, zh = (64,), 128
        if mask in ("cols-aligned", "rows-and-cols"):
            zc = (_mid(N), _mid(N) + 128)
        if mask == "cols-off16":
            zc = (16, 144)
        if mask == "skip-middle":
            skip = (_mid(N), _mid(N) + 128)
        if mask == "store":
            op = "store"
        c = _case(M, N, K, zr=zr, zh=zh, zc=(zc[0], min(zc[1], N)), skip=skip, op=op)  # (skip: whole tiles)
        if mask == "store":  # C = A B is C += A B with every column entering as 0, there on the masked path
            a = _case(M, N, K, zc=(0, N))
            _check(c, native, store_ref=_call(a, native, 128, general=True))
        else:
            _check(c, native)


@pytest.mark.parametrize("cover", ["all", "none-of-later-tiles", "half"])
def test_neg_transpose_bound_on_a_tile(cover, native):
    """-C^T of the columns < tneg_cols: the bound past a tile, before it, and through its middle"""
    for M, N, K in SHAPES:
        tcols = N if cover == "all" else min(128, N) if cover == "none-of-later-tiles" else 64
        _check(_case(M, N, K, tcols=tcols), native)
        _check(_case(M, N, K, tcols=tcols, zr=(_mid(M),), zh=128, zc=(0, min(128, N))), native)


def test_cache_policy_bits(native):
    """c_nt 0..3 on the unmasked and the zeroed tiles"""
    for M, N, K in ((384, 384, 40), (300, 200, 512)):
        _check(_case(M, N, K), native, c_nts=(0, 1, 2, 3))
        _check(_case(M, N, K, zr=(128,), zh=128, zc=(128, N)), native, c_nts=(0, 1, 2, 3))


def test_row_selection_keeps_the_masked_path(native):
    """two of three 128-row blocks (GemmExtra::rsel)"""
    for N, K in itertools.product((128, 384, 200), (8, 40, 512)):
        _check(_case(256, N, K, rsel=([0, 2], 128)), native)
        _check(_case(256, N, K, rsel=([0, 2], 128), zr=(256,), zh=128, tcols=min(N, 128)), native)


def test_strided_c_in_matches_in_place(native):
    """c_in with its own leading dimension on both tile widths against the in-place call"""
    for M, N, K in SHAPES:
        c = _case(M, N, K, zc=(0, min(128, N)))
        ref, _ = _call(c, native, 128)
        for tile in TILES:
            assert _same(_call(c, native, tile, general=True)[0], ref), (M, N, K, tile)


# (tile, build): the kernel launch_glds names for it.  Build 25 is the dense (5-per-CU) build, which
# exists on the 64-wide tile only; 32 on the 128-wide one only.
BUILDS = {(64, 23): "glds64:t64:b23:peel", (64, 33): "glds64:t64:b33:peel", (64, 25): "glds64:t64:b25:peel",
          (128, 23): "glds64:t128:b23:peel", (128, 33): "glds64:t128:b33:peel", (128, 32): "glds64:t128:b32:peel"}


@pytest.mark.parametrize("M,N,K", [(384, 384, 40), (300, 200, 512)])
def test_builds_agree_bit_for_bit(M, N, K, native):
    """Every LDS-DMA build of both tile widths on one call with a zero row block and zero columns: the
    stage count, the register bound and the tile width may not change a bit (each output element is the
    same ascending-k chain of v_mfma_f64_16x16x4), which is what lets an engine's inverse be compared
    across the policies that pick these builds (tests/test_gpu_policy_corners.py)."""
    c = _case(M, N, K, zr=(128,), zh=128, zc=(16, 144))
    out = {}
    for (tile, build), name in BUILDS.items():
        C = c["Cin"].clone()
        kw = dict(c["kw"], glds_tile=tile, c_nt=3)
        if build == 25:
            kw["dense"] = True
        else:
            kw["glds_build"] = build
        ops.gemm(c["At"], c["B"], C, **kw)
        assert native.last_gemm_kernel() == name, (tile, build, native.last_gemm_kernel())
        out[(tile, build)] = C
    first = out[(64, 23)]
    err = np.abs(first.cpu().numpy() - c["ref"]).max()
    assert err < 1e-12 * K, err
    for key, C in out.items():
        assert _same(C, first), (key, float((C - first).abs().max()))


def test_solve_bits_across_tile_width(native, monkeypatch):
    """p = 1, N = 1024, m = 128, depth 4: the inverse with the 128-wide tile forced has the bits of
    the 64-wide one"""
    n, m = 1024, 128
    A = generate_matrix(n, "random", 21)

    def solve(tile):
        monkeypatch.setenv("GJ_GLDS_TILE", str(tile))
        native.set_glds_tile(tile)  # (the variable is read once per process)
        try:
            return gj.GaussJordan(block_size=m, device="gpu", depth=4).inverse(A)
        finally:
            native.set_glds_tile(0)

    ref = solve(64)
    assert np.abs(ref @ A - np.eye(n)).max() < 1e-8
    assert np.array_equal(solve(128), ref)
