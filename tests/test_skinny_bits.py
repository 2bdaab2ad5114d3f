"""The bits of the four skinny streaming products on the GPU: ops.panel_rhs, panel_rhs_t, panel_abs_rhs
and panel_abs_rhs_t against SHA-256 digests recorded on an MI355X (tests/golden/skinny_bits.json).

The contract tests (test_rhs_block_ops.py, test_rhs_trans_ops.py, test_abs_ops.py) bound the error of
these ops; this one pins the exact result, so a change to their kernels that claims "same bits" is
checked to have them.  The digests are recorded by running this file as a script at the commit whose
bits are to be kept:

    python tests/test_skinny_bits.py --record

Cases.  (n, m, p, rank) = (300, 16, 1, 0) and (1003, 59, 3, 1): a partial row tile and local padding
rows, a K tail that is no multiple of 16, m no multiple of the 4-row K step of the transposed
products, more than one slice.  k in {1, 17, 64} (the three column widths), both dtypes, P 16-byte
aligned and not (the vec and the scalar kernels), the split forced to 1 and 7 and reset afterwards, so
nothing depends on the CU count.  panel_rhs runs three variants: plain, C_in with sign = -1, and an
active mask with a zero in it.

Operands come from a fixed numpy seed and are interior views of NaN-filled parents (the method of
test_abs_ops.py): what is never read holds NaN.  Hashed are the contiguous bytes of Y (the local rows
x k) or S (n x k) and of colmax; the outputs start from a sentinel, so a column that is not written
enters the digest as the sentinel.
"""
import functools
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinny_bits.json")
SENT = -777.25
SHAPES = [(300, 16, 1, 0), (1003, 59, 3, 1)]
KS = [1, 17, 64]
DTYPES = ["fp64", "fp32"]
SPLITS = [1, 7]
OPS = ["panel_rhs", "panel_rhs_t", "panel_abs_rhs", "panel_abs_rhs_t"]
RHS_VARIANTS = ["plain", "cin_neg", "active"]
_TD = {"fp64": torch.float64, "fp32": torch.float32}


def _layout(n, m, p, rank):
    Nr = (n + m - 1) // m
    nblk = Nr // p + (1 if rank < Nr % p else 0)
    rows = nblk * m
    loc = np.arange(rows)
    grow = ((loc // m) * p + rank) * m + loc % m
    return dict(npad=Nr * m, rows=rows, grow=grow, real=grow < n)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt):
    """P (rows x n, mixed signs, graded columns), V (n x 64) and C (rows x 64) from a fixed seed"""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rng = np.random.default_rng([53, n, m, p, rank])
    P = rng.uniform(-1, 1, (L["rows"], n)) * np.ldexp(1.0, (np.arange(n) * 7) % 21 - 10)[None, :]
    V = rng.uniform(-1, 1, (n, 64)) * np.ldexp(1.0, (np.arange(64) * 5) % 17 - 8)[None, :]
    C = rng.uniform(-1, 1, (L["rows"], 64)) * np.ldexp(1.0, (np.arange(64) * 3) % 11 - 5)[None, :]
    if dt == "fp32":
        P = P.astype(np.float32).astype(np.float64)
    for x in (P, V, C):
        x.setflags(write=False)
    return P, V, C


def _embed(t, r0, c0, ld, fill, extra_rows=9):
    """t as an interior view of a `fill`-filled parent with leading dimension ld, on the GPU"""
    rows, cols = t.shape
    parent = torch.full((rows + r0 + extra_rows, ld), fill, dtype=t.dtype)
    parent[r0:r0 + rows, c0:c0 + cols] = t
    parent = parent.to("cuda")
    return parent, parent[r0:r0 + rows, c0:c0 + cols]


@functools.lru_cache(maxsize=2)
def _place_P(shape, dt, aligned):
    """the panel (rows x npad; the columns >= n and the local padding rows NaN), 16-byte aligned or not"""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    rows, npad = L["rows"], L["npad"]
    es = 8 if dt == "fp64" else 4
    Pfull = np.full((rows, npad), np.nan)
    Pfull[:, :n] = _operands(shape, dt)[0]
    Pfull[~L["real"], :] = np.nan
    if aligned:
        c0, ldp = 16 // es * 2, -(-(npad + 24) // 4) * 4
    else:
        c0, ldp = 5, (npad + 11) | 1
    Ppar, Pv = _embed(torch.from_numpy(Pfull).to(_TD[dt]), 3, c0, ldp, float("nan"))
    assert (Pv.data_ptr() % 16 == 0 and (Pv.stride(0) * es) % 16 == 0) == aligned
    return Ppar, Pv


def _place_V(shape, dt, k, owned_only):
    """V in natural row order: the rows >= n NaN, and for the transposed products the rows of other ranks"""
    n, m, p, rank = shape
    L = _layout(n, m, p, rank)
    V = _operands(shape, dt)[1]
    Vfull = np.full((L["npad"], k), np.nan)
    idx = L["grow"][L["real"]] if owned_only else np.arange(n)
    Vfull[idx] = V[idx, :k]
    return _embed(torch.from_numpy(Vfull), 2, 3, k + 7, float("nan"))


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _rows_product(op, shape, k, dt, aligned, split, variant):
    """panel_rhs / panel_abs_rhs: the digest of Y over the local rows and of colmax"""
    native = gj.load_native()
    n, m, p, rank = shape
    rows = _layout(n, m, p, rank)["rows"]
    _, Pv = _place_P(shape, dt, aligned)
    _, Vv = _place_V(shape, dt, k, owned_only=False)
    _, Yv = _embed(torch.full((rows, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT)
    cm = torch.full((k + 16,), SENT, dtype=torch.float64, device="cuda")[8:8 + k]
    Cv = None
    if variant == "cin_neg" or op == "panel_abs_rhs":
        _, Cv = _embed(torch.from_numpy(_operands(shape, dt)[2][:, :k].copy()), 1, 2, k + 3, float("nan"))
    native.set_rhs_splitk(split)
    try:
        if op == "panel_abs_rhs":
            ops.panel_abs_rhs(Pv, Vv, Yv, n, m, p, rank, C_in=Cv, colmax=cm, ncols=k)
        else:
            active = None
            if variant == "active":  # a zero in it: every third column off, the first included
                active = torch.tensor([0 if j % 3 == 0 else 1 for j in range(k)], dtype=torch.int32, device="cuda")
            ops.panel_rhs(Pv, Vv, Yv, n, m, p, rank, C_in=Cv, sign=-1.0 if variant == "cin_neg" else 1.0,
                          active=active, colmax=cm, ncols=k)
    finally:
        native.set_rhs_splitk(0)
    return _sha(Yv, cm)


def _cols_product(op, shape, k, dt, aligned, split):
    """panel_rhs_t / panel_abs_rhs_t: the digest of S over its n written rows"""
    native = gj.load_native()
    n, m, p, rank = shape
    npad = _layout(n, m, p, rank)["npad"]
    _, Pv = _place_P(shape, dt, aligned)
    _, Vv = _place_V(shape, dt, k, owned_only=True)
    _, Sv = _embed(torch.full((npad, k), SENT, dtype=torch.float64), 8, 5, k + 13, SENT)
    native.set_rhs_t_split(split)
    try:
        getattr(ops, op)(Pv, Vv, Sv, n, m, p, rank, ncols=k)
    finally:
        native.set_rhs_t_split(0)
    return _sha(Sv[:n])


def _digests(op):
    """case id -> digest, over every case of one op"""
    out = {}
    for shape, dt, aligned, k, split in itertools.product(SHAPES, DTYPES, [True, False], KS, SPLITS):
        cid = f"n{shape[0]}m{shape[1]}p{shape[2]}r{shape[3]}-{dt}-{'vec' if aligned else 'scalar'}-k{k}-split{split}"
        if op == "panel_rhs":
            for variant in RHS_VARIANTS:
                out[f"{cid}-{variant}"] = _rows_product(op, shape, k, dt, aligned, split, variant)
        elif op == "panel_abs_rhs":
            out[cid] = _rows_product(op, shape, k, dt, aligned, split, "plain")
        else:
            out[cid] = _cols_product(op, shape, k, dt, aligned, split)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_same_bits(op):
    with open(GOLDEN) as f:
        want = json.load(f)[op]
    got = _digests(op)
    assert set(got) == set(want)
    differ = sorted(c for c in got if got[c] != want[c])
    assert not differ, f"{len(differ)} of {len(got)} cases differ from the recorded bits: {differ[:8]}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_skinny_bits.py --record")
    assert torch.cuda.is_available(), "the digests are recorded on the GPU"
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    rec = {op: _digests(op) for op in OPS}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in rec.values())} digests to {GOLDEN}")
