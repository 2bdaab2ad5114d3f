"""Device::block_inverse at the edges of its contract (csrc/include/gj/device.hpp), on the host executor
and on every GPU kernel family:

  A  the singularity test `|pivot| < thresh` exactly at and one ulp below the threshold, at pivot
     positions that cover the first / last column of a panel, column m - 1 and the ragged tail;
  B  the score is the inf-norm of the inverse that was written, to the rounding of an fp64 sum;
  C  the inverse against numpy within the first-order forward-error bound m u kappa max|ref|
     (Higham, Accuracy and Stability of Numerical Algorithms, section 14.4, constant 1);
  D  the engine applies eps * ||A||_inf with the same edge (CLI, exit code and message).

Every output buffer carries one guard candidate behind it, pre-filled with a sentinel."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj

F64, F32 = torch.float64, torch.float32
BOTH = [F64, F32]
_DT = {F64: "fp64", F32: "fp32"}
_NP = {F64: np.float64, F32: np.float32}
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24}  # unit roundoff
SENT = -777.25  # exact in fp32 and fp64, never produced by the inputs below
PANEL = 16  # column panel width of the matrix-core and blocked families
_devices = {}

# (variant, m, dtypes, groups, reduced positions): one launch per row and group; the comment names the
# GPU kernel the row reaches (the host executor has one implementation and runs the same shapes)
FAMILIES = [
    ("panel", 16, BOTH, "AB", False),  # register sweep <32>
    ("panel", 17, BOTH, "AB", False),  # matrix-core panels, ragged and full
    ("panel", 37, BOTH, "AB", False),
    ("panel", 64, BOTH, "AB", False),
    ("panel", 128, BOTH, "AB", False),
    ("panel", 200, [F64], "AB", False),  # L2-image kernel
    ("panel", 256, [F64], "AB", False),
    ("panel", 200, [F32], "AB", False),  # register sweep <256,1024>
    ("sweep", 37, BOTH, "AB", False),  # register sweep <64> / <128>
    ("sweep", 64, BOTH, "AB", False),
    ("sweep", 100, BOTH, "AB", False),
    ("co", 33, [F64], "AB", False),  # co-resident kernel
    ("co", 100, [F64], "AB", False),
    ("co", 128, [F64], "AB", False),
    ("generic", 300, BOTH, "AB", False),  # per-step global sweep
    ("blocked", 300, BOTH, "AB", False),  # RPT 2 / PB 16
    ("blocked", 520, BOTH, "AB", False),  # RPT 3 / PB 8
    ("blocked", 1030, [F64], "A", True),  # RPT 6 / PB 4
    ("blocked", 2050, [F64], "A", True),  # RPT 12 / PB 2
    ("huge", 300, BOTH, "AB", True),  # kPB = 32 panels
    ("huge", 520, BOTH, "AB", True),
]


def _cases(group):
    out = []
    for variant, m, dts, groups, reduced in FAMILIES:
        if group not in groups:
            continue
        for dt in dts:
            for ex in ("cpu", "gpu"):
                if ex == "cpu" and m > 1000:
                    continue
                marks = [pytest.mark.gpu] if ex == "gpu" else []
                out.append(pytest.param(ex, variant, m, dt, reduced, marks=marks, id=f"{variant}-{m}-{_DT[dt]}-{ex}"))
    return out


def _dev(ex):
    if ex not in _devices:
        C = gj.load_native()
        _devices[ex] = C.host_device(0) if ex == "cpu" else C.hip_device(0)
    return _devices[ex]


def _t(arr, ex):
    t = torch.from_numpy(np.ascontiguousarray(arr)).clone()  # never the caller's memory
    if ex == "gpu":
        t = t.cuda()
        torch.cuda.synchronize()
    return t


def _run(ex, variant, dtype, W, thresh):
    """One block_inverse launch over the candidates W[b] (m x m, row-major, the tested dtype).  Returns
    (inverses [b] as fp64 m x m, scores, valid) of the nblk candidates; the guard candidate behind each
    output buffer must come back untouched."""
    nblk, m = W.shape[0], W.shape[1]
    assert W.dtype == _NP[dtype]
    Lt = _t(-W.reshape(nblk * m, m).T, ex)
    inv_t = _t(np.full((nblk + 1, m, m), SENT, _NP[dtype]), ex)
    scores = _t(np.full(nblk + 1, SENT, np.float64), ex)
    valid = _t(np.full(nblk + 1, -7, np.int32), ex)
    used = _t(np.zeros(nblk, np.int32), ex)
    C = gj.load_native()
    C.set_block_inverse_variant(variant)
    try:
        _dev(ex).block_inverse(_DT[dtype], Lt.data_ptr(), nblk * m, inv_t.data_ptr(), scores.data_ptr(),
                               valid.data_ptr(), used.data_ptr(), nblk * m, m, 1, 0, thresh, -1)
        if ex == "gpu":
            torch.cuda.synchronize()
    finally:
        C.set_block_inverse_variant("panel")
    inv_t, scores, valid = inv_t.cpu().numpy(), scores.cpu().numpy(), valid.cpu().numpy()
    assert (inv_t[nblk] == SENT).all() and scores[nblk] == SENT and valid[nblk] == -7, "guard candidate written"
    return inv_t[:nblk], scores[:nblk], valid[:nblk]


def _reference(Wb):
    """(inverse, kappa_inf) of the block as its dtype holds it, in fp64."""
    W64 = Wb.astype(np.float64)
    ref = np.linalg.inv(W64)
    kappa = np.abs(W64).sum(1).max() * np.abs(ref).sum(1).max()
    assert kappa < 1e4, kappa  # the inputs are meant to be well conditioned
    ref.setflags(write=False)
    return ref, kappa


def _check_accuracy(got_t, ref, kappa, m, dtype, what):
    """Group C: got_t is the block's inv_t (the inverse transposed)."""
    got = got_t.astype(np.float64).T
    err = np.abs(got - ref).max()
    bound = m * UNIT[dtype] * kappa * np.abs(ref).max()
    assert err <= bound, (what, err, bound, err / bound)


# ------------------------------------------------------------------ group A: the threshold boundary
THRESH = 0.75  # exact in both dtypes


def _positions(m, reduced):
    if m > 2048:  # fewer candidates, to keep the case at a few seconds: both columns of a PB = 2 panel
        pos = [0, 1, 32, m // 2, m - 1]
    elif reduced:
        pos = [0, 1, 2, 31, 32, m // 2, m - 1]
    else:
        pos = [0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, m // 2, m - 2, m - 1]
    return sorted({j for j in pos if 0 <= j < m})


def tri_block(rng, m, dtype, jstar, value):
    """A row-shuffled upper triangular block: in column j the only non-zero among the rows not yet
    pivoted is the diagonal entry d_j, in a row that no earlier step has modified (its multipliers
    were exact zeros), so partial pivoting meets d_j at step j bit for bit in any kernel."""
    U = np.triu(rng.uniform(-1.0, 1.0, size=(m, m)) * 0.5 / m, 1)
    U[np.arange(m), np.arange(m)] = rng.uniform(1.0, 2.0, size=m) * rng.choice([-1.0, 1.0], size=m)
    U = U.astype(_NP[dtype])
    if jstar is not None:
        U[jstar, jstar] = value
    return U[rng.permutation(m)]


@functools.lru_cache(maxsize=2)
def _group_a(m, dtype, reduced):
    """(W, expected valid, {b: (ref, kappa)} of the valid candidates): per position one candidate whose
    pivot j* is +-thresh and one with the next number towards 0, then two controls."""
    rng = np.random.default_rng(1000 + m)
    npdt = _NP[dtype]
    below = np.nextafter(npdt(THRESH), npdt(0))
    assert npdt(THRESH) == THRESH and below < THRESH and below.dtype == npdt
    blocks, expect = [], []
    for i, j in enumerate(_positions(m, reduced)):
        sign = npdt(1 if i % 2 == 0 else -1)
        blocks += [tri_block(rng, m, dtype, j, sign * npdt(THRESH)), tri_block(rng, m, dtype, j, sign * below)]
        expect += [1, 0]
    blocks += [tri_block(rng, m, dtype, None, None), tri_block(rng, m, dtype, None, None)]
    expect += [1, 1]
    W = np.stack(blocks)
    W.setflags(write=False)
    refs = {b: _reference(W[b]) for b, e in enumerate(expect) if e}
    return W, np.array(expect, np.int32), refs


@pytest.mark.parametrize("ex,variant,m,dtype,reduced", _cases("A"))
def test_threshold_boundary(ex, variant, m, dtype, reduced):
    """valid = (|pivot| >= thresh) with the pivot exactly at thresh and one ulp below it."""
    W, expect, refs = _group_a(m, dtype, reduced)
    inv_t, _, valid = _run(ex, variant, dtype, W, THRESH)
    assert valid.tolist() == expect.tolist(), np.flatnonzero(valid != expect).tolist()
    for b, (ref, kappa) in refs.items():
        _check_accuracy(inv_t[b], ref, kappa, m, dtype, b)
    if m % PANEL and m < 1000:
        # the same batch times 8 (exact) against thresh 6: a padded column, whose pivot is 1 or where
        # there is nothing to choose, must not make a candidate singular when thresh > 1 (the two
        # m > 1000 rows keep to one launch: their kernel is the blocked family's, covered at 300 / 520)
        _, _, valid8 = _run(ex, variant, dtype, W * _NP[dtype](8), 8 * THRESH)
        assert valid8.tolist() == expect.tolist(), np.flatnonzero(valid8 != expect).tolist()


# ------------------------------------------------------------------ group B: the score
def dom_block(rng, m, dtype, r):
    """randn + 2 sqrt(m) I with column r times 2^-6 (exact): row r of the inverse is 64 times larger
    than without the scaling and is the maximum row by a wide margin."""
    B = (rng.standard_normal((m, m)) + 2.0 * np.sqrt(m) * np.eye(m)).astype(_NP[dtype])
    B[:, r] *= _NP[dtype](2.0 ** -6)
    return B


@functools.lru_cache(maxsize=2)
def _group_b(m, dtype):
    rng = np.random.default_rng(2000 + m)
    rows = sorted({r for r in [0, 1, 15, 16, 63, 64, 255, 256, m - 1] if 0 <= r < m})
    W = np.stack([dom_block(rng, m, dtype, r) for r in rows])
    W.setflags(write=False)
    refs = [_reference(W[b]) for b in range(len(rows))]
    for r, (ref, _) in zip(rows, refs):  # the reference side: row r is the clear maximum
        sums = np.abs(ref).sum(1)
        assert sums.argmax() == r and np.sort(sums)[-2] <= 0.25 * sums[r], (r, sums.argmax())
    return W, rows, refs


@pytest.mark.parametrize("ex,variant,m,dtype,reduced", _cases("B"))
def test_score_is_norm_of_written_inverse(ex, variant, m, dtype, reduced):
    """score = max_i sum_j |inv[i][j]| of the stored inverse.  Both sides sum m non-negative terms in
    fp64, each within (m - 1) 2^-53 of the exact sum: they differ by at most 2 m 2^-53 score, in
    fp32 as in fp64."""
    W, rows, refs = _group_b(m, dtype)
    inv_t, scores, valid = _run(ex, variant, dtype, W, 1e-12)
    assert valid.tolist() == [1] * len(rows)
    for b, r in enumerate(rows):
        sums = np.abs(inv_t[b].astype(np.float64).T).sum(1)
        assert sums.argmax() == r, (r, int(sums.argmax()))
        assert abs(scores[b] - sums.max()) <= 2 * m * 2.0 ** -53 * scores[b], (r, scores[b], sums.max(),
                                                                             scores[b] / sums.max() - 1)
        _check_accuracy(inv_t[b], *refs[b], m, dtype, r)


# ------------------------------------------------------------------ group D: the engine's eps * ||A||_inf
N, M, EPS = 100, 32, 0.125


def _edge_matrix(jstar):
    """(A, ||A||_inf / 8) with A[j*, j*] on the threshold: upper triangular in multiples of 2^-6, so
    every row sum, and with it the norm, is exact in fp32 and fp64 in any order; rows shuffled within
    each block row only, so the block rows below the diagonal stay all-zero (invalid) candidates and
    the diagonal block reaches its inverse unmodified."""
    rng = np.random.default_rng(3000 + jstar)
    U = np.triu(rng.integers(-1, 2, size=(N, N)).astype(np.float64) / 64, 1)
    U[np.arange(N), np.arange(N)] = rng.integers(64, 129, size=N) / 64
    norm = np.abs(np.delete(U, jstar, 0)).sum(1).max()
    edge = norm / 8
    U[jstar, jstar] = edge
    sums = np.abs(U).sum(1)
    assert sums.max() == norm and sums[jstar] < norm  # row j* is not the maximum row
    assert edge * 512 == int(edge * 512) and np.float32(edge) == edge and EPS * norm == edge
    A = U.copy()
    for r0 in range(0, N, M):
        r1 = min(r0 + M, N)
        A[r0:r1] = U[r0 + rng.permutation(r1 - r0)]
    return A, edge


def _gj(gj_bin, ex, dtype, path):
    p = subprocess.run([gj_bin, "--device", ex, "--dtype", _DT[dtype], "--eps", str(EPS), str(N), str(M), str(path)],
                       capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("ex", [pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("jstar", [0, 37, 99])  # the first block, a middle block, the ragged last block
def test_engine_threshold_edge(gj_bin, tmp_path, ex, dtype, jstar):
    A, edge = _edge_matrix(jstar)
    perm_row = int(np.flatnonzero(A[:, jstar] == edge)[0])
    npdt = _NP[dtype]
    for name, value in (("at", npdt(edge)), ("below", np.nextafter(npdt(edge), npdt(0)))):
        Av = A.copy()
        Av[perm_row, jstar] = value
        assert Av[perm_row, jstar].astype(npdt) == value and np.abs(Av).sum(1).max() == 8 * edge
        f = tmp_path / f"{name}.txt"
        np.savetxt(f, Av, fmt="%.17g")  # enough digits to round-trip
        rc, out, err = _gj(gj_bin, ex, dtype, f)
        if name == "at":
            assert rc == 0, (out[-200:], err[-500:])
            res = float(out.strip().split("\n")[-1].split()[1])
            kappa = np.linalg.cond(Av, np.inf)
            assert res <= N * UNIT[dtype] * kappa, (res, N * UNIT[dtype] * kappa)
        else:
            assert rc == 2, (rc, out[-200:], err[-500:])
            assert out.endswith("singular matrix\n"), out[-200:]
